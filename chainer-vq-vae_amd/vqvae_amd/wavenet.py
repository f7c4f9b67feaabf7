"""WaveNet decoder -- mirrors the reference's WaveNet/modules.py class for class
(ResidualBlock modules.py:7-74, ResidualNet 77-110, WaveNet 113-160) with the
same constructor and call signatures.  The per-block graph of ~10 Chainer
functions (dilated conv, crop, 1x1 conv, add, split, tanh, sigmoid, mul, two
1x1 convs, add) is one fused FunctionNode backed by vqvae_resblock_fwd/bwd.

The queue-based incremental generation (modules.py:58-74, 98-110, 232-255) is exposed at the
WaveNet level -- initialize(n) / generate(x, condition) / generate_sequence(...) -- with the
per-block push/pop fused into one device-side step (generation.py, csrc/generate.hip).
"""
import ctypes as C
from collections import namedtuple
from functools import partialmethod

import numpy as np

from . import _lib, backend, core, functions as F, links as L
from .backend import DeviceArray
from .core import Chain, ChainList, FunctionNode, type_expect

_S = backend.stream
DIL_WGRAD_GROUP = 5      # blocks per batched dilated-conv weight-gradient launch
PACK_ONCE = True         # weight slabs of the whole chain re-laid once per step (False: per call; test_pack_once_equals_pack_per_call)


def _p(a):
    return None if a is None else a.ptr


def _rb_desc(x, cond, Wd, Ws, dilation):
    B, Cr, T = x.shape[:3]
    Cd, _, K = Wd.shape[:3]
    return _lib.ResblockDesc(B, T, Cr, Cd, Ws.shape[0], cond.shape[1], K, dilation)


def _rb_workspace(desc):
    return backend.workspace(_lib.load().vqvae_resblock_workspace_bytes(C.byref(desc)))


class ResidualBlockFunction(FunctionNode):
    """(x, condition, Wd, bd, Wc, bc, Wr, br, Ws, bs) -> (residual, skip);
    modules.py:30-56 with dropout_zero_rate == 0."""

    def __init__(self, dilation):
        self.dilation = int(dilation)

    def check_type_forward(self, v):
        x, c = v[0], v[1]
        type_expect((x.ndim == 4 and c.ndim == 4, 'ResidualBlock: x, condition must be (B,C,T,1)'),
                    (x.shape[2] == c.shape[2] and x.shape[0] == c.shape[0],
                     'ResidualBlock: x %s and condition %s disagree' % (x.shape, c.shape)),
                    (v[2].shape[1] == x.shape[1], 'ResidualBlock: conv in-channels mismatch'),
                    (v[4].shape[1] == c.shape[1], 'ResidualBlock: condition_dim mismatch'))

    def forward(self, inputs):
        backend.require_device(*inputs)
        x, cond, Wd, bd, Wc, bc, Wr, br, Ws, bs = inputs
        d = _rb_desc(x, cond, Wd, Ws, self.dilation)
        self.desc = d
        prm = _lib.ResblockParams(Wd.ptr, bd.ptr, Wc.ptr, bc.ptr, Wr.ptr, br.ptr, Ws.ptr, bs.ptr)
        res = DeviceArray((d.B, d.Cr, d.T, 1), np.float32)
        skip = DeviceArray((d.B, d.Cs, d.T, 1), np.float32)
        self.gates = DeviceArray((d.B, d.Cd, d.T), np.float32)
        self.z = DeviceArray((d.B, d.Cd // 2, d.T), np.float32)
        ws = _rb_workspace(d)
        _lib.call('vqvae_resblock_fwd', C.byref(d), C.byref(prm), x.ptr, cond.ptr, None, res.ptr,
                  skip.ptr, 0, self.gates.ptr, self.z.ptr, ws.ptr, ws.nbytes, _S())
        self.retain_inputs(tuple(range(10)))
        return res, skip

    def backward(self, indexes, gys):
        ins = [v.data for v in self.get_retained_inputs()]
        x, cond, Wd, bd, Wc, bc, Wr, br, Ws, bs = ins
        d = self.desc
        g_res = None if gys[0] is None else gys[0].data
        g_skip = None if gys[1] is None else gys[1].data
        if g_skip is None:                      # skip unused: treat as zeros
            g_skip = backend.zeros((d.B, d.Cs, d.T, 1))
        prm = _lib.ResblockParams(Wd.ptr, bd.ptr, Wc.ptr, bc.ptr, Wr.ptr, br.ptr, Ws.ptr, bs.ptr)
        gx = DeviceArray(x.shape, np.float32) if 0 in indexes else None
        gc = DeviceArray(cond.shape, np.float32) if 1 in indexes else None
        gp = [DeviceArray(a.shape, np.float32) for a in ins[2:]]
        if g_res is None:                       # residual output unused (last block)
            gp[4] = gp[5] = None
        grd = _lib.ResblockGrads(*[_p(a) for a in gp])
        ws = _rb_workspace(d)
        _lib.call('vqvae_resblock_bwd', C.byref(d), C.byref(prm), x.ptr, cond.ptr, self.gates.ptr,
                  self.z.ptr, _p(g_res), g_skip.ptr, _p(gx), _p(gc), 0, None, C.byref(grd), 0,
                  ws.ptr, ws.nbytes, _S())
        return tuple([gx, gc] + gp)


def _groups(nb, size=_lib.MAX_STACK_GROUP):
    """[lo, hi) block ranges of at most ``size`` blocks (one resstack call each)."""
    return [(lo, min(nb, lo + size)) for lo in range(0, nb, size)]


# one block's parameters: ResidualBlock.param_list is built from it, so this is THE order of every flat list of 8 per block
BlockParams = namedtuple('BlockParams', 'Wd bd Wc bc Wr br Ws bs')


def _per_block(flat):
    """A flat list of eight entries per block (arrays, Variables, gradients) as one BlockParams per block."""
    n = len(BlockParams._fields)
    assert len(flat) % n == 0
    return [BlockParams(*flat[i:i + n]) for i in range(0, len(flat), n)]


def _prm(b):
    return _lib.ResblockParams(*[a.ptr for a in b])


def _value_key(params):
    """The parameters' buffers AND the values in them: pointers, the memory's value versions (backend._Block.wver: in-place
    writes through DeviceArray methods -- Link.copyparams, p.data.set(...) -- and recycled addresses), the load / layout /
    init epochs (serializers, arena adoption, lazily shaped parameters).  Optimizer steps are checked by the caller
    (ResidualNet._forward: a slab set packed ahead is only offered to the forward of the step it was packed in)."""
    return (tuple(p.ptr for p in params), tuple(p.wver for p in params),
            core.param_epoch('load'), core.param_epoch('layout'), core.param_epoch('init'))


def _pack_key(params, d0):
    """What slabs packed ahead (ResidualNet.prepack_async) are valid for: _value_key, the block geometry, the matmul mode."""
    return _value_key(params) + (d0.B, d0.T, d0.Cr, d0.Cd, d0.Cs, d0.Cc, d0.K, _lib.load().vqvae_get_matmul_dtype())


def _owner_steps(pvars):
    """The optimizer step count behind each parameter Variable (optimizers.Adam sets `_owner_step`); None without an owner."""
    out = []
    for v in pvars:
        f = getattr(v, '_owner_step', None)
        out.append(f() if f is not None else None)
    return tuple(set(out)) if len(set(out)) <= 1 else tuple(out)


# The latent-rate condition projection of all blocks as ONE conv: its weight (nb * Cd, Cc, 1, 1) and its bias, which also
# carries the dilated convs' biases (the lerp weights of a column sum to one, so they can ride in the projection:
# vqvae_resblock_cproj::P_has_bd; bd_all: kept alive until the add has run); slab_f / slab_b: the weight packed for the
# forward / backward-data conv over a latent of ``shape`` = (B, Cc, Tl), or None.
CprojPack = namedtuple('CprojPack', 'Wc_all bc_all bd_all slab_f slab_b shape')

# What ResidualNet.prepack_async leaves for the next forward: the keys the projection / the slabs are valid for, every
# block's weight slabs and the bytes per block, the side-stream event behind all of it, a CprojPack or None, the skip
# sum's prepared workspace or None, _owner_steps of the parameters at pack time.
Prepack = namedtuple('Prepack', 'value_key pack_key slabs stride ready cproj skipws owner_steps')


def _build_cproj(blocks, stream):
    """A CprojPack without slabs from the blocks' parameters: three allocations, then the launches on ``stream``."""
    nb, (Cd, Cc) = len(blocks), blocks[0].Wc.shape[:2]
    cp = CprojPack(DeviceArray((nb * Cd, Cc, 1, 1), np.float32), DeviceArray((nb * Cd,), np.float32),
                   DeviceArray((nb * Cd,), np.float32), None, None, None)
    for lo, hi in _groups(nb):
        for dst, name, n in ((cp.Wc_all, 'Wc', Cd * Cc), (cp.bc_all, 'bc', Cd), (cp.bd_all, 'bd', Cd)):
            _lib.call('vqvae_concat', dst.ptr + lo * n * 4, _lib.ptr_array([getattr(b, name) for b in blocks[lo:hi]]),
                      hi - lo, n, stream)
    _lib.call('vqvae_elementwise', 0, nb * Cd, cp.bc_all.ptr, cp.bd_all.ptr, cp.bc_all.ptr, 1.0, 1.0, stream)
    return cp


def _pack_stack(blocks, d0, stream):
    """Every block's weight slabs (forward and backward forms) re-laid for this step (vqvae_resstack_pack): the
    allocation, then the launch on ``stream``.  Returns (slabs, bytes per block)."""
    nb = len(blocks)
    per = _lib.load().vqvae_resstack_packed_bytes(C.byref(d0))
    packed = DeviceArray((nb * per // 4,), np.float32)
    prms = (_lib.ResblockParams * nb)(*[_prm(b) for b in blocks])
    has_res = (C.c_int * nb)(*([1] * (nb - 1) + [0]))
    _lib.call('vqvae_resstack_pack', C.byref(d0), nb, prms, has_res, packed.ptr, packed.nbytes, stream)
    return packed, per


FUSE_PULLBACK = True     # (tests A/B it through this attribute)
DEFER_WGRAD = True
PB_REDUCE_GROUP = 20      # blocks per vqvae_pullback_reduce_into launch (5 while the chain's weight gradients ran 90 us longer per launch; re-measured on the LDS-DMA kernel: 5 / 7 / 10 / 20 -> 14.17 / 14.15 / 14.14 / 14.09 ms per step, two rounds on one box)
DEFER_DIL_BLOCKS = 5      # how many of the blocks nearest the input keep their dilated-conv weight gradients for the side stream (a multiple of DIL_WGRAD_GROUP; 10 and 15 measured 0.05-0.1 ms slower: the tail they would run beside is full)
BATCH_PULLBACK = True
PREPACK_ASYNC = True
# 'bfloat16' mode: the chain's tensors the caller may keep in HBM as bf16 (x_l, gh_l, g_res_l: vqvae_resblock_desc.storage) are
# taken whenever the library offers them; wavenet.BF16_STORAGE = False leaves every one fp32 (operand rounding only: ADVICE r4)
BF16_STORAGE = True


def _grad_out(var, shape):
    """Gradient destination for input ``var``: its slot in the flat gradient arena
    when it is a Parameter that has no gradient yet, else a fresh array."""
    buf = var.grad_buffer() if hasattr(var, 'grad_buffer') else None
    if buf is not None and buf.size == int(np.prod(shape)):
        return buf.reshape(shape)
    return DeviceArray(shape, np.float32)


def _pullback_forms(d0, Tl, f16):
    """How the gh_l of a chain over a latent of Tl positions can be pulled back to the latent rate besides the plain
    per-block launch over an fp32 gh_l: (fused, segmented).  fused: 'float32x2', inside the launch that produces gh_l
    (vqvae_resblock_amax.pb_part: 128 gate channels, T % 128 == 0, T >= 64 Tl; FUSE_PULLBACK = False: not taken).
    segmented: the domain of the kernel behind vqvae_upsample_linear_bwd_blocks / _bf16 / _f16x2 -- the only pull-back
    that reads a STORED gh_l (csrc/misc.hip launch_upsample_bwd_seg)."""
    fused = bool(f16 and FUSE_PULLBACK and _lib.load().vqvae_get_fused_pullback(C.byref(d0)) and d0.T >= 64 * Tl)
    segmented = Tl >= 3 and d0.T >= 8 * Tl and d0.T % 4 == 0 and d0.T // 4 <= 2048
    return fused, segmented


def _plan_storage(descs, packed, f16, Tl=None):
    """vqvae_resblock_desc.storage of every block for the forward and the backward sweep, ([fwd], [bwd]), from one round of
    queries (they depend on a descriptor's geometry only).  Forward, packed chain only: the residual stream between the
    blocks kept as bf16 (BASELINE configs[4], mode 'bfloat16'; the buffers stay fp32-sized, half used) or, with ``f16``
    ('float32x2'), PRE-SPLIT (fp16 hi | lo dwords under an a-priori bound: its three readers stage it with two v_perm_b32
    per element pair instead of splitting it again); and of tanh, sigmoid, z only the last two are saved (the backward
    takes tanh = z / sigmoid).  Backward: those, plus gh_l as bf16 / pre-split and the gradient stream g_res_l = gx_{l+1}
    as bf16.

    The rule: a tensor that crosses from block l to block l + 1 (x_{l+1}; g_res_l = gx_{l+1}) is stored in a format only
    when the library offers that format to BOTH blocks -- the answers differ inside a chain (a dilation beyond the
    sequence is refused pre-split storage) -- and a tensor one block owns (gh_l, the saved gates) from that block's own
    answer.  No kernel reads a stored x_l and writes an fp32 x_{l+1} (rb_formats refuses it), so a block that cannot store
    its output takes the stored stream from every block in front of it: it resumes, from fp32, behind that block.  And
    gh_l is stored only where a pull-back can read it stored (``Tl``: the latent length; _pullback_forms)."""
    nb = len(descs)
    fwd = [0] * nb
    if not packed:
        return fwd, fwd
    lib = _lib.load()
    sup16 = [lib.vqvae_resblock_bf16_storage(C.byref(d)) if BF16_STORAGE else 0 for d in descs]
    supx2 = [lib.vqvae_resblock_f16x2_storage(C.byref(d)) if f16 else 0 for d in descs]
    for sup, xbit, rbit in ((sup16, _lib.STORE_X_BF16, _lib.STORE_RES_BF16), (supx2, _lib.STORE_X_F16X2, _lib.STORE_RES_F16X2)):
        both = [bool(a & xbit and a & rbit) for a in sup]
        stored = [both[l] and both[l + 1] for l in range(nb - 1)]          # x_{l+1}, between block l and block l + 1
        for l in range(nb - 3, -1, -1):                                    # block l + 1 reads x_{l+1} and writes x_{l+2}
            stored[l] = stored[l] and stored[l + 1]
        for l in range(nb - 1):
            if stored[l]:
                fwd[l] |= rbit
                fwd[l + 1] |= xbit
    bwd = list(fwd)
    gh_ok = Tl is not None and any(_pullback_forms(descs[0], Tl, f16))
    for l in range(nb):
        fwd[l] |= supx2[l] & _lib.STORE_GATES_SIG
        bwd[l] |= supx2[l] & _lib.STORE_GATES_SIG
        if gh_ok:
            bwd[l] |= (supx2[l] & _lib.STORE_GH_F16X2) if f16 else (sup16[l] & _lib.STORE_GH_BF16)
    gs = [bool(a & _lib.STORE_GX_BF16 and a & _lib.STORE_GRES_BF16) for a in sup16]
    for l in range(nb - 1):                                                # g_res_l = gx_{l+1}
        if gs[l] and gs[l + 1]:
            bwd[l] |= _lib.STORE_GRES_BF16
            bwd[l + 1] |= _lib.STORE_GX_BF16
    return fwd, bwd


KEEP_CONTRACT_WORDS = False        # tests: keep a host copy of the last sweep's maxima / scale words in LAST_CONTRACT_WORDS
LAST_CONTRACT_WORDS = None


class ChainWords(object):
    """Matmul mode 'float32x2': the absolute maximum of every tensor of the chain travels with it as a group of
    _lib.AMAX_SLOTS device uint32 (float bits) -- groups x_l | gh_l | g_res_l | g_skip; the kernels' epilogues raise the
    words of what they store (atomicMax), only the tensors that arrive from outside are scanned.  Behind them the SCALE
    words of the tensors kept pre-split (vqvae_resblock_desc.storage & VQVAE_STORE_*_F16X2): x_l | gh_l again -- the bound
    each was split under, written by its producer.  One zeroed buffer per step; x(l) ... gh_scale(l) are device addresses."""
    FIRST = {'x': (0, 0), 'gh': (1, 0), 'g_res': (2, 0), 'g_skip': (3, 0), 'x_scale': (3, 1), 'gh_scale': (4, 1)}

    def __init__(self, nb):
        self.nb = nb
        self.buf = backend.zeros(((5 * nb + 1) * _lib.AMAX_SLOTS,), np.uint32)

    @classmethod
    def index(cls, nb, what, l=0):
        """Group number of ``what`` for block l in a chain of nb blocks -- also the row of host()'s table."""
        a, b = cls.FIRST[what]
        return a * nb + b + l

    def _at(self, what, l=0):
        return self.buf.ptr + 4 * _lib.AMAX_SLOTS * self.index(self.nb, what, l)

    x, gh, g_res = partialmethod(_at, 'x'), partialmethod(_at, 'gh'), partialmethod(_at, 'g_res')
    g_skip, x_scale, gh_scale = partialmethod(_at, 'g_skip'), partialmethod(_at, 'x_scale'), partialmethod(_at, 'gh_scale')

    def host(self):
        """(nb, the words as a host table of one row per group): what KEEP_CONTRACT_WORDS keeps."""
        return self.nb, self.buf.get().reshape(-1, _lib.AMAX_SLOTS).copy()


class _Sweep(object):
    """What the phases of one ResidualStackFunction.backward share.  Everything the side stream reads or writes is referenced
    from here or from the node until the join is enqueued or backend.defer_to_side has it (the invariant in backend.py)."""
    __slots__ = ('indexes', 'cond', 'blocks', 'pvars',       # what was asked for; the inputs as arrays / Variables per block
                 'g_skip', 'gh_store', 'hpre',               # the incoming gradient; per block: gh_l's storage bit; gh_l is pre-split
                 'overlap', 'side', 'defer',                 # two-stream sweep and its stream; deferred weight gradients
                 'tb', 'Tl', 'gP', 'pb_part', 'gh_all',      # latent-rate condition: tables, pulled-back gh, its two batched forms
                 'dil_group', 'ws_side', 'ws_defer',         # dilated wgrad blocks per launch; scratch of the two side uses
                 'ghs', 'g_ress', 'g', 'dil_pending')        # per block: gh_l, g_res_l, gradients by name; blocks awaiting dil wgrad

    def grad_out(self, l, name):
        """Destination of block l's gradient ``name`` (see _grad_out), remembered in self.g."""
        a = self.g[l][name] = _grad_out(getattr(self.pvars[l], name), getattr(self.blocks[l], name).shape)
        return a


class ResidualStackFunction(FunctionNode):
    """All blocks of a ResidualNet in one node (modules.py:89-96).
    inputs: (x, condition, then 8 params per block) -> skip_connections.

    MI355X-first restructuring (same math, summation order aside):
      * skip_connections = sum_l skip_l(z_l) is ONE GEMM over K = n_blocks*Cd/2 at the
        end (vqvae_resstack_skip_fwd) instead of n_blocks read-modify-write passes;
      * the last block's unused residual branch is not computed;
      * backward keeps every block's gh in HBM (2.5 GB at B=16 -- 288 GB part) so the
        condition gradient sum_l Wc_l^T gh_l is ONE GEMM over K = n_blocks*Cd, and all
        skip-weight gradients share one launch (g_skip is their common operand)."""

    def __init__(self, dilations, relu_out=False, prepacked=None):
        self.dilations = [int(d) for d in dilations]
        self.prepacked = prepacked       # ResidualNet.prepack_async's Prepack for this step's parameters, or None
        # relu_out: the F.relu WaveNet applies to the skip sum (modules.py:158) in the skip GEMM's epilogue; its backward
        # arrives done when the conv that reads the result masked its gradient (functions.FUSE_RELU_BWD)
        self.relu_out = bool(relu_out)
        # the latent-rate projection (set by _project_condition): its latent shape, conv descriptor, weight, backward slab
        self.cproj_shape = self.pdesc = self.Wc_all = self._cslab_b = None

    def forward(self, inputs):
        backend.require_device(*inputs)
        x, cond = inputs[0], inputs[1]
        blocks = _per_block(inputs[2:])
        assert len(blocks) == len(self.dilations)
        if self.prepacked is not None:      # whatever becomes of the slabs, the main stream is behind the side stream's writes of them
            backend.wait_event(_S(), self.prepacked.ready)
        # The three facts forward and backward branch on, each implying the one before: the condition arrives at the
        # latent rate (self.lat; else materialised), the weight slabs are laid out once for the step (self.packed; else
        # per call), the chain runs matmul mode 3, 'float32x2', and its maxima travel with it (self.words)
        self.lat = cond.latent if isinstance(cond, F.LazyUpsampled) else None                # (B, Cc, Tl)
        pack = self.lat is not None and PACK_ONCE
        f16 = pack and _lib.load().vqvae_get_matmul_dtype() == 3
        self.descs = [_rb_desc(x, cond, b.Wd, b.Ws, dil) for b, dil in zip(blocks, self.dilations)]
        proj = self._project_condition(inputs[2:], blocks, x.shape[2]) if self.lat is not None else None
        self.words = ChainWords(len(blocks)) if f16 else None
        if f16 and getattr(x, 'amax', None) is not None:     # x_0's maximum: it travelled with the tensor, or a scan
            _lib.call('vqvae_memcpy_d2d', self.words.x(0), x.amax.ptr, 4 * _lib.AMAX_SLOTS, _S())
        elif f16:
            _lib.call('vqvae_absmax', x.ptr, x.size, self.words.x(0), _S())
        self.packed, self.packed_stride, self._skipws = self._stack_slabs(inputs[2:], blocks) if pack else (None, 0, None)
        self.pullback = _pullback_forms(self.descs[0], self.lat.shape[2], f16) if self.lat is not None else (False, False)
        self.storage = _plan_storage(self.descs, pack, f16, self.lat.shape[2] if self.lat is not None else None)
        self.saved = []
        h = x
        for i, b in enumerate(blocks):
            self.descs[i].storage = self.storage[0][i]
            res, gates, z = self._block_forward(i, h, cond, b, proj)
            self.saved.append((h, gates, z))
            h = res
        skip = self._skip_sum(blocks)
        self.retain_inputs(tuple(range(len(inputs))))
        return skip,

    def _project_condition(self, params, blocks, T):
        """The condition projection of every block at the latent rate, one conv (see vqvae_resblock_cproj in the header).
        Its weight / bias (the dilated convs' biases ride in the latter: the gate kernels then add no bias, and their
        condition term is one more step of the contraction -- vqvae_resblock_cproj::P_has_bd / P_amax) and its packed
        slabs were built on the side stream by ResidualNet.prepack_async when the step started, if the parameters are the
        ones it saw; else they are built here, without slabs.  Returns (P_all, P_amax, lerp tables, the CprojPack)."""
        B, Cc, Tl = self.cproj_shape = tuple(self.lat.shape)
        nb, Cd = len(blocks), blocks[0].Wd.shape[0]
        pre = self.prepacked
        cp = pre.cproj if (pre is not None and pre.value_key == _value_key(params)) else None
        slab_f = None
        if cp is None:
            cp = _build_cproj(blocks, _S())
        elif cp.shape == (B, Cc, Tl):
            slab_f, self._cslab_b = cp.slab_f, cp.slab_b
        self.Wc_all = cp.Wc_all
        self.pdesc = _lib.Conv1dDesc(B, Cc, Tl, nb * Cd, Tl, 1, 1, 0, 1, 0)
        P_all = DeviceArray((B, nb * Cd, Tl), np.float32)
        P_amax = backend.new_amax()
        ws = backend.workspace(_lib.load().vqvae_conv1d_workspace_bytes(C.byref(self.pdesc)))
        _lib.call('vqvae_conv1d_fwd_amax', C.byref(self.pdesc), self.lat.ptr, self.Wc_all.ptr, cp.bc_all.ptr,
                  P_all.ptr, ws.ptr, ws.nbytes, C.byref(_lib.Conv1dAmax(None, None, P_amax.ptr, _p(slab_f))), _S())
        return P_all, P_amax, F.resize_tables(Tl, T), cp

    def _stack_slabs(self, params, blocks):
        """(slabs, bytes per block, prepared skip-sum workspace or None): every block's weight slabs, as packed on the side
        stream while the encoder / quantiser / condition embed ran (ResidualNet.prepack_async; with them the skip sum's
        slabs / bias sums, vqvae_resstack_skip_prepare) if they are valid for this call, else re-laid here."""
        d0, pre = self.descs[0], self.prepacked
        if pre is not None and pre.pack_key == _pack_key(params, d0):
            return pre.slabs, pre.stride, pre.skipws
        return _pack_stack(blocks, d0, _S()) + (None,)

    def _block_forward(self, i, h, cond, b, proj):
        """Block i on input h -> (residual output or None for the last block, gates, z)."""
        d, nb = self.descs[i], len(self.descs)
        last = i == nb - 1
        prm = _prm(b)
        res = None if last else DeviceArray((d.B, d.Cr, d.T, 1), np.float32)
        gates = DeviceArray((d.B, d.Cd, d.T), np.float32)
        z = DeviceArray((d.B, d.Cd // 2, d.T), np.float32)
        ws = _rb_workspace(d)
        if proj is None:
            _lib.call('vqvae_resblock_fwd', C.byref(d), C.byref(prm), h.ptr, cond.ptr, None,
                      _p(res), None, 0, gates.ptr, z.ptr, ws.ptr, ws.nbytes, _S())
            return res, gates, z
        P_all, P_amax, tb = proj[:3]
        Tl = self.lat.shape[2]
        cp = _lib.ResblockCproj(P_all.ptr + i * d.Cd * Tl * 4, nb * d.Cd * Tl, Tl,
                                tb['v0'].ptr, tb['w0'].ptr, tb['w1'].ptr, 1, P_amax.ptr)
        if self.packed is None:
            _lib.call('vqvae_resblock_fwd', C.byref(d), C.byref(prm), h.ptr, None, C.byref(cp),
                      _p(res), None, 0, gates.ptr, z.ptr, ws.ptr, ws.nbytes, _S())
            return res, gates, z
        am, w = None, self.words
        if w is not None:       # (a pre-split x_l is read under its scale words; its maximum goes on as x_max)
            xpre = bool(d.storage & _lib.STORE_X_F16X2)
            am = C.byref(_lib.ResblockAmax(
                w.x_scale(i) if xpre else w.x(i), None if last else w.x(i + 1), None, None, None, None,
                w.x(i), None if last else w.x_scale(i + 1), None))
        _lib.call('vqvae_resblock_fwd_packed', C.byref(d), C.byref(prm), h.ptr, C.byref(cp),
                  _p(res), gates.ptr, z.ptr, ws.ptr, ws.nbytes,
                  self.packed.ptr + i * self.packed_stride, am, _S())
        return res, gates, z

    def _skip_sum(self, blocks):
        d, nb = self.descs[0], len(self.descs)
        skip = DeviceArray((d.B, d.Cs, d.T, 1), np.float32)
        if self.words is not None:
            skip.amax = backend.new_amax()       # published by the skip sum's epilogue: the next conv's operand scale
        for lo, hi in _groups(nb):
            n = hi - lo
            zs = _lib.ptr_array([s[2] for s in self.saved[lo:hi]])
            if self._skipws is not None and n == nb:       # slabs and bias sums were prepared ahead (prepack_async): the GEMM only
                _lib.call('vqvae_resstack_skip_fwd_prepared', C.byref(d), n, zs, skip.ptr, 0, 1 if self.relu_out else 0,
                          self._skipws.ptr, self._skipws.nbytes, _p(skip.amax), _S())
                continue
            ws = backend.workspace(_lib.load().vqvae_resstack_workspace_bytes(C.byref(d), n))
            _lib.call('vqvae_resstack_skip_fwd', C.byref(d), n, _lib.ptr_array([b.Ws for b in blocks[lo:hi]]),
                      _lib.ptr_array([b.bs for b in blocks[lo:hi]]), zs, skip.ptr,
                      0 if lo == 0 else 1, 1 if (self.relu_out and hi == nb) else 0, ws.ptr, ws.nbytes, _p(skip.amax), _S())
        skip.relu_out = self.relu_out
        self._skip = skip if self.relu_out else None
        return skip

    def _check_contract(self, hpre):
        """'float32x2': every pre-split tensor of this sweep -- x_l (l >= 1) and the gh_l with `hpre[l]` -- against the bound it was
        split under (backend.f32x2_contract_violations; one launch, no host round trip unless backend.contract_debug())."""
        w, nb = self.words, len(self.descs)
        pairs = [(w.x_scale(l), w.x(l)) for l in range(1, nb) if self.descs[l].storage & _lib.STORE_X_F16X2]
        pairs += [(w.gh_scale(l), w.gh(l)) for l in range(nb) if hpre[l]]
        if not pairs:
            return
        global LAST_CONTRACT_WORDS
        if KEEP_CONTRACT_WORDS and backend._state.get('arena') is None:           # (tests: the words themselves, per block)
            backend.synchronize()
            LAST_CONTRACT_WORDS = w.host()
        sc = (C.c_void_p * len(pairs))(*[p[0] for p in pairs])
        am = (C.c_void_p * len(pairs))(*[p[1] for p in pairs])
        rep = backend.contract_report()
        _lib.call('vqvae_f32x2_contract_check', len(pairs), sc, am, backend.CONTRACT_LOG2_LIMIT, rep.ptr, _S())
        if backend.contract_debug() and backend._state.get('arena') is None:      # (never inside a recording: the read synchronises)
            r = backend.f32x2_contract_violations()
            before, backend._state['contract_seen'] = backend._state.get('contract_seen', 0), r['violations']
            if r['violations'] > before:
                raise FloatingPointError(
                    "float32x2: a pre-split tensor of ResidualNet's chain was split under a bound 2^%.1f above its maximum "
                    "(limit 2^%d, %d violation(s) so far): outside the mode's dynamic-range contract (DESIGN.md 3a) -- use "
                    "set_matmul_dtype('float32x3') or backend.set_presplit(4)" % (r['worst_log2'], r['log2_limit'], r['violations']))

    def backward(self, indexes, gys):
        """The sweep as a schedule.  Two streams: the backward-data chain (gz -> gh -> gx, block by block) is serial and
        each of its kernels leaves a residency tail (1920 workgroups on 1024 slots); the weight gradients of block l only
        need gh_l, so they -- and the pull-back of gh_l to the latent rate -- run on the side stream and fill those tails."""
        s = self._begin_sweep(indexes, gys)
        self._size_workspaces(s)
        self._skip_wgrad(s)
        nb, g_res = len(self.descs), None
        for i in range(nb - 1, -1, -1):
            g_res = self._block_backward(s, i, g_res)          # gx of block i is g_res of block i - 1
            if self.lat is not None:
                self._block_side_work(s, i)
        if s.defer:
            # The weight gradients still due when the chain has reached the first block -- the last group of dilated-conv
            # gradients and every res conv's -- need nothing that comes later, and what comes later is the latent-rate tail
            # of the backward pass (~70 launches of 5-30 us on a handful of workgroups each, 0.7 ms of an all but idle chip).
            # They run BESIDE that tail on the side stream; Variable.backward() joins the streams (backend.join_side)
            sd = backend.side_stream()
            backend.wait_event(sd, backend.Event().record(_S()))       # every gh, g_res of the chain is complete
            self._dil_wgrad(s, sd, s.ws_defer)
            self._res_wgrad(s, sd, s.ws_defer)
            backend.defer_to_side([self.saved, s.ghs, s.g_ress, s.g, s.ws_defer, self.packed, self.words, s.g_skip],
                                  writes=[g[n] for g in s.g for n in ('Wd', 'bd', 'Wr', 'br')])
        else:
            self._res_wgrad(s, _S(), None)
        if s.overlap:
            # join: what the main stream (and the caller, after backward returns) issues from here is behind the side stream
            backend.wait_event(_S(), backend.Event().record(s.side))
        gcond = None
        if self.lat is not None:
            gcond = self._cproj_backward(s)
        elif 1 in indexes:
            gcond = self._gcond_backward(s)
        if self.words is not None:
            self._check_contract(s.hpre)
        self.saved = None                      # release activations
        self.packed = None
        self.words = None
        return tuple([g_res if 0 in indexes else None, gcond] + [a for g in s.g for a in BlockParams(**g)])

    def _begin_sweep(self, indexes, gys):
        """The fused ReLU's backward, g_skip's maximum, the backward's storage bits, streams, and the latent-rate
        destinations (gP and the buffers of the two batched pull-back forms)."""
        s = _Sweep()
        in_vars = self.get_retained_inputs()
        s.indexes, s.cond = indexes, in_vars[1].data
        s.pvars, s.blocks = _per_block(in_vars[2:]), _per_block([v.data for v in in_vars[2:]])
        nb, w = len(self.descs), self.words
        g_skip = gys[0].data
        if self.relu_out and not getattr(g_skip, 'relu_masked', False):     # the fused ReLU's backward, unless the reader did it
            g0 = g_skip
            g_skip = F._ew(_lib.EW_RELU_BWD, g0, self._skip)
            g_skip.amax = getattr(g0, 'amax', None)
        s.g_skip = g_skip
        if w is not None:
            if getattr(g_skip, 'amax', None) is not None:
                _lib.call('vqvae_memcpy_d2d', w.g_skip(), g_skip.amax.ptr, 4 * _lib.AMAX_SLOTS, _S())
            else:
                _lib.call('vqvae_absmax', g_skip.ptr, g_skip.size, w.g_skip(), _S())
        for d, bits in zip(self.descs, self.storage[1]):
            d.storage = bits
        s.gh_store = [bits & (_lib.STORE_GH_BF16 | _lib.STORE_GH_F16X2) for bits in self.storage[1]]
        s.hpre = [bool(g & _lib.STORE_GH_F16X2) for g in s.gh_store]
        s.overlap = backend.overlap_enabled()
        s.side = backend.side_stream() if s.overlap else _S()
        s.ghs, s.g_ress, s.dil_pending = [None] * nb, [None] * nb, []
        s.g = [dict.fromkeys(BlockParams._fields) for _ in range(nb)]
        d0 = self.descs[0]
        s.tb = s.Tl = s.gP = s.pb_part = s.gh_all = None
        if self.lat is None:
            return s
        Bl, Cc, s.Tl = self.lat.shape
        s.tb = F.resize_tables(s.Tl, d0.T)
        s.gP = DeviceArray((Bl, nb * d0.Cd, s.Tl), np.float32)
        # 'float32x2': the pull-back of every gh_l to the latent rate runs inside the launch that produces gh_l
        # (vqvae_resblock_amax.pb_part) and a reduce launch finishes PB_REDUCE_GROUP blocks; FUSE_PULLBACK = False: a launch
        # per block.  (Measured in the bf16 mode too: the gate-derivative kernel of that mode loses more than the launch
        # costs -- configs[4] 18.8 -> 20.4 ms -- so it keeps its pull-back launches)
        # -- where the library's gate-derivative launch can carry it (128 gate channels; the 512-channel decoder's gh_l are pulled
        # back by a launch per block on the side stream, below)
        if self.pullback[0]:
            s.pb_part = DeviceArray((nb, d0.B, d0.T // 128, d0.Cd, 4), np.float32)
        # where the pull-back stays a kernel of its own (bf16 mode, float32x3, fp32 MFMA): ONE launch over all blocks' gh when
        # the chain is done (vqvae_upsample_linear_bwd_blocks) instead of a launch per block -- the gh_l then are the
        # slices of one array.  BATCH_PULLBACK = False: a launch per block, as before (same sums in the same order)
        if (BATCH_PULLBACK and s.pb_part is None and self.packed is not None and not s.overlap and not any(s.hpre)
                and len(set(s.gh_store)) == 1
                and self.pullback[1]
                and all((dd.B, dd.Cd, dd.T) == (d0.B, d0.Cd, d0.T) for dd in self.descs)):
            s.gh_all = DeviceArray((nb, d0.B, d0.Cd, d0.T), np.float32)
        return s

    def _size_workspaces(self, s):
        """Side-stream scratch, sized once for everything it will run (never regrown mid-flight), and whether the last
        weight gradients are deferred (DEFER_WGRAD = False: in line)."""
        d0, nb, lib = self.descs[0], len(self.descs), _lib.load()
        # dilated-conv weight gradients: dil_group blocks per launch (each block is filter_size segments of one contraction),
        # so the K splits and their partial slabs are shared by dil_group * 8 output tiles instead of 8
        s.dil_group = max(1, min(DIL_WGRAD_GROUP, _lib.MAX_STACK_GROUP // d0.K))
        need = max(lib.vqvae_resblock_workspace_bytes(C.byref(d0)),
                   lib.vqvae_resstack_workspace_bytes(C.byref(d0), min(nb, _lib.MAX_STACK_GROUP)),
                   lib.vqvae_resstack_dil_wgrad_workspace_bytes(C.byref(d0), min(nb, s.dil_group)))
        s.ws_side = backend.workspace(need, 'side' if s.overlap else 'main')
        s.defer = DEFER_WGRAD and not s.overlap and self.packed is not None
        if s.defer:          # (sized for everything this sweep sends to the side stream before the first of it is enqueued)
            need = max(need, lib.vqvae_conv1d_workspace_bytes(C.byref(self.pdesc)))
        s.ws_defer = backend.workspace(need, 'side') if s.defer else None

    def _skip_wgrad(self, s):
        """Skip-conv weight gradients need only g_skip and the saved z_l: started right away, one launch per group."""
        d0, nb = self.descs[0], len(self.descs)
        gWs = [s.grad_out(l, 'Ws') for l in range(nb)]
        gbs = [s.grad_out(l, 'bs') for l in range(nb)]
        if s.overlap:
            backend.wait_event(s.side, backend.Event().record(_S()))       # g_skip is ready
        for lo, hi in _groups(nb):
            zs = _lib.ptr_array([sv[2] for sv in self.saved[lo:hi]])
            _lib.call('vqvae_resstack_skip_wgrad', C.byref(d0), hi - lo, s.g_skip.ptr, zs,
                      _lib.ptr_array(gWs[lo:hi]), _lib.ptr_array(gbs[lo:hi]), 0, s.ws_side.ptr,
                      s.ws_side.nbytes, self.words.g_skip() if self.words is not None else None, s.side)

    def _block_backward(self, s, i, g_res):
        """Block i's backward-data launch on the main stream (gz, gate derivative -> gh_i, then gx); returns gx.  With a
        materialised condition the same launch also gives the dilated conv's and the condition projection's gradients."""
        d, b, w = self.descs[i], s.blocks[i], self.words
        h, gates, z = self.saved[i]
        prm = _prm(b)
        gx = DeviceArray(h.shape, np.float32) if (i > 0 or 0 in s.indexes) else None
        gWd, gbd = s.grad_out(i, 'Wd'), s.grad_out(i, 'bd')
        s.g_ress[i] = g_res                # None for the last block: residual unused
        if self.lat is None:
            grd = _lib.ResblockGrads(gWd.ptr, gbd.ptr, s.grad_out(i, 'Wc').ptr, s.grad_out(i, 'bc').ptr, *([None] * 4))
        gh = s.ghs[i] = (DeviceArray((d.B, d.Cd, d.T), np.float32) if s.gh_all is None else
                         s.gh_all.flat_view(i * d.B * d.Cd * d.T, d.B * d.Cd * d.T, (d.B, d.Cd, d.T)))
        ws = _rb_workspace(d)
        if self.lat is None:
            _lib.call('vqvae_resblock_bwd', C.byref(d), C.byref(prm), h.ptr, s.cond.ptr, gates.ptr,
                      z.ptr, _p(g_res), s.g_skip.ptr, _p(gx), None, 0, gh.ptr, C.byref(grd), 0,
                      ws.ptr, ws.nbytes, _S())
        elif self.packed is None:
            none = _lib.ResblockGrads(*([None] * 8))
            _lib.call('vqvae_resblock_bwd', C.byref(d), C.byref(prm), h.ptr, None, gates.ptr,
                      z.ptr, _p(g_res), s.g_skip.ptr, _p(gx), None, 0, gh.ptr, C.byref(none), 0,
                      ws.ptr, ws.nbytes, _S())
        else:
            am = None
            if w is not None:      # in: g_res_i, g_skip; out: gh_i and gx = g_res_{i-1}
                am = C.byref(_lib.ResblockAmax(
                    None, None, None if g_res is None else w.g_res(i), w.g_skip(),
                    w.gh(i), w.g_res(i - 1) if (gx is not None and i > 0) else None,
                    None, None, w.gh_scale(i) if s.hpre[i] else None,
                    (s.pb_part.ptr + i * (s.pb_part.nbytes // len(self.descs))) if s.pb_part is not None else None,
                    s.tb['v0'].ptr, s.tb['w0'].ptr, s.tb['w1'].ptr, s.Tl))
            _lib.call('vqvae_resblock_bwd_packed', C.byref(d), C.byref(prm), h.ptr, gates.ptr,
                      z.ptr, _p(g_res), s.g_skip.ptr, _p(gx), gh.ptr, ws.ptr, ws.nbytes,
                      self.packed.ptr + i * self.packed_stride, am, _S())
        return gx

    def _block_side_work(self, s, i):
        """Latent-rate condition, behind block i's launch: its dilated-conv weight gradient joins a group (issued when the
        group is full, unless kept for the deferred batch), gh_i is pulled back to the latent rate."""
        d, d0, nb, tb = self.descs[i], self.descs[0], len(self.descs), s.tb
        s.dil_pending.append(i)
        if (len(s.dil_pending) >= s.dil_group or i == 0) and not (s.defer and i < DEFER_DIL_BLOCKS):
            self._dil_wgrad(s, s.side, s.ws_side)               # waits (on the side stream) for the chain up to here
        elif s.overlap:
            backend.wait_event(s.side, backend.Event().record(_S()))
        dst, tabs = s.gP.ptr + i * d.Cd * s.Tl * 4, [tb[k].ptr for k in ('w0', 'w1', 'lo0', 'hi0', 'lo1', 'hi1')]
        if s.pb_part is not None or s.gh_all is not None:
            pass                       # done in the gate-derivative launch's epilogue and reduced below / one launch after the chain
        elif s.hpre[i]:
            _lib.call('vqvae_upsample_linear_bwd_f16x2', s.ghs[i].ptr, d.Cd * d.T, d.B, d.Cd, s.Tl, d.T,
                      *(tabs + [dst, nb * d.Cd * s.Tl, self.words.gh_scale(i), s.side]))
        else:
            _lib.call('vqvae_upsample_linear_bwd_bf16' if s.gh_store[i] & _lib.STORE_GH_BF16 else 'vqvae_upsample_linear_bwd',
                      s.ghs[i].ptr, d.Cd * d.T, d.B, d.Cd, s.Tl, d.T, *(tabs + [dst, nb * d.Cd * s.Tl, s.side]))
        # the fused pull-back's partial sums of the blocks the chain has passed, PB_REDUCE_GROUP at a time (round 5: ~15 us
        # between two chip-filling launches instead of one launch over all blocks in the tail -- 52 us alone, 160 us beside
        # the deferred weight gradients; round 6, with those 90 us shorter each: one launch behind the chain measures best)
        if s.pb_part is not None and (i % PB_REDUCE_GROUP == 0):
            hi_b = min(nb, i + PB_REDUCE_GROUP)
            _lib.call('vqvae_pullback_reduce_into', s.pb_part.ptr + i * (s.pb_part.nbytes // nb), tb['v0'].ptr, hi_b - i,
                      d0.B, d0.T, d0.Cd, s.Tl, s.gP.ptr + i * d0.Cd * s.Tl * 4, nb * d0.Cd * s.Tl, _S())

    def _dil_wgrad(self, s, stream, ws):
        """Dilated-conv weight gradients of the pending blocks (their gh exist), dil_group blocks at a time."""
        pending, s.dil_pending = s.dil_pending, []
        w = self.words
        for at in range(0, len(pending), s.dil_group):
            blocks = pending[at:at + s.dil_group]
            if s.overlap:
                backend.wait_event(s.side, backend.Event().record(_S()))    # their gh are complete
            # one launch per kind of (x, gh): the blocks whose input is the bf16 / pre-split residual stream, and the rest
            # (block 0; the blocks around one that is refused pre-split storage), each with the blocks that keep gh alike
            kinds = [(x16, g16) for x16 in (_lib.STORE_X_BF16, _lib.STORE_X_F16X2, 0)
                     for g16 in sorted(set(s.gh_store), reverse=True)]
            for x16, g16 in kinds:
                sel = [i for i in blocks if (self.descs[i].storage & (_lib.STORE_X_BF16 | _lib.STORE_X_F16X2)) == x16
                       and s.gh_store[i] == g16]
                if not sel:
                    continue
                dg = _lib.ResblockDesc.from_buffer_copy(self.descs[sel[0]])      # (a block the library offers these bits)
                dg.storage = g16 | x16
                dils = (C.c_int * len(sel))(*[self.dilations[i] for i in sel])
                xam = gam = None
                if w is not None:      # (a pre-split operand is read under the bound it was split under: its scale words)
                    xam = (C.c_void_p * len(sel))(*[w.x_scale(i) if x16 == _lib.STORE_X_F16X2 else w.x(i) for i in sel])
                    gam = (C.c_void_p * len(sel))(*[w.gh_scale(i) if s.hpre[i] else w.gh(i) for i in sel])
                _lib.call('vqvae_resstack_dil_wgrad', C.byref(dg), len(sel), dils,
                          _lib.ptr_array([self.saved[i][0] for i in sel]), _lib.ptr_array([s.ghs[i] for i in sel]),
                          _lib.ptr_array([s.g[i]['Wd'] for i in sel]), _lib.ptr_array([s.g[i]['bd'] for i in sel]),
                          0, ws.ptr, ws.nbytes, xam, gam, stream)

    def _res_wgrad(self, s, stream, ws):
        """gWr_l, gbr_l of every block that has a residual output (g_res_l exists once the chain has passed block l + 1): one
        batched launch per group behind the chain; ``ws`` None: the main stream's workspace."""
        d0, nb, w = self.descs[0], len(self.descs), self.words
        for l in range(nb):
            if s.g_ress[l] is not None:
                s.grad_out(l, 'Wr')
                s.grad_out(l, 'br')
        for a, b in _groups(nb):
            wsm = ws if ws is not None else backend.workspace(_lib.load().vqvae_resstack_workspace_bytes(C.byref(d0), b - a))
            zs = _lib.ptr_array([sv[2] for sv in self.saved[a:b]])
            ram = None
            if w is not None:      # g_res_l was published by block l + 1's backward-data launch
                ram = (C.c_void_p * (b - a))(*[None if s.g_ress[l] is None else w.g_res(l) for l in range(a, b)])
            _lib.call('vqvae_resstack_res_wgrad', C.byref(d0), b - a, _lib.ptr_array(s.g_ress[a:b]), zs,
                      _lib.ptr_array([g['Wr'] for g in s.g[a:b]]), _lib.ptr_array([g['br'] for g in s.g[a:b]]),
                      0, wsm.ptr, wsm.nbytes, ram, stream)

    def _cproj_backward(self, s):
        """Every block's gh has been pulled back to the latent rate (adjoint of the epilogue lerp) into gP; the
        (nb*Cd, Cc) 1x1 conv's own backward then gives gWc_l, gbc_l and (returned) the condition gradient."""
        d, nb, lat, tb = self.descs[0], len(self.descs), self.lat, s.tb
        Cc = lat.shape[1]
        if s.gh_all is not None:       # neither the fused nor the per-block pull-back ran: ONE launch over all blocks' gh
            bf = 1 if s.gh_store[0] & _lib.STORE_GH_BF16 else 0
            _lib.call('vqvae_upsample_linear_bwd_blocks', s.gh_all.ptr, bf, d.B * d.Cd * d.T * (2 if bf else 1), d.Cd * d.T,
                      nb, d.B, d.Cd, s.Tl, d.T, tb['w0'].ptr, tb['w1'].ptr, tb['lo0'].ptr, tb['hi0'].ptr, tb['lo1'].ptr,
                      tb['hi1'].ptr, s.gP.ptr, d.Cd * s.Tl, nb * d.Cd * s.Tl, _S())
        wsc = backend.workspace(_lib.load().vqvae_conv1d_workspace_bytes(C.byref(self.pdesc)))
        # the condition gradient first: it is what the rest of the sweep (condition embed, quantiser, encoder) waits
        # for; the projection's own weight gradient is a leaf -- on the side stream behind the other deferred ones
        gcond = None
        if 1 in s.indexes:
            glat = DeviceArray(lat.shape, np.float32)
            _lib.call('vqvae_conv1d_bwd_data_amax', C.byref(self.pdesc), self.Wc_all.ptr, s.gP.ptr,
                      glat.ptr, 0, wsc.ptr, wsc.nbytes,
                      C.byref(_lib.Conv1dAmax(None, None, None, _p(self._cslab_b))), _S())
            gcond = F.LatentGrad(s.cond.shape, glat)
        sw, wsw = _S(), wsc
        if s.defer:
            sw, wsw = backend.side_stream(), s.ws_defer
            backend.wait_event(sw, backend.Event().record(_S()))        # gP is complete
        gWc_all = DeviceArray(self.Wc_all.shape, np.float32)
        gbc_all = DeviceArray((nb * d.Cd,), np.float32)
        _lib.call('vqvae_conv1d_bwd_weight', C.byref(self.pdesc), lat.ptr, s.gP.ptr, gWc_all.ptr,
                  gbc_all.ptr, 0, wsw.ptr, wsw.nbytes, sw)
        gWc = [s.grad_out(l, 'Wc') for l in range(nb)]
        gbc = [s.grad_out(l, 'bc') for l in range(nb)]
        for lo, hi in _groups(nb):
            _lib.call('vqvae_split', gWc_all.ptr + lo * d.Cd * Cc * 4, _lib.ptr_array(gWc[lo:hi]),
                      hi - lo, d.Cd * Cc, 0, sw)
            _lib.call('vqvae_split', gbc_all.ptr + lo * d.Cd * 4, _lib.ptr_array(gbc[lo:hi]),
                      hi - lo, d.Cd, 0, sw)
        if s.defer:
            backend.defer_to_side([gWc_all, gbc_all, s.gP, lat, gWc, gbc, wsw], writes=[gWc_all, gbc_all] + gWc + gbc)
        return gcond

    def _gcond_backward(self, s):
        """Materialised condition: its gradient sum_l Wc_l^T gh_l, one GEMM per group."""
        d = self.descs[0]
        gcond = DeviceArray(s.cond.shape, np.float32)
        for lo, hi in _groups(len(self.descs)):
            ws = backend.workspace(_lib.load().vqvae_resstack_workspace_bytes(C.byref(d), hi - lo))
            _lib.call('vqvae_resstack_gcond_bwd', C.byref(d), hi - lo, _lib.ptr_array([b.Wc for b in s.blocks[lo:hi]]),
                      _lib.ptr_array(s.ghs[lo:hi]), gcond.ptr, 0 if lo == 0 else 1, ws.ptr, ws.nbytes, _S())
        return gcond


class ResidualBlock(Chain):
    """modules.py:7-56."""

    def __init__(self, filter_size, dilation, residual_channels, dilated_channels, skip_channels,
                 condition_dim, dropout_zero_rate):
        super(ResidualBlock, self).__init__()
        with self.init_scope():
            self.conv = L.DilatedConvolution2D(
                residual_channels, dilated_channels, ksize=(filter_size, 1),
                pad=(dilation * (filter_size - 1), 0), dilate=(dilation, 1))
            self.condition_proj = L.Convolution2D(condition_dim, dilated_channels, 1)
            self.res = L.Convolution2D(dilated_channels // 2, residual_channels, 1)
            self.skip = L.Convolution2D(dilated_channels // 2, skip_channels, 1)
        self.filter_size = filter_size
        self.dilation = dilation
        self.residual_channels = residual_channels
        self.condition_dim = condition_dim
        self.dropout_zero_rate = dropout_zero_rate
        if dropout_zero_rate:
            raise NotImplementedError(
                'dropout_zero_rate > 0 (modules.py:34-35) is outside the hot-path scope: '
                'every BASELINE config trains with 0 (params.py:42)')

    def param_list(self):
        return list(BlockParams(Wd=self.conv.W, bd=self.conv.b, Wc=self.condition_proj.W, bc=self.condition_proj.b,
                                Wr=self.res.W, br=self.res.b, Ws=self.skip.W, bs=self.skip.b))

    def __call__(self, x, condition):
        residual, skip_connection = ResidualBlockFunction(self.dilation).apply(
            [x, condition] + self.param_list())
        return residual, skip_connection


class ResidualNet(ChainList):
    """modules.py:77-96."""

    def __init__(self, n_loop, n_layer, filter_size, residual_channels, dilated_channels,
                 skip_channels, condition_dim, dropout_zero_rate):
        super(ResidualNet, self).__init__()
        dilations = [2 ** i for i in range(n_layer)] * n_loop
        for dilation in dilations:
            self.add_link(ResidualBlock(
                filter_size, dilation, residual_channels, dilated_channels, skip_channels,
                condition_dim, dropout_zero_rate))
        self._prepacked = None        # prepack_async's Prepack, until the next forward takes it
        self._cproj_shape = None      # (B, Cc, Tl) of the last forward's latent-rate projection: the next prepack_async packs for it

    def __call__(self, x, condition):
        return self._forward(x, condition, False)

    def relu_call(self, x, condition):
        """F.relu(self(x, condition)) with the ReLU in the skip sum's epilogue (WaveNet.__call__, modules.py:158)."""
        return self._forward(x, condition, True)

    def _forward(self, x, condition, relu):
        blocks = list(self.children())
        args = [x, condition]
        for b in blocks:
            args += b.param_list()
        pre, self._prepacked = self._prepacked, None
        if pre is not None and pre.owner_steps != _owner_steps(args[2:]):       # an optimizer step between the pack and this forward
            pre = None
        fn = ResidualStackFunction([b.dilation for b in blocks], relu_out=relu, prepacked=pre)
        out = fn.apply(args)[0]
        self._cproj_shape = fn.cproj_shape
        return out

    def prepack_async(self, B, T, after=None):
        """The chain's weight slabs for an upcoming forward over (B, ., T), packed on the SIDE stream now: the 25 packing
        launches (~0.3 ms on a handful of workgroups) run beside the encoder / quantiser / condition-embed chain instead of in
        front of the first gate GEMM.  The forward takes the result if nothing changed (parameters, shapes, matmul mode), else
        packs as before.  ``after``: the main-stream event the side stream has to be behind (the optimizer's last write of the
        parameters); None: the main stream as it is now.  VAE.__call__ records that event when the step starts but calls this
        AFTER it has enqueued the encoder: launches reach the GPU in the order they are issued -- from Python and from a
        replayed hipGraph alike (ROCm enqueues a graph's nodes one by one, in capture order) -- so 25 side-stream launches
        issued in front of the first encoder conv delayed the whole critical path by the time it takes to ISSUE them.
        Each of the three parts below allocates (from the pool, as it is at this call) and then launches."""
        if not (PACK_ONCE and PREPACK_ASYNC):
            return
        pvars = [p for b in self.children() for p in b.param_list()]
        params = [p.data for p in pvars]
        if any(not isinstance(p, DeviceArray) for p in params):
            return
        blocks = _per_block(params)
        nb, b0 = len(blocks), blocks[0]
        Cd, Cc = b0.Wc.shape[:2]
        d0 = _lib.ResblockDesc(B, T, b0.Wd.shape[1], b0.Wd.shape[0], b0.Ws.shape[0], Cc, b0.Wd.shape[2],
                               next(self.children()).dilation)
        side = backend.side_stream()
        backend.wait_event(side, after if after is not None else backend.Event().record(_S()))       # the optimizer's last write of the parameters
        packed, per = _pack_stack(blocks, d0, side)
        # ... and, when the last forward projected the condition at the latent rate, that projection's weight / bias
        # (three concats and an add over the blocks' parameters) and its packed slabs for both directions
        cp, shape = None, self._cproj_shape
        if shape is not None:
            cp = _build_cproj(blocks, side)
            if shape[0] == B and shape[1] == Cc:
                lib = _lib.load()
                descs = (_lib.Conv1dDesc * 2)()
                for i in range(2):
                    C.pointer(descs[i])[0] = _lib.Conv1dDesc(B, shape[1], shape[2], nb * Cd, shape[2], 1, 1, 0, 1, 0)
                cp = cp._replace(
                    slab_f=DeviceArray((int(lib.vqvae_conv1d_packed_bytes(C.byref(descs[0]), 0)) // 4,), np.float32),
                    slab_b=DeviceArray((int(lib.vqvae_conv1d_packed_bytes(C.byref(descs[1]), 1)) // 4,), np.float32),
                    shape=tuple(shape))
                _lib.call('vqvae_conv1d_pack', 2, descs, (C.c_void_p * 2)(cp.Wc_all.ptr, cp.Wc_all.ptr), (C.c_int * 2)(0, 1),
                          (C.c_void_p * 2)(cp.slab_f.ptr, cp.slab_b.ptr), side)
        # ... and the skip sum's weight slabs and bias sums (one contraction over all blocks: vqvae_resstack_skip_prepare)
        skipws = None
        if nb <= _lib.MAX_STACK_GROUP:
            nbytes = _lib.load().vqvae_resstack_workspace_bytes(C.byref(d0), nb)
            skipws = DeviceArray((int(nbytes) // 4 + 1,), np.float32)
            _lib.call('vqvae_resstack_skip_prepare', C.byref(d0), nb, _lib.ptr_array([b.Ws for b in blocks]),
                      _lib.ptr_array([b.bs for b in blocks]), skipws.ptr, skipws.nbytes, side)
        self._prepacked = Prepack(_value_key(params), _pack_key(params, d0), packed, per, backend.Event().record(side),
                                  cp, skipws, _owner_steps(pvars))


class WaveNet(Chain):
    """modules.py:113-160."""

    def __init__(self, n_loop, n_layer, filter_size, input_dim, residual_channels,
                 dilated_channels, skip_channels,
                 # arguments for output
                 quantize, use_logistic, n_mixture, log_scale_min,
                 # arguments for conditioning
                 condition_dim,
                 # arguments for dropout
                 dropout_zero_rate):
        super(WaveNet, self).__init__()
        with self.init_scope():
            self.embed = L.Convolution2D(input_dim, residual_channels, (2, 1), pad=(1, 0))
            self.resnet = ResidualNet(
                n_loop, n_layer, filter_size, residual_channels, dilated_channels, skip_channels,
                condition_dim, dropout_zero_rate)
            self.proj1 = L.Convolution2D(skip_channels, skip_channels, 1)
            output_dim = n_mixture if use_logistic else quantize
            self.proj2 = L.Convolution2D(skip_channels, output_dim, 1)
        self.input_dim = input_dim
        self.quantize = quantize
        self.use_logistic = bool(use_logistic)
        self.skip_channels = skip_channels
        self.log_scale_min = log_scale_min

    def calculate_logistic_loss(self, y, t):
        """modules.py:169-230 as one fused kernel pair."""
        return F.mixture_of_logistics_nll(y, t, self.quantize, self.log_scale_min)

    def embed_input(self, x):
        """The causal embed conv (modules.py:151-152) on whichever form of the input arrived."""
        if np.dtype(x.dtype) == np.int32:
            # device-side input pipeline: x holds mu-law bin indices (B, T) instead of the
            # one-hot (B, q, T, 1) tensor -- the embed conv is a gather of its weight columns
            return F.embed_conv_indices(x, self.embed.W, self.embed.b)
        if (self.input_dim >= 8 and self.embed.W.data is not None and x.shape[1] == self.embed.W.shape[1]
                and self.embed.pad[0] == self.embed.ksize[0] - 1 and self.embed.stride[0] == 1
                and _lib.load().vqvae_get_matmul_dtype() != 1):      # bf16 mode rounds W: dense kernels
            # the reference's one-hot float input (utils.py:85-87): same causal conv, but the device
            # checks for one-hot-ness and then gathers / bincounts instead of multiplying by zeros
            return F.embed_conv_onehot(x, self.embed.W, self.embed.b)
        # causal conv: pad 1 then crop to the input length (modules.py:151-152), fused as out_len
        return self.embed(x, out_len=x.shape[2])

    def __call__(self, x, condition, generating=False):
        # `generating` is accepted and ignored, as in modules.py:148-160
        x = self.embed_input(x)
        # residual & skip connections (modules.py:155)
        z = self.resnet.relu_call(x, condition)
        # output (modules.py:158-159); the ReLU after proj1 is fused into its epilogue
        z = self.proj1(z, relu=True)
        y = self.proj2(z)
        return y

    # ---- incremental generation (modules.py:232-255; generate.py:100-145) ----
    def initialize(self, n):
        """modules.py:232-244: fresh all-zero queues for ``n`` sequences (the reference supports
        n = 1, generate.py:42; here 1..4 run in lockstep)."""
        from .generation import GenerationState
        self._gen = GenerationState(self, n)

    def _gen_state(self):
        st = getattr(self, '_gen', None)
        if st is None:
            raise RuntimeError('call WaveNet.initialize(n) before generate (generate.py:100)')
        from . import core
        if st._epochs != (core.param_epoch('layout'), core.param_epoch('load')):
            raise RuntimeError('parameters were moved (optimizer.setup) or re-loaded (load_npz) since '
                               'WaveNet.initialize(n): call initialize(n) again')
        return st

    def _gen_args(self, condition):
        """(the condition's array or LatentCondition, the sample mode of this decoder's output) for the generate_* calls."""
        from .core import Variable
        return (condition.data if isinstance(condition, Variable) else condition,
                _lib.GEN_MOL if self.use_logistic else _lib.GEN_SOFTMAX)

    def generate(self, x, condition):
        """modules.py:246-255: one step.  x (n, input_dim, 1, 1), condition (n, condition_dim, 1, 1)
        -> logits Variable (n, out_dim, 1, 1); the queues advance by one sample."""
        from .core import Variable
        from .generation import refuse_latent
        xd = x.data if isinstance(x, Variable) else x
        cd, _ = self._gen_args(condition)
        refuse_latent(cd, 'generate')
        backend.require_device(xd, cd)
        return Variable(self._gen_state().step_logits(xd, cd))

    def generate_sequence(self, condition, uniforms, n_steps=None, forced=None, return_logits=False,
                          graph_steps=8, persistent=True, temperature=None, top_k=None, top_p=None):
        """The loop of generate.py:101-145 as one device-resident run from fresh queues:
        condition (n, condition_dim, T[, 1]) on the device; ``uniforms`` the host doubles NumPy's
        RNG would hand generate.py:117 / 136 -- (T, n) for the softmax output, (T, n, nr_mix) for
        the mixture of logistics.  Returns the device array ``output`` (n, T): int32 mu-law bins or
        float32 samples, last column 0 as in generate.py:103-105 (plus the per-step logits
        (steps, n, out_dim) when ``return_logits``).  ``forced`` (T, n) feeds these values back
        instead of the samples (teacher forcing).  ``persistent`` runs the loop as one persistent
        kernel (csrc/generate.hip, channel counts <= 512, condition <= 640); otherwise as a replayed hipGraph of
        per-step kernels (``graph_steps`` steps per graph, 0 = eager launches).

        ``temperature`` / ``top_k`` / ``top_p``: sampling controls (include/vqvae_sampling.h), each None, a scalar or one
        value per sequence: temperature >= 0 (0 = greedy: the most likely class, lowest index on ties), top_k >= 0 (0 =
        off), top_p in (0, 1] (1 = off); the mixture of logistics takes a temperature > 0 only.  All None is the call
        as it was.  With any control the persistent kernel is not used, whatever ``persistent`` says: it has no filtered
        form, and the run is the replayed hipGraph of per-step kernels (for one sequence of the default decoder 667 us
        against 95 us per sample).

        The condition is the dense tensor: a generation.LatentCondition is a TypeError here (the persistent launch runs
        thousands of steps and cannot take a per-step column); generate_lockstep takes one, ``.dense()`` expands it.

        ``uniforms`` may be a DeviceUniforms(seed, stream_ids) instead of the array: the numbers are then Philox4x32-10
        draws made on the device (include/vqvae_gen_rng.h), sequence i the stream stream_ids[i] (default i), and the
        host draws and uploads nothing.  The kernels of this call (n <= 4) keep reading an array, so it is filled on the
        device first, (steps, n[, nr_mix]) doubles; every other argument means what it means with an array, and the
        result is that of the call with ``uniforms.host(steps, n_uniform)``, bit for bit."""
        from .generation import refuse_latent, sampling_controls
        cd, mode = self._gen_args(condition)
        refuse_latent(cd, 'generate_sequence')
        sampling = sampling_controls(cd.shape[0], temperature, top_k, top_p, self.use_logistic, 'generate_sequence')
        backend.require_device(cd)
        self.initialize(cd.shape[0])
        return self._gen_state().run(cd, uniforms, mode, n_steps, forced, return_logits, graph_steps,
                                     persistent, sampling=sampling)

    def generate_batch(self, condition, uniforms, n_steps=None, group=4, max_streams=8, temperature=None, top_k=None,
                       top_p=None):
        """Serving form: N sequences generated as concurrent groups of <= ``group`` lockstep sequences,
        one persistent launch per group on its own stream.  condition (N, condition_dim, T[, 1]) on the
        device, uniforms (T, N[, nr_mix]) host doubles; returns the host array (N, T).  Every sequence
        gets exactly the samples generate_sequence would give it alone with its column of uniforms.
        It exists only as persistent launches, which have no filtered sampler: any of ``temperature`` / ``top_k`` /
        ``top_p`` is a ValueError; generate_lockstep takes them.  So is a generation.LatentCondition a TypeError: the
        persistent launches read the dense tensor (``.dense()``); generate_lockstep takes the latent form.  And so is a
        DeviceUniforms: the persistent launches read an array (``.host(...)``); generate_lockstep draws on the device."""
        from .generation import refuse_device_uniforms, refuse_latent, run_many
        cd, mode = self._gen_args(condition)
        refuse_latent(cd, 'generate_batch')
        refuse_device_uniforms(uniforms, 'generate_batch')
        if temperature is not None or top_k is not None or top_p is not None:
            raise ValueError('generate_batch runs persistent launches only, which have no sampling controls: '
                             'use generate_lockstep (any number of sequences) or generate_sequence (n <= 4)')
        backend.require_device(cd)
        return run_many(self, cd, uniforms, mode, n_steps, group, max_streams)

    def generate_lockstep(self, condition, uniforms, n_steps=None, lengths=None, forced=None, return_logits=False,
                          graph_steps=8, group=128, temperature=None, top_k=None, top_p=None, refill=False):
        """Many sequences (a validation set, a corpus): N sequences of any count as groups of <= ``group`` (<= 128)
        sequences that advance in lockstep on the matrix pipe, one weight stream per step for the whole group
        (csrc/generate_lockstep.hip).  condition (N, condition_dim, T[, 1]) on the device, uniforms (T, N[, nr_mix])
        host doubles; ``lengths`` (N,): sequence i runs lengths[i] - 1 steps and the rest of its row is 0.  Returns the
        host array (N, T) in the caller's order (plus the logits (steps, N, out_dim) when ``return_logits``).  One
        sequence alone is faster on generate_sequence (persistent kernel); see INTEGRATION.md "Generation".
        ``temperature`` / ``top_k`` / ``top_p``: as in generate_sequence, each None, a scalar or one value per sequence
        (N), so one batch can mix settings; all None is the call as it was.
        ``refill``: with sequences of different lengths a group runs to its longest member and the columns of the
        shorter ones do dead work.  True keeps the columns busy instead: ``group`` (5..128) is the number of slots, and a
        slot whose sequence has finished takes the next waiting one, longest first, on the device
        (csrc/generate_slots.hip; generation.run_lockstep_refill documents the memory it needs).  Every other argument
        means what it means without, the return value is the same, bit for bit.  False (the default) is the call as
        it was.
        ``condition`` may be a generation.LatentCondition instead of the dense tensor: the local latents and the speaker
        vectors the tensor is an up-sampling of, 1/80 of its bytes for the default model (32 instead of 2 560 per
        sample).  Every step, with and without ``refill``, then starts with one small launch that computes the
        condition column of each live sequence (csrc/generate_cond.hip); T is the longest sequence, ``lengths`` defaults
        to the object's own, and the return value is that of the call with ``condition.dense()``, bit for bit.  The way to
        convert a corpus whose dense condition does not fit the device.
        ``uniforms`` may be a DeviceUniforms(seed, stream_ids) instead of the (T, N[, nr_mix]) array: every finishing
        launch then computes its own uniforms (Philox4x32-10 counted by the sequence's step and keyed by the seed;
        include/vqvae_gen_rng.h), so no array of N x T doubles exists on the host or on the device, only the (N,)
        stream ids (default arange(N)).  Sequence i's values then depend on (seed, stream_ids[i]), its own condition and
        the model alone: not on N, on ``group``, on ``refill``, on its position or on the other lengths.  The result is
        that of the call with ``uniforms.host(steps, n_uniform)``, bit for bit.  ``out`` (N, T) and ``forced`` stay dense."""
        from .generation import LatentCondition, run_lockstep, run_lockstep_refill, sampling_controls
        cd, mode = self._gen_args(condition)
        sampling = sampling_controls(cd.shape[0], temperature, top_k, top_p, self.use_logistic, 'generate_lockstep')
        if not isinstance(cd, LatentCondition):
            backend.require_device(cd)
        return (run_lockstep_refill if refill else run_lockstep)(
            self, cd, uniforms, mode, n_steps, lengths, forced, return_logits, graph_steps, group, sampling=sampling)
