"""C ABI contract tests of the packed latent-rate-condition chain: the twelve entry points wavenet.ResidualStackFunction
drives, called here directly (never through that class), one tests/zoned.py run_contract per entry point call, in the
chain's order:

  vqvae_resstack_pack -> vqvae_resblock_fwd_packed (blocks 0 .. n-1) -> vqvae_resstack_skip_fwd, and
  vqvae_resstack_skip_prepare + vqvae_resstack_skip_fwd_prepared -> vqvae_resblock_bwd_packed (blocks n-1 .. 0) ->
  vqvae_resstack_dil_wgrad, _res_wgrad, _skip_wgrad, _gcond_bwd -> vqvae_pullback_reduce / _reduce_into.

What one call hands to the next is the array read back from the ZONED run of the producer (its buffers started as
NaN poison): the slab image, the prepared skip workspace, res / gates / z / gh / gx, the maxima and scale words, pb_part.
A word a producer never writes therefore reaches its consumer as a NaN pattern.  Every workspace is exactly as large as
its query says.  The three contracts are those of tests/test_gpu_abi_contract.py (zones, inputs_only, maxima), and every
output is compared with the float64 chain (oracle.resblock_fwd / resblock_bwd block by block over
oracle.upsample_fwd of the latent condition) at the bars of the neighbouring tests: 1e-4.

The packed slabs are tagged on the host by the address vqvae_resstack_pack wrote them to (conv_api.hip packed_check), so
a consumer's fn re-packs into ITS slab buffer and then overwrites it with the image of the zoned pack run before it calls
the entry point: the bytes the entry point reads are the image's, unwritten words included.

Storage bits are planned here by the rule of wavenet._plan_storage, restated (the first block RES only, the last block X
only, a stored stream only between two blocks that are both offered it and behind which no block is refused, GH where
offered and a pull-back can read it stored, GATES_SIG where offered), and asserted against the predicates of
csrc/conv_api.hip restated in _expect_bits.

Published words, decided from the epilogues (gemm_common.h: `am` = max |value stored|, amax_commit):
  res, gx, gh stored fp32      the maximum over the 16 words EQUALS max |output| (bit pattern);
  res, gh stored pre-split     the word is the maximum of the fp32 values before the split, times 1 + 2^-22 (the stored
                               pieces keep 22 significant bits, rounded to nearest): >= the decoded maximum and within
                               2^-20 of it;
  skip_amax_out                EQUALS max |skip| with accumulate = 0; with accumulate = 1 checked as a bound (as
                               test_conv1d_contract does for gx);
  res_scale, gh_scale          documented as bounds: word 0 >= the published maximum, and bound / max inside
                               2^backend.CONTRACT_LOG2_LIMIT (the ratio is printed per block: CHAIN_ABI ... ratio).

Shown able to fail (one-line mutations of chain code built into a scratch copy of csrc/ and run once; never committed):
  inputs_only: vqvae_resstack_pack skipping the backward-data slab (pk_bd) of the LAST block: test_packed_chain_contract
               fails in float32x2 (c256_T256) and float32 (c512_T256) at that block's vqvae_resblock_bwd_packed with "output gx:
               non-finite at flat index 0 (131072 in all): an element was not written, or was computed from memory outside
               the inputs" -- the slab image of the zoned pack run carries the poison to its reader;
  zones:       pullback_reduce_kernel storing ONE element past its 64 rows when gP_bstride is wider than the rows written:
               test_packed_chain_contract[float32x2-c256_T256] fails at vqvae_pullback_reduce_into with "output gP: element
               (0, 2048) outside the documented extent was written (2 such elements)".  (The overrun was confined to the
               padded stride on purpose: past an exactly-sized buffer it would also have left the plain run's pool block);
  maxima:      amax_commit skipping the atomicMax of a launch's LAST workgroup: test_packed_chain_contract[float32x2-c256_T256]
               fails with "published max |gx| of block 1 is 2.2273707389831543, the tensor holds 2.366529941558838", and
               test_published_maximum_chain fails for the spike in the last tile of the last batch item of both classes
               (c256-last_all, c512-last_all: "published max |res| of block 0 is 4.790260314941406, the stored values decode
               to 63.95338439941406") while c512-first and c512-last_rows pass;
  value:       the `tnum >= 0` guard of the tap column in the float32x2 / float32x3 GEMM (conv_gemm_x3.hip col_offset) dropped:
               the kernels address x through a buffer descriptor that starts at the batch item's first row, so a tap in
               front of the row cannot leave the tensor: it reads the previous channel's tail.  No zone and no NaN is
               involved; test_packed_chain_contract fails by value in both modes at all three rows tried (c256_T256,
               c256_T384_dil_ge_T, c512_T256): "sigmoid of block 0: max err 4.207e-01 at 39424" / "gates of block 0: max err
               1.632e+00 at 70912"; 'float32' (another kernel) passes.

Found by these tests: the maximum published for a tensor stored pre-split (`res`, `gh`) was the maximum of the fp32 values
BEFORE the split, and the stored pieces (22 significant bits, rounded to nearest) decode to as much as 2^-23 more: in
c256_T256 block 1 published 5.5913825 for a tensor that decodes to 5.5913830.  No reader was hurt (the word enters bounds that
carry a 2^-10 margin), but the word was below the tensor it describes; the four epilogues that store pre-split now publish
max * (1 + 2^-22) (gemm_common.h PRESPLIT_AMAX_UP).
"""
import ctypes as C

import numpy as np
import pytest

import vqvae_oracle as O
from helpers import assert_close, assert_close_scaled
from test_gpu_abi_contract import ZERO_WORDS, _amax_of, _bf16_round, _bits32, _call, _f32, _L, _presplit, _rs, bf16_mode  # noqa: F401
from test_gpu_kernels import _rb_params
from zoned import In, Out, Ws, run_contract

pytestmark = pytest.mark.gpu

GH16, X16, RES16, GX16, GRES16 = 1, 2, 4, 8, 16            # VQVAE_STORE_*_BF16
GHX2, XX2, RESX2, GSIG = 32, 64, 128, 256                   # VQVAE_STORE_*_F16X2, VQVAE_STORE_GATES_SIG
ORDER = ('conv', 'condition_proj', 'res', 'skip')
K = 2


def _row(name, Cr, Cs, Cc, T, Tl, B, dils):
    return pytest.param((name, Cr, Cs, Cc, T, Tl, B, tuple(dils)), id=name)


# name, Cr = Cd, Cs, condition channels at the latent rate, T, Tl, B, dilations
ROW_BASE = _row('c256_T256', 256, 256, 192, 256, 4, 2, (1, 64, 2))          # one tile pair per row; block 1's taps reach 64 samples in front of the row
ROWS = [
    ROW_BASE,
    _row('c256_T384_dil_ge_T', 256, 256, 192, 384, 6, 3, (256, 512, 1)),    # dil < T < 2 dil, then dil >= T: block 1 refused, its neighbours fp32
    _row('c256_T192', 256, 256, 192, 192, 3, 2, (1, 2, 4)),                 # T % 64 == 0, T % 128 != 0
    _row('c256_T1000_up8', 256, 256, 192, 1000, 125, 2, (1, 2, 4)),         # nothing stored, no lin128_shape, T = 8 Tl
    _row('c512_T256', 512, 256, 128, 256, 4, 2, (1, 2, 256)),               # lin_stream_wide, gate-derivative strip; block 2: dil >= T
    _row('c512_T384', 512, 256, 128, 384, 6, 2, (1, 2, 256)),
    _row('c384_Cs320', 384, 320, 96, 256, 4, 2, (1, 2, 4)),                 # neither class: the generic packed chain
    _row('c256_Cs128', 256, 128, 192, 256, 4, 2, (1, 2, 4)),
    _row('c256_Cs512', 256, 512, 192, 256, 4, 2, (1, 2, 4)),
]
BF16_ROWS = [ROW_BASE, _row('c256_T192', 256, 256, 192, 192, 3, 2, (1, 2, 4))]


# --------------------------------------------------------------------------- #
# inputs and the float64 chain
# --------------------------------------------------------------------------- #
_INPUTS, _REF = {}, {}


def _inputs(row):
    if row not in _INPUTS:
        name, Cr, Cs, Cc, T, Tl, B, dils = row
        rs = _rs('chain_abi', row)
        _INPUTS[row] = dict(blocks=[_rb_params(rs, Cr, Cr, Cs, Cc, K) for _ in dils],
                            x=_f32(rs.standard_normal((B, Cr, T))), lat=_f32(rs.standard_normal((B, Cc, Tl))),
                            gy=_f32(rs.standard_normal((B, Cs, T))))
    return _INPUTS[row]


def _chain(row, inp, dtype=np.float64):
    """The chain block by block on the oracle over the materialised condition -> every tensor an entry point produces."""
    name, Cr, Cs, Cc, T, Tl, B, dils = row
    c = lambda a: a.astype(dtype)
    blocks = [{n: (c(W), c(b)) for n, (W, b) in blk.items()} for blk in inp['blocks']]
    x, lat, gy = c(inp['x']), c(inp['lat']), c(inp['gy'])
    cond = O.upsample_fwd(lat, T)
    nb, Ch = len(dils), Cr // 2
    ref = dict(x=[x], gates=[], z=[], skip=None, gh=[None] * nb, gx=[None] * nb, grads=[None] * nb, cond=cond)
    caches = []
    for blk, dil in zip(blocks, dils):
        res, sk, cch = O.resblock_fwd(blk, ref['x'][-1], cond, dil)
        caches.append(cch)
        ref['x'].append(res)
        ref['gates'].append(np.concatenate([cch[1], cch[2]], 1))
        ref['z'].append(cch[3])
        ref['skip'] = sk if ref['skip'] is None else ref['skip'] + sk
    g_res, gcond = None, 0
    for i in range(nb - 1, -1, -1):
        _, ta, sb, z = caches[i]
        gz = O.conv1d_bwd(z, blocks[i]['skip'][0], gy)[0]
        if g_res is not None:
            gz = gz + O.conv1d_bwd(z, blocks[i]['res'][0], g_res)[0]
        one = z.dtype.type(1)
        gh = np.concatenate([gz * sb * (one - ta * ta), gz * ta * sb * (one - sb)], 1)
        if gh.dtype == np.float32 and O.gh_saved_as_bf16(Ch, Cr, Cs, T, K):
            gh = O.bf16_round(gh)
        ref['gh'][i] = gh
        g_res, gc, ref['grads'][i] = O.resblock_bwd(blocks[i], caches[i], cond, dils[i], g_res, gy)
        if dtype == np.float32 and i >= 1 and Cs == Cr and T % 128 == 0 and O.gh_saved_as_bf16(Ch, Cr, Cs, T, K):
            g_res = O.bf16_round(g_res)                       # VQVAE_STORE_GX_BF16, as oracle.wavenet_bwd restates it
        ref['gx'][i] = g_res
        gcond = gcond + gc
    ref['gcond'] = gcond
    ref['gP'] = np.concatenate([O.upsample_bwd(np.ascontiguousarray(g), Tl) for g in ref['gh']], 1)      # (B, nb * Cd, Tl)
    return ref


def _reference(row):
    if row not in _REF:
        _REF[row] = _chain(row, _inputs(row))
    return _REF[row]


# --------------------------------------------------------------------------- #
# storage: the planner's rule and the library's predicates, both restated
# --------------------------------------------------------------------------- #
def _segmented(T, Tl):
    return Tl >= 3 and T >= 8 * Tl and T % 4 == 0 and T // 4 <= 2048      # the pull-back kernel that reads a stored gh


def _plan_bits(lib, descs, mode, T, Tl, fused):
    """([forward bits], [backward bits]) per block from the library's answers, by wavenet._plan_storage's rule."""
    nb = len(descs)
    f16, b16 = mode == 'float32x2', mode == 'bfloat16'
    sup = [lib.vqvae_resblock_f16x2_storage(C.byref(d)) if f16 else (lib.vqvae_resblock_bf16_storage(C.byref(d)) if b16 else 0)
           for d in descs]
    xbit, rbit = (XX2, RESX2) if f16 else (X16, RES16)
    both = [bool(s & xbit and s & rbit) for s in sup]
    stored = [both[l] and both[l + 1] for l in range(nb - 1)]
    for l in range(nb - 3, -1, -1):
        stored[l] = stored[l] and stored[l + 1]
    fwd = [0] * nb
    for l in range(nb - 1):
        if stored[l]:
            fwd[l] |= rbit                                    # the first block: RES only
            fwd[l + 1] |= xbit                                # the last block: X only
    bwd = list(fwd)
    gh_ok = fused or _segmented(T, Tl)
    for l in range(nb):
        if f16:
            fwd[l] |= sup[l] & GSIG
            bwd[l] |= sup[l] & GSIG
        if gh_ok:
            bwd[l] |= sup[l] & (GHX2 if f16 else GH16)
    if b16:
        gs = [bool(s & GX16 and s & GRES16) for s in sup]
        for l in range(nb - 1):
            if gs[l] and gs[l + 1]:
                bwd[l] |= GRES16
                bwd[l + 1] |= GX16
    return fwd, bwd


def _expect_bits(row, mode):
    """The bits a row is meant to run with, from the predicates of csrc/conv_api.hip (f16x2_storage_supported,
    bf16_storage_supported, vqvae_get_fused_pullback) -> (fwd, bwd, fused pull-back)."""
    name, Cr, Cs, Cc, T, Tl, B, dils = row
    nb = len(dils)
    fwd, bwd = [0] * nb, [0] * nb
    fused = mode == 'float32x2' and Cr == 256 and T % 128 == 0 and T >= 64 * Tl
    seg = _segmented(T, Tl)
    if mode == 'float32x2':
        shape = (Cr == 256 or (Cr == 512 and Cs in (256, 512))) and T % 128 == 0
        sup = [shape and d < T for d in dils]
        for l in range(nb):
            own = GSIG if sup[l] else 0
            gh = GHX2 if (sup[l] and (fused or seg)) else 0
            res = RESX2 if (l < nb - 1 and all(sup[l:])) else 0
            xin = XX2 if (l >= 1 and all(sup[l - 1:])) else 0
            fwd[l], bwd[l] = own | res | xin, own | res | xin | gh
    if mode == 'bfloat16' and Cr == 256 and Cs % 256 == 0 and T % 64 == 0:
        for l in range(nb):
            stream = T % 128 == 0
            fwd[l] = ((RES16 if l < nb - 1 else 0) | (X16 if l >= 1 else 0)) if stream else 0
            grad = stream and Cs == Cr
            bwd[l] = fwd[l] | (GH16 if seg else 0) | (((GRES16 if l < nb - 1 else 0) | (GX16 if l >= 1 else 0)) if grad else 0)
    return fwd, bwd, fused


# --------------------------------------------------------------------------- #
# stored forms: specs and decoders
# --------------------------------------------------------------------------- #
def _words(v):
    w = ZERO_WORDS.copy()
    w[5] = _bits32(v)
    return w


def _dec_presplit(words, scale):
    """The inverse of _presplit under scale word 0."""
    e = int(np.floor(np.log2(np.float64(np.asarray(scale, np.uint32)[:1].view(np.float32)[0]))))
    w = np.ascontiguousarray(words).view(np.uint32)
    hi = (w & 0xFFFF).astype(np.uint16).view(np.float16).astype(np.float64)
    lo = (w >> 16).astype(np.uint16).view(np.float16).astype(np.float64)
    return np.ldexp(hi + lo, e - 14)


def _dec_bf16(raw, shape):
    """bf16 kept in the first half of an fp32-sized buffer: the upper half-words of the values."""
    n = int(np.prod(shape))
    return (raw.reshape(-1)[:n].astype(np.uint32) << 16).view(np.float32).reshape(shape)


def _out_for(shape, fmt, valid=None):
    """The Out spec of a tensor kept as 'f32', 'x2' (one opaque dword per element) or 'bf16' (2-byte elements in the first
    half of the fp32-sized buffer: the other half keeps its bits)."""
    if fmt == 'f32':
        return Out(shape, valid=valid)
    if fmt == 'x2':
        return Out(shape, np.uint32, nan_ok=True)
    n = int(np.prod(shape))
    v = np.zeros(2 * n, bool)
    v[:n] = True if valid is None else np.asarray(valid, bool).reshape(-1)
    return Out((2 * n,), np.uint16, valid=v, nan_ok=True)


def _decode(raw, shape, fmt, scale=None):
    if fmt == 'f32':
        return raw
    return _dec_presplit(raw, scale) if fmt == 'x2' else _dec_bf16(raw, shape)


def _fmt(bits, x2bit, b16bit):
    return 'x2' if bits & x2bit else ('bf16' if bits & b16bit else 'f32')


# --------------------------------------------------------------------------- #
# the driver
# --------------------------------------------------------------------------- #
class Chain(object):
    """State of one direct run of the chain: host copies of everything the zoned runs produced, raw and decoded."""

    def __init__(self, gpu, row, mode, inp=None):
        self.gpu, self.row, self.mode = gpu, row, mode
        self.L = _L()
        self.lib = self.L.load()
        name, self.Cr, self.Cs, self.Cc, self.T, self.Tl, self.B, self.dils = row
        self.Cd, self.Ch, self.nb = self.Cr, self.Cr // 2, len(self.dils)
        self.inp = _inputs(row) if inp is None else inp
        self.f16 = mode == 'float32x2'
        self.descs = [self.L.ResblockDesc(self.B, self.T, self.Cr, self.Cd, self.Cs, self.Cc, K, d, 0) for d in self.dils]
        self.fused = bool(self.f16 and self.lib.vqvae_get_fused_pullback(C.byref(self.descs[0])) and self.T >= 64 * self.Tl)
        self.fwd_bits, self.bwd_bits = _plan_bits(self.lib, self.descs, mode, self.T, self.Tl, self.fused)
        self.zfmt = 'bf16' if (mode == 'bfloat16' and self.Ch == 128 and self.Cr == 256 and self.Cs % 256 == 0 and self.T % 64 == 0) else 'f32'
        from vqvae_amd.functions import resize_tables_host
        self.tab = resize_tables_host(self.Tl, self.T)
        # the latent-rate projection of every block (with bd riding in its bias: vqvae_resblock_cproj::P_has_bd), on the host
        lat = self.inp['lat'].astype(np.float64)
        P = [np.einsum('oc,bct->bot', blk['condition_proj'][0][:, :, 0].astype(np.float64), lat)
             + (blk['condition_proj'][1].astype(np.float64) + blk['conv'][1])[None, :, None] for blk in self.inp['blocks']]
        self.P_all = _f32(np.concatenate(P, 1))                                   # (B, nb * Cd, Tl)
        self.weights = {}
        for l, blk in enumerate(self.inp['blocks']):
            for n, short in zip(ORDER, ('d', 'c', 'r', 's')):
                self.weights['W%s%d' % (short, l)] = In(blk[n][0])
                self.weights['b%s%d' % (short, l)] = In(blk[n][1])
        self.x = [self.inp['x']] + [None] * self.nb                               # raw, as stored
        self.x_dec = [self.inp['x']] + [None] * self.nb
        self.x_words = [_words(np.abs(self.inp['x']).max())] + [None] * self.nb   # actual maxima
        self.x_scale = [None] * (self.nb + 1)
        self.gates, self.z, self.z_dec = [None] * self.nb, [None] * self.nb, [None] * self.nb
        self.gh, self.gh_dec, self.gh_words, self.gh_scale = ([None] * self.nb for _ in range(4))
        self.gx, self.gx_dec, self.gx_words = ([None] * self.nb for _ in range(3))
        self.pb_part = [None] * self.nb
        self.ratios = []

    # -- helpers ---------------------------------------------------------------------------------------------------
    def call(self, name, *args):
        _call(self.gpu, name, *args)

    def params(self, b, l):
        return self.L.ResblockParams(*[b['%s%s%d' % (k, s, l)].ptr for s in 'dcrs' for k in 'Wb'])

    def desc(self, l, bits):
        d = self.L.ResblockDesc.from_buffer_copy(self.descs[l])
        d.storage = bits
        return d

    def rb_ws(self, l):
        return self.lib.vqvae_resblock_workspace_bytes(C.byref(self.descs[l]))

    def pack_into(self, b):
        """vqvae_resstack_pack into b.slab (this registers the address), on the host order wavenet._pack_stack uses."""
        prms = (self.L.ResblockParams * self.nb)(*[self.params(b, l) for l in range(self.nb)])
        has_res = (C.c_int * self.nb)(*([1] * (self.nb - 1) + [0]))
        self.call('vqvae_resstack_pack', C.byref(self.descs[0]), self.nb, prms, has_res, b.slab.ptr, self.nb * self.per)

    def slab_image(self, b):
        self.pack_into(b)
        b.slab.set(self.slab)                                  # ... and what the entry point reads is the zoned pack run's image

    def tol(self, got, want, name, scaled=True, addend=None):
        """The bar of the neighbouring tests: 1e-4 (of scale, or of max(1, |want|)); addend: the caller's content of an
        accumulate = 1 call."""
        if addend is not None:
            want = want + addend
        (assert_close_scaled if scaled else assert_close)(got, want, 1e-4, '%s %s: %s' % (self.row[0], self.mode, name))

    # -- forward ---------------------------------------------------------------------------------------------------
    def pack(self):
        self.per = self.lib.vqvae_resstack_packed_bytes(C.byref(self.descs[0]))
        assert self.per > 0 and self.per % 4 == 0
        # the slab keeps words nobody writes (the condition-projection slabs of the unpacked form, the last block's res
        # slabs): its content is judged by the entry points that read it
        r = run_contract(self.gpu, self.pack_into, dict(self.weights, slab=Out((self.nb * self.per // 4,), np.uint32, exact=False)))
        self.slab = r['slab']

    def block_forward(self, i):
        d = self.desc(i, self.fwd_bits[i])
        last = i == self.nb - 1
        B, Cr, Cd, Ch, T, Tl = self.B, self.Cr, self.Cd, self.Ch, self.T, self.Tl
        xf, rf = _fmt(d.storage, XX2, X16), _fmt(d.storage, RESX2, RES16)
        gsig = bool(d.storage & GSIG)
        gvalid = None
        if gsig:                                               # the tanh half keeps its poison bits
            gvalid = np.zeros((B, Cd, T), bool)
            gvalid[:, Ch:] = True
        if self.zfmt == 'bf16':                                # bf16 (tanh | sigmoid << 16) as ONE dword in tanh's fp32 position (gemm_common.h, EPI_GATE)
            gvalid = np.zeros((B, Cd, T), bool)
            gvalid[:, :Ch] = True
        specs = dict(self.weights, x=In(self.x[i]), P=In(self.P_all), v0=In(self.tab['v0'], index_range=(0, Tl - 1)),
                     w0=In(self.tab['w0']), w1=In(self.tab['w1']), Pam=In(_words(np.abs(self.P_all).max())),
                     gates=Out((B, Cd, T), np.uint32, valid=gvalid) if self.zfmt == 'bf16' else Out((B, Cd, T), valid=gvalid),
                     z=_out_for((B, Ch, T), self.zfmt),
                     ws=Ws(self.rb_ws(i)), slab=In(self.slab))
        if not last:
            specs['res'] = _out_for((B, Cr, T), rf)
        if self.f16:
            specs['xw'] = In(self.x_scale[i] if xf == 'x2' else self.x_words[i])
            specs['xmax'] = In(self.x_words[i])
            if not last:
                specs['resw'], specs['rscale'] = Out(init=ZERO_WORDS), Out(init=ZERO_WORDS)

        def fn(b):
            self.slab_image(b)
            cp = self.L.ResblockCproj(b.P.ptr + i * Cd * Tl * 4, self.nb * Cd * Tl, Tl, b.v0.ptr, b.w0.ptr, b.w1.ptr, 1, b.Pam.ptr)
            am = None
            if self.f16:
                am = C.byref(self.L.ResblockAmax(b.xw.ptr, None if last else b.resw.ptr, None, None, None, None, b.xmax.ptr,
                                                 None if last else b.rscale.ptr, None))
            self.call('vqvae_resblock_fwd_packed', C.byref(d), C.byref(self.params(b, i)), b.x.ptr, C.byref(cp),
                      None if last else b.res.ptr, b.gates.ptr, b.z.ptr, b.ws.ptr, self.rb_ws(i),
                      b.slab.ptr + i * self.per, am)
        r = run_contract(self.gpu, fn, specs)
        self.gates[i], self.z[i] = r['gates'], r['z']
        self.z_dec[i] = _decode(r['z'], (B, Ch, T), self.zfmt)
        if not last:
            self.x[i + 1] = r['res']
            if self.f16:
                self.x_words[i + 1], self.x_scale[i + 1] = r['resw'], r['rscale']
            self.x_dec[i + 1] = _decode(r['res'], (B, Cr, T), rf, r.get('rscale'))
        return r

    def check_forward(self, i, ref, r):
        B, Cd, Ch, T = self.B, self.Cd, self.Ch, self.T
        last = i == self.nb - 1
        g = r['gates']
        if self.zfmt == 'bf16':
            w = np.ascontiguousarray(g[:, :Ch])
            g = np.concatenate([((w & 0xFFFF) << 16).view(np.float32), ((w >> 16) << 16).view(np.float32)], 1)
        if self.fwd_bits[i] & GSIG:
            assert (r['gates'][:, :Ch].view(np.uint32) == 0x7FD5A5A5).all(), 'GATES_SIG: the tanh half was written'
            self.tol(g[:, Ch:], ref['gates'][i][:, Ch:], 'sigmoid of block %d' % i, scaled=False)
        else:
            self.tol(g, ref['gates'][i], 'gates of block %d' % i, scaled=False)
        self.tol(self.z_dec[i], ref['z'][i], 'z of block %d' % i, scaled=False)
        if last:
            return
        self.tol(self.x_dec[i + 1], ref['x'][i + 1], 'res of block %d' % i, scaled=False)
        if self.f16:
            self.check_words('res', i, r['resw'], self.x_dec[i + 1], self.fwd_bits[i] & RESX2, r['rscale'])

    def check_words(self, what, i, words, values, presplit, scale=None, tight=True):
        """The published maximum of a tensor (see the module docstring) and, where it is pre-split, its scale words."""
        pub, true = _amax_of(words), float(np.abs(values).max())
        tag = '%s %s: published max |%s| of block %d' % (self.row[0], self.mode, what, i)
        if not presplit:
            assert int(np.asarray(words).max()) == _bits32(true), '%s is %r, the tensor holds %r' % (tag, pub, true)
            return
        assert true <= pub <= true * (1 + 2.0 ** -20), '%s is %r, the stored values decode to %r' % (tag, pub, true)
        from vqvae_amd import backend
        bound = float(np.asarray(scale, np.uint32)[:1].view(np.float32)[0])
        ratio = bound / max(pub, 1e-30)
        self.ratios.append((what, i, ratio))
        print('CHAIN_ABI %s %s block %d: %s bound / max ratio %.3f' % (self.row[0], self.mode, i, what, ratio))
        assert bound >= pub, '%s: scale word 0 = %r is below the maximum %r' % (tag, bound, pub)
        assert not tight or ratio <= 2.0 ** backend.CONTRACT_LOG2_LIMIT, '%s: bound %r is 2^%.1f above the maximum' % (tag, bound, np.log2(ratio))

    def skip_specs(self):
        specs = dict(self.weights)
        for l in range(self.nb):
            specs['z%d' % l] = In(self.z[l])
        return specs

    def skip_forward(self, accumulate, relu, init=None, prepared=None):
        """vqvae_resstack_skip_fwd, or (prepared = the zoned vqvae_resstack_skip_prepare run's workspace) _fwd_prepared."""
        d0, nb = self.descs[0], self.nb
        ws_bytes = self.lib.vqvae_resstack_workspace_bytes(C.byref(d0), nb)
        specs = self.skip_specs()
        specs['skip'] = Out(init=init) if accumulate else Out((self.B, self.Cs, self.T))
        specs['ws'] = Ws(ws_bytes) if prepared is None else In(prepared)
        if self.f16:
            specs['words'] = Out(init=ZERO_WORDS)

        def fn(b):
            zs = (C.c_void_p * nb)(*[b['z%d' % l].ptr for l in range(nb)])
            am = b.words.ptr if self.f16 else None
            if prepared is not None:
                self.call('vqvae_resstack_skip_fwd_prepared', C.byref(d0), nb, zs, b.skip.ptr, accumulate, relu, b.ws.ptr, ws_bytes, am)
                return
            Wp = (C.c_void_p * nb)(*[b['Ws%d' % l].ptr for l in range(nb)])
            bp = (C.c_void_p * nb)(*[b['bs%d' % l].ptr for l in range(nb)])
            self.call('vqvae_resstack_skip_fwd', C.byref(d0), nb, Wp, bp, zs, b.skip.ptr, accumulate, relu, b.ws.ptr, ws_bytes, am)
        r = run_contract(self.gpu, fn, specs)
        if self.f16:
            pub, true = _amax_of(r['words']), float(np.abs(r['skip']).max())
            assert pub >= true, 'skip_amax_out %r below max |skip| %r (accumulate %d relu %d)' % (pub, true, accumulate, relu)
            if not accumulate:
                assert int(r['words'].max()) == _bits32(true), 'skip_amax_out %r is not max |skip| %r (relu %d)' % (pub, true, relu)
        return r

    def skip_prepare(self):
        d0, nb = self.descs[0], self.nb
        ws_bytes = self.lib.vqvae_resstack_workspace_bytes(C.byref(d0), nb)

        def fn(b):
            Wp = (C.c_void_p * nb)(*[b['Ws%d' % l].ptr for l in range(nb)])
            bp = (C.c_void_p * nb)(*[b['bs%d' % l].ptr for l in range(nb)])
            self.call('vqvae_resstack_skip_prepare', C.byref(d0), nb, Wp, bp, b.ws.ptr, ws_bytes)
        # (the tail of the workspace belongs to the other resstack entry points: judged through _fwd_prepared)
        return run_contract(self.gpu, fn, dict(self.weights, ws=Out((ws_bytes,), np.uint8, exact=False)))['ws']

    # -- backward --------------------------------------------------------------------------------------------------
    def block_backward(self, i):
        d = self.desc(i, self.bwd_bits[i])
        last = i == self.nb - 1
        B, Cr, Cd, Ch, Cs, T, Tl = self.B, self.Cr, self.Cd, self.Ch, self.Cs, self.T, self.Tl
        ghf, gxf = _fmt(d.storage, GHX2, GH16), _fmt(d.storage, 0, GX16)
        nt = T // 128
        specs = dict(self.weights, x=In(self.x[i]), gates=In(self.gates[i]), z=In(self.z[i]), g_skip=In(self.inp['gy']),
                     gx=_out_for((B, Cr, T), gxf), gh=_out_for((B, Cd, T), ghf), ws=Ws(self.rb_ws(i)), slab=In(self.slab))
        if not last:
            specs['g_res'] = In(self.gx[i + 1])
        if self.f16:
            specs['gskipw'] = In(_words(np.abs(self.inp['gy']).max()))
            specs['ghw'], specs['gxw'] = Out(init=ZERO_WORDS), Out(init=ZERO_WORDS)
            if not last:
                specs['gresw'] = In(self.gx_words[i + 1])
            if ghf == 'x2':
                specs['ghscale'] = Out(init=ZERO_WORDS)
            if self.fused:
                specs['pb'] = Out((B, nt, Cd, 4))
                specs.update(v0=In(self.tab['v0'], index_range=(0, Tl - 1)), w0=In(self.tab['w0']), w1=In(self.tab['w1']))

        def fn(b):
            self.slab_image(b)
            am = None
            if self.f16:
                pb = [b.pb.ptr, b.v0.ptr, b.w0.ptr, b.w1.ptr, Tl] if self.fused else [None, None, None, None, 0]
                am = C.byref(self.L.ResblockAmax(None, None, None if last else b.gresw.ptr, b.gskipw.ptr, b.ghw.ptr, b.gxw.ptr,
                                                 None, None, b.ghscale.ptr if ghf == 'x2' else None, *pb))
            self.call('vqvae_resblock_bwd_packed', C.byref(d), C.byref(self.params(b, i)), b.x.ptr, b.gates.ptr, b.z.ptr,
                      None if last else b.g_res.ptr, b.g_skip.ptr, b.gx.ptr, b.gh.ptr, b.ws.ptr, self.rb_ws(i),
                      b.slab.ptr + i * self.per, am)
        r = run_contract(self.gpu, fn, specs)
        self.gh[i], self.gx[i] = r['gh'], r['gx']
        self.gh_dec[i] = _decode(r['gh'], (B, Cd, T), ghf, r.get('ghscale'))
        self.gx_dec[i] = _decode(r['gx'], (B, Cr, T), gxf)
        if self.f16:
            self.gh_words[i], self.gx_words[i], self.gh_scale[i] = r['ghw'], r['gxw'], r.get('ghscale')
            self.pb_part[i] = r.get('pb')
        return r

    def check_backward(self, i, ref, r):
        self.tol(self.gh_dec[i], ref['gh'][i], 'gh of block %d' % i)
        self.tol(self.gx_dec[i], ref['gx'][i], 'gx of block %d' % i)
        if self.f16:
            self.check_words('gh', i, r['ghw'], self.gh_dec[i], self.bwd_bits[i] & GHX2, r.get('ghscale'))
            self.check_words('gx', i, r['gxw'], self.gx_dec[i], 0)

    def _acc(self, rs, acc, shape):
        init = _f32(rs.standard_normal(shape)) if acc else None
        return init, (Out(init=init) if acc else Out(shape))

    def dil_wgrad(self, ref, rs):
        """One launch per kind of (x, gh) storage, as wavenet._dil_wgrad groups the blocks; accumulate 0 and 1; in the
        accumulate = 0 call of a group of several blocks the SECOND block's gWd and the first block's gbd are NULL."""
        Cr, Cd, T = self.Cr, self.Cd, self.T
        kinds = {}
        for l in range(self.nb):
            kinds.setdefault((self.bwd_bits[l] & (XX2 | X16), self.bwd_bits[l] & (GHX2 | GH16)), []).append(l)
        for (xb, gb), sel in sorted(kinds.items()):
            n = len(sel)
            d = self.desc(sel[0], xb | gb)
            ws_bytes = self.lib.vqvae_resstack_dil_wgrad_workspace_bytes(C.byref(d), n)
            for acc in (0, 1):
                nullW = sel[1] if (not acc and n > 1) else None
                nullb = sel[0] if (not acc and n > 1) else None
                specs, init = dict(ws=Ws(ws_bytes)), {}
                for l in sel:
                    specs['x%d' % l], specs['gh%d' % l] = In(self.x[l]), In(self.gh[l])
                    if self.f16:
                        specs['xa%d' % l] = In(self.x_scale[l] if xb == XX2 else self.x_words[l])
                        specs['ga%d' % l] = In(self.gh_scale[l] if gb == GHX2 else self.gh_words[l])
                    if l != nullW:
                        init['W%d' % l], specs['gW%d' % l] = self._acc(rs, acc, (Cd, Cr, K))
                    if l != nullb:
                        init['b%d' % l], specs['gb%d' % l] = self._acc(rs, acc, (Cd,))

                def fn(b):
                    pa = lambda k, skip=None: (C.c_void_p * n)(*[None if l == skip else b['%s%d' % (k, l)].ptr for l in sel])
                    self.call('vqvae_resstack_dil_wgrad', C.byref(d), n, (C.c_int * n)(*[self.dils[l] for l in sel]),
                              pa('x'), pa('gh'), pa('gW', nullW), pa('gb', nullb), acc, b.ws.ptr, ws_bytes,
                              pa('xa') if self.f16 else None, pa('ga') if self.f16 else None)
                r = run_contract(self.gpu, fn, specs)
                for l in sel:
                    gW64, gb64 = ref['grads'][l]['conv']
                    if l != nullW:
                        self.tol(r['gW%d' % l], gW64, 'gWd of block %d, accumulate %d' % (l, acc), addend=init['W%d' % l] if acc else None)
                    if l != nullb:
                        self.tol(r['gb%d' % l], gb64, 'gbd of block %d, accumulate %d' % (l, acc), addend=init['b%d' % l] if acc else None)

    def res_skip_wgrad(self, ref, rs):
        d0, nb, Ch = self.desc(0, self.bwd_bits[0]), self.nb, self.Ch
        ws_bytes = self.lib.vqvae_resstack_workspace_bytes(C.byref(d0), nb)
        for acc in (0, 1):
            # res: g_res_l = gx_{l+1}; the last block has none (NULL, with NULL destinations)
            specs, init = dict(ws=Ws(ws_bytes)), {}
            for l in range(nb):
                specs['z%d' % l] = In(self.z[l])
                if l < nb - 1:
                    specs['g%d' % l] = In(self.gx[l + 1])
                    if self.f16:
                        specs['a%d' % l] = In(self.gx_words[l + 1])
                    init['W%d' % l], specs['gW%d' % l] = self._acc(rs, acc, (self.Cr, Ch, 1))
                    init['b%d' % l], specs['gb%d' % l] = self._acc(rs, acc, (self.Cr,))

            def fn(b):
                pa = lambda k, stop=nb - 1: (C.c_void_p * nb)(*[b['%s%d' % (k, l)].ptr if l < stop else None for l in range(nb)])
                self.call('vqvae_resstack_res_wgrad', C.byref(d0), nb, pa('g'), pa('z', nb), pa('gW'), pa('gb'), acc, b.ws.ptr,
                          ws_bytes, pa('a') if self.f16 else None)
            if nb > 1:
                r = run_contract(self.gpu, fn, specs)
                for l in range(nb - 1):
                    gW64, gb64 = ref['grads'][l]['res']
                    self.tol(r['gW%d' % l], gW64, 'gWr of block %d, accumulate %d' % (l, acc), addend=init['W%d' % l] if acc else None)
                    self.tol(r['gb%d' % l], gb64, 'gbr of block %d, accumulate %d' % (l, acc), addend=init['b%d' % l] if acc else None)
            # skip
            specs, init = dict(ws=Ws(ws_bytes), g_skip=In(self.inp['gy'])), {}
            if self.f16:
                specs['gskipw'] = In(_words(np.abs(self.inp['gy']).max()))
            for l in range(nb):
                specs['z%d' % l] = In(self.z[l])
                init['W%d' % l], specs['gW%d' % l] = self._acc(rs, acc, (self.Cs, Ch, 1))
                init['b%d' % l], specs['gb%d' % l] = self._acc(rs, acc, (self.Cs,))

            def fn2(b):
                pa = lambda k: (C.c_void_p * nb)(*[b['%s%d' % (k, l)].ptr for l in range(nb)])
                self.call('vqvae_resstack_skip_wgrad', C.byref(d0), nb, b.g_skip.ptr, pa('z'), pa('gW'), pa('gb'), acc, b.ws.ptr,
                          ws_bytes, b.gskipw.ptr if self.f16 else None)
            r = run_contract(self.gpu, fn2, specs)
            for l in range(nb):
                gW64, gb64 = ref['grads'][l]['skip']
                self.tol(r['gW%d' % l], gW64, 'gWs of block %d, accumulate %d' % (l, acc), addend=init['W%d' % l] if acc else None)
                self.tol(r['gb%d' % l], gb64, 'gbs of block %d, accumulate %d' % (l, acc), addend=init['b%d' % l] if acc else None)

    def gcond_bwd(self, ref, rs):
        """vqvae_resstack_gcond_bwd reads fp32 gh (storage 0; the packed chain itself never calls it: its condition gradient goes
        through the latent-rate projection): it is handed the chain's gh, decoded where they were kept pre-split, over the
        blocks' Wc -- the condition gradient of the materialised form of the same chain.  Not in 'bfloat16' (a bf16 gh is
        refused by the entry point)."""
        if self.mode == 'bfloat16':
            return
        d0, nb, B, Cc, T = self.desc(0, 0), self.nb, self.B, self.Cc, self.T
        ws_bytes = self.lib.vqvae_resstack_workspace_bytes(C.byref(d0), nb)
        ghs = [_f32(g) for g in self.gh_dec]
        want = sum(np.einsum('oc,bot->bct', self.inp['blocks'][l]['condition_proj'][0][:, :, 0].astype(np.float64),
                             ghs[l].astype(np.float64)) for l in range(nb))
        self.tol(want, ref['gcond'], 'the reference of gcond itself (the chain\'s gh)')
        for acc in (0, 1):
            init, out = self._acc(rs, acc, (B, Cc, T))
            specs = dict(self.weights, ws=Ws(ws_bytes), gcond=out)
            for l in range(nb):
                specs['gh%d' % l] = In(ghs[l])

            def fn(b):
                pa = lambda k: (C.c_void_p * nb)(*[b['%s%d' % (k, l)].ptr for l in range(nb)])
                self.call('vqvae_resstack_gcond_bwd', C.byref(d0), nb, pa('Wc'), pa('gh'), b.gcond.ptr, acc, b.ws.ptr, ws_bytes)
            r = run_contract(self.gpu, fn, specs)
            self.tol(r['gcond'], ref['gcond'], 'gcond, accumulate %d' % acc, addend=init)

    def pullback(self, ref):
        """The fused pull-back's second half over the pb_part of every block: vqvae_pullback_reduce, and _reduce_into for the
        blocks 1 .. n-1 inside a gP whose batch stride is 7 columns wider than the rows written."""
        if not self.fused:
            return
        nb, B, T, Cd, Tl = self.nb, self.B, self.T, self.Cd, self.Tl
        part = np.stack(self.pb_part)
        io = dict(part=In(part), v0=In(self.tab['v0'], index_range=(0, Tl - 1)))
        r = run_contract(self.gpu, lambda b: self.call('vqvae_pullback_reduce', b.part.ptr, b.v0.ptr, nb, B, T, Cd, Tl, b.gP.ptr),
                         dict(io, gP=Out((B, nb * Cd, Tl))))
        self.tol(r['gP'], ref['gP'], 'gP (vqvae_pullback_reduce)')
        if nb < 2:
            return
        rows, stride = (nb - 1) * Cd * Tl, nb * Cd * Tl + 7
        valid = np.zeros((B, stride), bool)
        valid[:, :rows] = True
        r2 = run_contract(self.gpu, lambda b: self.call('vqvae_pullback_reduce_into', b.part.ptr + part[0].nbytes, b.v0.ptr, nb - 1,
                                                        B, T, Cd, Tl, b.gP.ptr, stride),
                          dict(io, gP=Out((B, stride), valid=valid)))
        got = r2['gP'][:, :rows].reshape(B, (nb - 1) * Cd, Tl)
        np.testing.assert_array_equal(got, r['gP'][:, Cd:], 'reduce_into of blocks 1.. == the same rows of reduce')


def _run_forward(ch, ref, check=True):
    ch.pack()
    for i in range(ch.nb):
        r = ch.block_forward(i)
        if check:
            ch.check_forward(i, ref, r)


def _run_chain(gpu, row, mode):
    name, Cr, Cs, Cc, T, Tl, B, dils = row
    ref = _reference(row)
    ch = Chain(gpu, row, mode)
    fwd, bwd, fused = _expect_bits(row, mode)
    assert (ch.fwd_bits, ch.bwd_bits, ch.fused) == (fwd, bwd, fused), \
        '%s %s runs with storage %s / %s, fused pull-back %s; the predicates say %s / %s, %s' % (
            name, mode, ch.fwd_bits, ch.bwd_bits, ch.fused, fwd, bwd, fused)
    rs = _rs('chain_abi_acc', row)
    _run_forward(ch, ref)
    # the skip sum: accumulate x relu, and the same in two halves
    prepared = ch.skip_prepare()
    for acc in (0, 1):
        for relu in (0, 1):
            init = _f32(rs.standard_normal((B, Cs, T))) if acc else None
            want = ref['skip'] + (init if acc else 0)
            want = np.maximum(want, 0) if relu else want
            r = ch.skip_forward(acc, relu, init)
            ch.tol(r['skip'], want, 'skip, accumulate %d relu %d' % (acc, relu), scaled=False)
            # vqvae_resstack_skip_fwd is stage 1 | stage 2 of resstack_skip_impl over the same workspace layout: the same
            # kernel over the same slabs
            r2 = ch.skip_forward(acc, relu, init, prepared=prepared)
            np.testing.assert_array_equal(r2['skip'], r['skip'], 'skip_fwd_prepared == skip_fwd (accumulate %d relu %d)' % (acc, relu))
            if ch.f16:
                np.testing.assert_array_equal(r2['words'], r['words'])
    for i in range(ch.nb - 1, -1, -1):
        ch.check_backward(i, ref, ch.block_backward(i))
    ch.dil_wgrad(ref, rs)
    ch.res_skip_wgrad(ref, rs)
    ch.gcond_bwd(ref, rs)
    ch.pullback(ref)
    return ch


@pytest.mark.parametrize('row', ROWS)
def test_packed_chain_contract(gpu, matmul_mode, row):
    """Every entry point of the packed chain under zones / inputs_only / maxima and against the float64 chain."""
    ch = _run_chain(gpu, row, matmul_mode)
    if row[0] == 'c256_T256' and matmul_mode == 'float32x2':      # spelled out once: RES | GSIG, X | RES | GSIG, X | GSIG, each + GH
        assert (ch.fwd_bits, ch.bwd_bits, ch.fused) == ([384, 448, 320], [416, 480, 352], True)
        assert len(ch.ratios) == 2 + 3                            # two pre-split res, three pre-split gh
    if matmul_mode != 'float32x2':
        assert ch.fwd_bits == ch.bwd_bits == [0] * ch.nb and not ch.fused


def _rel_l2(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


class Bf16Chain(Chain):
    """'bfloat16': the bar of test_gpu_chain_domain's bf16 rows per tensor -- e_ref = the bf16 oracle's relative L2 distance
    from the float64 chain; device against the bf16 oracle <= 2 e_ref + 1e-2, against float64 <= 1.5 e_ref + 1e-2."""

    def tol(self, got, want16, name, scaled=True, addend=None):
        want64 = self._pair[id(want16)]
        if addend is not None:                                 # the caller's addend of an accumulate = 1 call is taken off again
            got = np.asarray(got, np.float64) - addend
        e_pair, e_dev, e_ref = _rel_l2(got, want16), _rel_l2(got, want64), _rel_l2(want16, want64)
        print('CHAIN_ABI %s bfloat16 %s: vs bf16 oracle %.3e, vs float64 %.3e, e_ref %.3e' % (self.row[0], name, e_pair, e_dev, e_ref))
        assert e_pair <= 2.0 * e_ref + 1e-2 and e_dev <= 1.5 * e_ref + 1e-2, \
            '%s %s: relative L2 vs the bf16 oracle %.3e, vs float64 %.3e (e_ref %.3e)' % (self.row[0], name, e_pair, e_dev, e_ref)


def _pair_refs(ref16, ref64):
    """id(array of the bf16 oracle) -> the float64 chain's array of the same tensor."""
    pair = {}
    for k in ('x', 'gates', 'z', 'gh', 'gx'):
        for a, b in zip(ref16[k], ref64[k]):
            if a is not None:
                pair[id(a)] = b
    for k in ('skip', 'gP', 'gcond'):
        pair[id(ref16[k])] = ref64[k]
    for g16, g64 in zip(ref16['grads'], ref64['grads']):
        for n in ORDER:
            if g16[n] is not None:
                for a, b in zip(g16[n], g64[n]):
                    pair[id(a)] = b
    return pair


@pytest.mark.parametrize('row', BF16_ROWS)
def test_packed_chain_contract_bf16(gpu, bf16_mode, row):
    """The 256-channel row at T = 256 (X / RES / GX / GRES / GH stored as bf16, z and the gates too) and at T = 192 (GH, z and
    the gates only): the stored tensors are 2-byte elements in the first half of fp32-sized buffers, the other half keeps
    its poison bits."""
    name, Cr, Cs, Cc, T, Tl, B, dils = row
    ref64 = _reference(row)
    ref16 = _chain(row, _inputs(row), np.float32)
    ch = Bf16Chain(gpu, row, 'bfloat16')
    ch._pair = _pair_refs(ref16, ref64)
    fwd, bwd, fused = _expect_bits(row, 'bfloat16')
    assert (ch.fwd_bits, ch.bwd_bits, ch.fused) == (fwd, bwd, False), (ch.fwd_bits, ch.bwd_bits, fwd, bwd)
    assert ch.zfmt == 'bf16' and all(b & GH16 for b in bwd) and bool(bwd[1] & X16) == (T % 128 == 0)
    rs = _rs('chain_abi_acc16', row)
    _run_forward(ch, ref16)
    prepared = ch.skip_prepare()
    r = ch.skip_forward(0, 0)
    ch.tol(r['skip'], ref16['skip'], 'skip')
    r2 = ch.skip_forward(0, 0, prepared=prepared)
    np.testing.assert_array_equal(r2['skip'], r['skip'])
    for i in range(ch.nb - 1, -1, -1):
        ch.check_backward(i, ref16, ch.block_backward(i))
    ch.dil_wgrad(ref16, rs)
    ch.res_skip_wgrad(ref16, rs)


# --------------------------------------------------------------------------- #
# the dilated conv's weight gradient on its LDS-DMA path, both operands stored
# --------------------------------------------------------------------------- #
DMA_DILS = (1, 3, 32, 40, 255)          # 32-column steps: 32 is a whole step in front of the row, 1 / 3 / 40 / 255 cross its first sample


def _dma_reference(gv, xv, dils):
    out = []
    g64, x64 = gv.astype(np.float64), xv.astype(np.float64)
    T = x64.shape[2]
    for dil in dils:
        gW = np.zeros((g64.shape[1], x64.shape[1], K))
        gW[:, :, 1] = np.einsum('bot,bct->oc', g64, x64)
        if dil < T:
            gW[:, :, 0] = np.einsum('bot,bct->oc', g64[:, :, dil:], x64[:, :, :T - dil])
        out.append((gW, g64.sum(axis=(0, 2))))
    return out


def _dma_contract(gpu, form):
    """B = 2, T = 256 is the smallest shape of the wide plan's domain with more than one batch item (wgrad_dma_shape: M % 256,
    T % 32, Cr % 256 -- it has no lower limit on B or T; the storage bits need T % 128 == 0), five blocks in one launch."""
    L = _L()
    lib = L.load()
    B, T, Cr = 2, 256, 256
    n = len(DMA_DILS)
    rs = _rs('dma', form)
    x, g = _f32(0.7 * rs.standard_normal((B, Cr, T))), _f32(3e-3 * rs.standard_normal((B, Cr, T)))
    d = L.ResblockDesc(B, T, Cr, Cr, Cr, 192, K, 1, (GHX2 | XX2) if form == 'x2' else (GH16 | X16))
    sup = lib.vqvae_resblock_f16x2_storage(C.byref(d)) if form == 'x2' else lib.vqvae_resblock_bf16_storage(C.byref(d))
    assert sup & d.storage == d.storage, sup
    if form == 'x2':
        xw, xs, xv = _presplit(x, 1.7 * np.abs(x).max())
        gw, gs, gv = _presplit(g, 5.0 * np.abs(g).max())
        bar = 1e-5                                             # three fp16 products of 22-bit operands, fp32 accumulation (test_dil_wgrad_lds_dma_presplit_operands)
    else:
        def half(a):                                           # 2-byte elements in the first half of an fp32-sized buffer; the rest is finite junk
            buf = _bf16_round(rs.standard_normal(2 * a.size))
            buf[:a.size] = _bf16_round(a).reshape(-1)
            return buf
        xw, gw = half(x), half(g)
        xv, gv = _dec_bf16(xw, x.shape), _dec_bf16(gw, g.shape)
        xs = gs = None
        bar = 1e-5                                             # exact products of bf16 operands, fp32 accumulation over B T = 512 terms
    ws_bytes = lib.vqvae_resstack_dil_wgrad_workspace_bytes(C.byref(d), n)
    want = _dma_reference(gv, xv, DMA_DILS)
    for acc in (0, 1):
        nullW, nullb = (2, 0) if not acc else (None, None)
        specs, init = dict(x=In(xw), g=In(gw), ws=Ws(ws_bytes)), {}
        if form == 'x2':
            specs.update(xs=In(xs), gs=In(gs))
        for l in range(n):
            if l != nullW:
                init['W%d' % l] = _f32(1e-3 * rs.standard_normal((Cr, Cr, K)))
                specs['gW%d' % l] = Out(init=init['W%d' % l]) if acc else Out((Cr, Cr, K))
            if l != nullb:
                init['b%d' % l] = _f32(1e-3 * rs.standard_normal(Cr))
                specs['gb%d' % l] = Out(init=init['b%d' % l]) if acc else Out((Cr,))

        def fn(b):
            rep = lambda a: (C.c_void_p * n)(*[a.ptr] * n)
            pa = lambda k, skip: (C.c_void_p * n)(*[None if l == skip else b['%s%d' % (k, l)].ptr for l in range(n)])
            _call(gpu, 'vqvae_resstack_dil_wgrad', C.byref(d), n, (C.c_int * n)(*DMA_DILS), rep(b.x), rep(b.g), pa('gW', nullW),
                  pa('gb', nullb), acc, b.ws.ptr, ws_bytes, rep(b.xs) if form == 'x2' else None, rep(b.gs) if form == 'x2' else None)
        r = run_contract(gpu, fn, specs)
        for l in range(n):
            if l != nullW:
                assert_close_scaled(r['gW%d' % l], want[l][0] + (init['W%d' % l] if acc else 0), bar, 'gWd, dil %d, accumulate %d' % (DMA_DILS[l], acc))
            if l != nullb:
                assert_close_scaled(r['gb%d' % l], want[l][1] + (init['b%d' % l] if acc else 0), bar, 'gbd, dil %d, accumulate %d' % (DMA_DILS[l], acc))


def test_dil_wgrad_dma_contract_presplit(gpu):
    gpu.set_matmul_dtype('float32x2')
    try:
        _dma_contract(gpu, 'x2')
    finally:
        gpu.set_matmul_dtype(gpu.default_matmul_dtype())


def test_dil_wgrad_dma_contract_bf16(gpu, bf16_mode):
    _dma_contract(gpu, 'bf16')


# --------------------------------------------------------------------------- #
# published maxima under a spike
# --------------------------------------------------------------------------- #
SPIKE_CLASSES = {'c256': ROW_BASE.values[0], 'c512': ('c512_T256_spike', 512, 256, 128, 256, 4, 2, (1, 2, 4))}


def _spike_at(where, B, Cc, T):
    return {'first': (0, 0, 0), 'last_all': (B - 1, Cc - 1, T - 1), 'last_rows': (0, Cc - 1, 100)}[where]


@pytest.mark.parametrize('where', ['first', 'last_all', 'last_rows'])
@pytest.mark.parametrize('cls', sorted(SPIKE_CLASSES))
def test_published_maximum_chain(gpu, cls, where):
    """'float32x2', magnitudes ~1 everywhere except ONE element of 64x planted where an epilogue is most likely to miss it:
    the first tile, the last tile of the last batch item, the last row block.
      fwd_packed `res`:  x_0[b, c, t] = 64 -> res_0[b, c, t] ~ 64 (res = Wr z + br + x, |z| <= 1);
      bwd_packed `gx`, `gh`:  block 0's g_res[b, c, t] = 1024 (the gx block 1 hands it, spiked on the host with its words
                         raised accordingly) -> gx_0[b, c, t] ~ 1024, and gz = Wr^T g_res puts the extreme gh in column t of b;
      skip_fwd `skip_amax_out`:  |z| <= 1 bounds the GEMM, so the spike arrives through accumulate = 1 (the caller's addend).
    Each published word must still cover its tensor (check_words / skip_forward assert it), and the consumers run on."""
    row = SPIKE_CLASSES[cls]
    name, Cr, Cs, Cc, T, Tl, B, dils = row
    gpu.set_matmul_dtype('float32x2')
    try:
        inp = dict(_inputs(row))
        b, c, t = _spike_at(where, B, Cr, T)
        inp['x'] = inp['x'].copy()
        inp['x'][b, c, t] = 64.0
        ref = _chain(row, inp)
        ch = Chain(gpu, row, 'float32x2', inp)
        assert all(bits & GSIG for bits in ch.fwd_bits) and ch.fwd_bits[0] & RESX2 and all(bits & GHX2 for bits in ch.bwd_bits)
        _run_forward(ch, ref)
        assert np.abs(ch.x_dec[1][b, c, t]) == np.abs(ch.x_dec[1]).max() > 60.0
        # skip: the addend carries the spike
        bs_, cs_, ts_ = _spike_at(where, B, Cs, T)
        init = _f32(_rs('spike_skip', cls, where).standard_normal((B, Cs, T)))
        init[bs_, cs_, ts_] = -64.0
        r = ch.skip_forward(1, 0, init)
        assert np.abs(r['skip'][bs_, cs_, ts_]) == np.abs(r['skip']).max() > 55.0
        ch.tol(r['skip'], ref['skip'] + init, 'skip with a spiked addend', scaled=False)
        # backward: blocks n-1 .. 1 as they are, then block 0 with a spiked g_res
        for i in range(ch.nb - 1, 0, -1):
            ch.check_backward(i, ref, ch.block_backward(i))
        g = ch.gx[1].copy()
        g[b, c, t] = 1024.0                                    # (64 x a weight of Wr would not stand out of a gh of ~5)
        ch.gx[1] = g
        ch.gx_words[1] = _words(np.abs(g).max())
        r = ch.block_backward(0)
        gx, gh = ch.gx_dec[0], ch.gh_dec[0]
        assert np.abs(gx[b, c, t]) == np.abs(gx).max() > 55.0
        assert np.abs(gh[b, :, t]).max() == np.abs(gh).max(), 'the extreme gh is in the spiked column'
        ch.check_words('gh', 0, r['ghw'], gh, True, r['ghscale'], tight=False)      # (the bound is 64 x a column norm of Wr: cover only)
        ch.check_words('gx', 0, r['gxw'], gx, 0)
    finally:
        gpu.set_matmul_dtype(gpu.default_matmul_dtype())
