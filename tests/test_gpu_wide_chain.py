"""The float32x2 PRE-SPLIT chain for the reference's default decoder (params.py: residual_channels = dilated_channels =
512, skip_channels = 256, condition 512 + 128): the 'wide' shape class of vqvae_resblock_f16x2_storage.

What runs where (csrc/conv_api.hip, f16x2_storage_supported): the gate GEMM and the backward-data GEMM are the 256 x 128-
tile two-tap kernels over pre-split operands (two row tiles; the packed gate slab pairs tanh row c with sigmoid row
256 + c inside every 64-row group), the residual 1x1 is lin256_stream_kernel (csrc/lin_stream_wide.hip: 256 -> 512 rows,
two row slices per column tile, x_{l+1} stored pre-split), the gate derivative writes gh pre-split from its tiled kernel,
the dilated weight gradients run on wgrad3_dma_kernel (2 x 4 tiles of 256 x 256 per block), and gh is pulled back to the
latent rate by vqvae_upsample_linear_bwd_f16x2 (vqvae_get_fused_pullback answers 0 for 256 gate channels)."""
import ctypes as C

import numpy as np
import pytest

import vqvae_oracle as O
from helpers import assert_close, assert_close_scaled, to4
from test_gpu_kernels import _rb_params

pytestmark = pytest.mark.gpu

B, T = 4, 7680
CR = CD = 512
CS = 256
CL, G, NSPK = 512, 128, 7          # local condition (d = 512) + speaker embedding (128) = 640 condition channels
ORDER = ['conv', 'condition_proj', 'res', 'skip']
ALL_BITS = 32 | 64 | 128 | 256     # VQVAE_STORE_GH_F16X2 | X_F16X2 | RES_F16X2 | GATES_SIG


def _dev(gpu, a):
    return gpu.to_device(np.ascontiguousarray(a))


def _stack_inputs(seed, dils, quiet=None, T=T):
    rs = np.random.RandomState(seed)
    Tl = T // 64
    blocks = [_rb_params(rs, CR, CD, CS, CL + G, 2) for _ in dils]
    x = rs.standard_normal((B, CR, T)).astype(np.float32)
    local = rs.standard_normal((B, CL, Tl)).astype(np.float32)
    E = rs.standard_normal((NSPK, G)).astype(np.float32)
    ids = rs.randint(0, NSPK, B).astype(np.int32)
    gy = rs.standard_normal((B, CS, T)).astype(np.float32)
    if quiet is not None:
        x[-1] *= quiet
        gy[-1] *= quiet
    return blocks, x, local, E, ids, gy


def _run_stack(gpu, dils, blocks, x, local, E, ids, gy, keep=False):
    """ResidualStackFunction over the latent-rate condition, forward and backward -> (outputs by name, storage bits used
    per block, the function node after the forward's words were read when ``keep``)."""
    from vqvae_amd import functions as F
    from vqvae_amd.core import Variable
    from vqvae_amd.wavenet import ResidualStackFunction
    vx = Variable(_dev(gpu, to4(x)))
    vlocal, vE = Variable(_dev(gpu, to4(local))), Variable(_dev(gpu, E))
    vcond = F.condition_assemble(vlocal, vE, _dev(gpu, ids), 64)
    assert isinstance(vcond.data, F.LazyUpsampled)
    pv = []
    for blk in blocks:
        for n in ORDER:
            pv += [Variable(_dev(gpu, to4(blk[n][0]))), Variable(_dev(gpu, blk[n][1]))]
    fn = ResidualStackFunction(dils)
    skip = fn.apply([vx, vcond] + pv)[0]
    used = [d.storage for d in fn.descs]
    kept = None
    if keep:              # the stored tensors and their words, before the backward releases them
        gpu.synchronize()
        kept = {'words': fn.words.host() if fn.words is not None else None,
                'x': [s[0].get() for s in fn.saved], 'z': [s[2].get() for s in fn.saved]}
    out = {'skip': skip.data.get()}
    skip.grad = _dev(gpu, to4(gy))
    skip.backward()
    used = [u | d.storage for u, d in zip(used, fn.descs)]
    out['gx'] = vx.grad.get()
    out['glocal'] = vlocal.grad.get()
    out['gE'] = vE.grad.get()
    for i, v in enumerate(pv):
        if v.grad is not None:
            out['p%d' % i] = v.grad.get()
    return out, used, kept


_ORACLE = {}


def _stack_oracle(seed, dils):
    """The oracle's per-block restatement fed the materialised (B, 640, T) condition (net.py:54-63, modules.py:89-96)."""
    key = (seed, tuple(dils))
    if key in _ORACLE:
        return _ORACLE[key]
    blocks, x, local, E, ids, gy = _stack_inputs(seed, dils)
    Tl = T // 64
    cond = np.concatenate([O.upsample_fwd(local, T), np.repeat(E[ids][:, :, None], T, axis=2)], axis=1).astype(np.float32)
    h, caches, skip_ref = x, [], None
    for blk, d in zip(blocks, dils):
        h, sk, cch = O.resblock_fwd(blk, h, cond, d)
        caches.append(cch)
        skip_ref = sk if skip_ref is None else skip_ref + sk
    g_res, gcond_ref, bg = None, np.zeros_like(cond), [None] * len(dils)
    for i in range(len(dils) - 1, -1, -1):
        g_res, gc, bg[i] = O.resblock_bwd(blocks[i], caches[i], cond, dils[i], g_res, gy)
        gcond_ref += gc
    glocal_ref = O.upsample_bwd(gcond_ref[:, :CL], Tl)
    gE_ref = np.zeros_like(E, dtype=np.float64)
    np.add.at(gE_ref, ids, gcond_ref[:, CL:].sum(axis=2, dtype=np.float64))
    _ORACLE[key] = (skip_ref, g_res, glocal_ref, gE_ref, bg)
    return _ORACLE[key]


def test_wide_storage_bits_on_the_device_library(gpu):
    """The query the chain plans its storage from, with the device initialised: all four bits for the default decoder's
    block in 'float32x2', none with the switch off, the 256-channel answer as before."""
    from vqvae_amd import _lib
    lib = _lib.load()
    gpu.set_matmul_dtype('float32x2')
    try:
        d = _lib.ResblockDesc(B, T, CR, CD, CS, CL + G, 2, 512, 0)
        assert lib.vqvae_resblock_f16x2_storage(C.byref(d)) == ALL_BITS
        assert lib.vqvae_get_fused_pullback(C.byref(d)) == 0
        d256 = _lib.ResblockDesc(16, T, 256, 256, 256, 192, 2, 512, 0)
        assert lib.vqvae_resblock_f16x2_storage(C.byref(d256)) == ALL_BITS
        assert lib.vqvae_get_fused_pullback(C.byref(d256)) == 1
        gpu.set_presplit(0)
        assert lib.vqvae_resblock_f16x2_storage(C.byref(d)) == 0
    finally:
        gpu.set_presplit(7)
        gpu.set_matmul_dtype(gpu.default_matmul_dtype())


@pytest.mark.parametrize('dil', [1, 2, 512])
def test_wide_resblock_vs_oracle(gpu, matmul_mode, dil):
    """One ResidualBlock of the default decoder (512 / 512 / 256 channels, condition 640) at B = 4, T = 7680 against
    oracle.resblock_fwd / resblock_bwd: outputs and every gradient to 1e-4 of scale."""
    from vqvae_amd.core import Variable
    from vqvae_amd.wavenet import ResidualBlockFunction
    rs = np.random.RandomState(300 + dil)
    p = _rb_params(rs, CR, CD, CS, CL + G, 2)
    x = rs.standard_normal((B, CR, T)).astype(np.float32)
    c = rs.standard_normal((B, CL + G, T)).astype(np.float32)
    res_ref, skip_ref, cache = O.resblock_fwd(p, x, c, dil)
    g_res = rs.standard_normal(res_ref.shape).astype(np.float32)
    g_skip = rs.standard_normal(skip_ref.shape).astype(np.float32)
    gx_ref, gc_ref, gr = O.resblock_bwd(p, cache, c, dil, g_res, g_skip)
    vs = [Variable(_dev(gpu, to4(x))), Variable(_dev(gpu, to4(c)))]
    for n in ORDER:
        vs += [Variable(_dev(gpu, to4(p[n][0]))), Variable(_dev(gpu, p[n][1]))]
    res, skip = ResidualBlockFunction(dil).apply(vs)
    assert_close(res.data.get(), res_ref, 1e-4, 'res')
    assert_close(skip.data.get(), skip_ref, 1e-4, 'skip')
    gouts = res.creator.backward(tuple(range(10)), (Variable(_dev(gpu, to4(g_res))), Variable(_dev(gpu, to4(g_skip)))))
    assert_close_scaled(gouts[0].get(), gx_ref, 1e-4, 'gx')
    assert_close_scaled(gouts[1].get(), gc_ref, 1e-4, 'gcond')
    for i, n in enumerate(ORDER):
        assert_close_scaled(gouts[2 + 2 * i].get(), gr[n][0], 1e-4, 'gW ' + n)
        assert_close_scaled(gouts[3 + 2 * i].get(), gr[n][1], 1e-4, 'gb ' + n)


def test_wide_stack_vs_oracle(gpu, matmul_mode):
    """Four blocks (dilations 1, 2, 256, 512) of the default decoder's ResidualNet over the latent-rate condition against
    the oracle: skip sum and every gradient to 1e-4 of scale in every matmul mode.  In 'float32x2' the chain keeps its
    tensors pre-split (every storage bit the blocks' positions allow), its own bookkeeping -- the bound each pre-split
    tensor was split under -- exists for every block, and the run-time guard counts no violation."""
    from vqvae_amd import backend, wavenet
    dils = [1, 2, 256, 512]
    nb = len(dils)
    skip_ref, gx_ref, glocal_ref, gE_ref, bg = _stack_oracle(21, dils)
    f16 = matmul_mode == 'float32x2'
    backend.f32x2_contract_violations(reset=True)
    wavenet.KEEP_CONTRACT_WORDS, wavenet.LAST_CONTRACT_WORDS = True, None
    try:
        out, used, _ = _run_stack(gpu, dils, *_stack_inputs(21, dils))
    finally:
        wavenet.KEEP_CONTRACT_WORDS = False
    if f16:
        assert all(u & 32 and u & 256 for u in used), used
        assert used[0] & 128 and not used[0] & 64 and used[-1] & 64 and not used[-1] & 128 and all(u & 192 == 192 for u in used[1:-1]), used
        n, words = wavenet.LAST_CONTRACT_WORDS
        assert n == nb

        def f(what, l):
            return np.array(words[wavenet.ChainWords.index(nb, what, l)], np.uint32).view(np.float32)
        for l in range(nb):
            bg_, mg = f('gh_scale', l)[0], f('gh', l).max()
            assert bg_ >= mg > 0 and bg_ / mg < 2.0 ** 12, (l, bg_, mg)
            if l >= 1:
                bx, mx = f('x_scale', l)[0], f('x', l).max()
                assert bx >= mx > 0 and bx / mx < 2.0 ** 6, (l, bx, mx)
        assert backend.f32x2_contract_violations()['violations'] == 0
    else:
        assert all(u == 0 for u in used), used
    wavenet.LAST_CONTRACT_WORDS = None
    assert_close(out['skip'][..., 0], skip_ref, 1e-4, 'skip_connections')
    assert_close_scaled(out['gx'][..., 0], gx_ref, 1e-4, 'gx')
    assert_close_scaled(out['glocal'][..., 0], glocal_ref, 1e-4, 'g local condition')
    assert_close_scaled(out['gE'], gE_ref, 1e-4, 'g speaker embedding')
    for i in range(nb):
        for j, n in enumerate(ORDER):
            k = 'p%d' % (8 * i + 2 * j)
            if i == nb - 1 and n == 'res':          # unused residual branch of the last block (modules.py:89-96)
                assert k not in out
                continue
            assert_close_scaled(out[k].reshape(bg[i][n][0].shape), bg[i][n][0], 1e-4, 'block %d gW %s' % (i, n))
            assert_close_scaled(out['p%d' % (8 * i + 2 * j + 1)], bg[i][n][1], 1e-4, 'block %d gb %s' % (i, n))


def test_wide_presplit_changes_only_the_rounding_point(gpu):
    """Pre-split storage on (mask 7) against off (mask 0: every tensor fp32, the generic kernels) on the same four-block
    stack: every output and gradient agrees to 2e-6 of its scale; two runs with it on are bit-identical."""
    dils = [1, 2, 256, 512]
    gpu.set_matmul_dtype('float32x2')
    try:
        gpu.set_presplit(0)
        ref, used0, _ = _run_stack(gpu, dils, *_stack_inputs(22, dils))
        assert all(u == 0 for u in used0)
        gpu.set_presplit(7)
        got, used, _ = _run_stack(gpu, dils, *_stack_inputs(22, dils))
        assert all(u & 32 and u & 256 for u in used) and all(u & 192 == 192 for u in used[1:-1]), used
        assert set(got) == set(ref)
        for k in ref:
            assert_close_scaled(got[k], ref[k], 2e-6, k)
        again, _, _ = _run_stack(gpu, dils, *_stack_inputs(22, dils))
        for k in got:
            assert np.array_equal(got[k], again[k]), k
    finally:
        gpu.set_presplit(7)
        gpu.set_matmul_dtype(gpu.default_matmul_dtype())


def _presplit_decode(dwords, bound):
    """Stored dwords (fp16 hi | fp16 lo << 16 of x * 2^k, k = 14 - exponent(bound)) -> float64 values."""
    u = np.ascontiguousarray(dwords).view(np.uint32)
    hi = (u & 0xffff).astype(np.uint16).view(np.float16).astype(np.float64)
    lo = (u >> 16).astype(np.uint16).view(np.float16).astype(np.float64)
    e = int(np.floor(np.log2(float(bound))))
    return (hi + lo) * 2.0 ** (e - 14)


def test_streaming_wide_1x1_against_float64_over_the_stored_values(gpu):
    """lin256_stream_kernel, both instantiations, from the chain's own stored tensors: x_1 = Wr_0 z_0 + br_0 + x_0 (x_0 fp32)
    and x_2 = Wr_1 z_1 + br_1 + x_1 (x_1 pre-split), decoded from their dwords under the bound in their scale words,
    against float64 over the stored z and x.  The tiled kernel sums this contraction in another order (two interleaved
    halves), so the documented agreement is a rounding, not bits: three fp16 products per term and a 22-bit stored value
    -- 4e-6 of the bound, per element."""
    from vqvae_amd import wavenet
    dils = [1, 2, 4]
    gpu.set_matmul_dtype('float32x2')
    try:
        blocks, x, local, E, ids, gy = _stack_inputs(23, dils)
        _, used, kept = _run_stack(gpu, dils, blocks, x, local, E, ids, gy, keep=True)
    finally:
        gpu.set_matmul_dtype(gpu.default_matmul_dtype())
    assert used[0] & 128 and used[1] & 192 == 192, used
    nb, words = kept['words']

    def f(what, l):
        return np.array(words[wavenet.ChainWords.index(nb, what, l)], np.uint32).view(np.float32)
    prev = kept['x'][0].reshape(B, CR, T).astype(np.float64)
    for l in (0, 1):
        Wr, br = blocks[l]['res']
        z = kept['z'][l].reshape(B, CD // 2, T).astype(np.float64)
        want = np.einsum('rc,bct->brt', Wr[:, :, 0].astype(np.float64), z) + br.astype(np.float64)[None, :, None] + prev
        bound = float(f('x_scale', l + 1)[0])
        got = _presplit_decode(kept['x'][l + 1].reshape(B, CR, T), bound)
        assert bound >= np.abs(want).max()
        err = np.abs(got - want).max()
        assert err <= 4e-6 * bound, (l, err, bound)
        assert abs(float(f('x', l + 1).max()) - np.abs(want).max()) <= 1e-5 * bound      # the published maximum of x_{l+1}
        prev = got


@pytest.mark.parametrize('ratio', [1e-4])
def test_wide_presplit_chain_keeps_a_quiet_sample(gpu, ratio):
    """The dynamic-range contract through the default decoder's full depth (30 blocks, dilations 1 .. 512 three times,
    B = 4, T = 2048) with its pre-split tensors: a batch whose last sample is `ratio` of the others in x and in the
    output gradient still gets that sample's skip output and input gradient to 1e-4 of ITS OWN scale against the same
    chain in 'float32x3' (an exact three-way split of every operand: no scale, no bound).  The guard stays silent."""
    dils = [2 ** (i % 10) for i in range(30)]
    inp = _stack_inputs(24, dils, quiet=ratio, T=2048)
    try:
        gpu.set_matmul_dtype('float32x3')
        ref, _, _ = _run_stack(gpu, dils, *inp)
        gpu.set_matmul_dtype('float32x2')
        gpu.f32x2_contract_violations(reset=True)
        got, used, _ = _run_stack(gpu, dils, *inp)
        rep = gpu.f32x2_contract_violations()
    finally:
        gpu.set_matmul_dtype(gpu.default_matmul_dtype())
    assert all(u & 32 for u in used) and all(u & 192 == 192 for u in used[1:-1]), used
    assert rep['violations'] == 0 and rep['checked'] == 2 * len(dils) - 1, rep
    for k in ('skip', 'gx'):
        assert_close_scaled(got[k][-1], ref[k][-1], 1e-4, 'quiet sample: ' + k)
        assert_close_scaled(got[k][:-1], ref[k][:-1], 1e-4, 'loud samples: ' + k)
