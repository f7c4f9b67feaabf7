"""Per-call references of the packed decoder chain: for every entry point call, that call's mathematical function over the
values THAT CALL was handed (the decoded stored tensors its producer wrote, the fp32 weights, the float32 resize tables),
evaluated in `dtype` = float64 (the truth) or float32 (NumPy's own fp32 arithmetic: the yardstick `e32` of
tests/test_gpu_chain_accuracy.py).  Either way the operands are cast first and every contraction is np.matmul per tap, as
oracle/vqvae_oracle.py does (BLAS; no einsum).

Nothing here restates a kernel: no tiles, no splits, no storage.  Stored forms are the caller's business.

tests/test_host_chain_accuracy.py feeds each float64 function the float64 output of the one before it and requires
oracle.resblock_fwd / resblock_bwd / upsample_bwd of the whole chain back to 1e-12: a wrong tap order or lerp index here
cannot hide behind the accuracy margin."""
import numpy as np


def _c(a, dtype):
    return np.ascontiguousarray(np.asarray(a).astype(dtype))


def lerp_matrix(tab, Tl, dtype):
    """U (T, Tl) with y[..., t] = sum_p U[t, p] x[..., p] == w0[t] x[v0[t]] + w1[t] x[v0[t] + 1]; the pull-back is g @ U."""
    v0 = np.asarray(tab['v0'])
    T = v0.shape[0]
    U = np.zeros((T, Tl), dtype)
    i = np.arange(T)
    U[i, v0] += _c(tab['w0'], dtype)
    U[i, v0 + 1] += _c(tab['w1'], dtype)
    return U


def _shift(x, s):
    """x[..., t - s], zero in front of the row (s >= 0)."""
    T = x.shape[-1]
    y = np.zeros_like(x)
    if s < T:
        y[..., s:] = x[..., :T - s]
    return y


def _unshift(g, s):
    """The adjoint of _shift: g[..., t + s], zero behind the row."""
    T = g.shape[-1]
    y = np.zeros_like(g)
    if s < T:
        y[..., :T - s] = g[..., s:]
    return y


def _sigmoid(x):
    one = x.dtype.type(1)
    return one / (one + np.exp(-x))


def resblock_fwd_packed(x, Wd, P, tab, dil, Wr=None, br=None, z_in=None, bd=None, dtype=np.float64):
    """x (B, Cr, T); Wd (Cd, Cr, K); P (B, Cd, Tl) = this block's rows of the latent-rate projection (with bd inside when the
    caller sets vqvae_resblock_cproj::P_has_bd; else pass bd); z_in: the z the residual 1x1 reads (the stored z; None: the z
    computed here).  -> dict(h = the pre-activation, tanh, sigmoid, z[, res])."""
    x, Wd, P = _c(x, dtype), _c(Wd, dtype), _c(P, dtype)
    K = Wd.shape[2]
    h = np.matmul(P, lerp_matrix(tab, P.shape[2], dtype).T)
    for j in range(K):
        h = h + np.matmul(np.ascontiguousarray(Wd[:, :, j]), _shift(x, (K - 1 - j) * dil))
    if bd is not None:
        h = h + _c(bd, dtype)[None, :, None]
    Ch = h.shape[1] // 2
    out = dict(h=h, tanh=np.tanh(h[:, :Ch]), sigmoid=_sigmoid(h[:, Ch:]))
    out['z'] = out['tanh'] * out['sigmoid']
    if Wr is not None:
        z = out['z'] if z_in is None else _c(z_in, dtype)
        out['res'] = np.matmul(_c(Wr, dtype)[:, :, 0], z) + _c(br, dtype)[None, :, None] + x
    return out


def skip_fwd(Ws, bs, zs, dtype=np.float64):
    """sum_l Ws_l z_l + bs_l (accumulate 0, relu 0)."""
    y = None
    for W, b, z in zip(Ws, bs, zs):
        t = np.matmul(_c(W, dtype)[:, :, 0], _c(z, dtype)) + _c(b, dtype)[None, :, None]
        y = t if y is None else y + t
    return y


def resblock_bwd_packed(Wd, Wr, Ws, g_skip, g_res, gates, dil, z=None, gsig=False, gh_in=None, dtype=np.float64):
    """g_res = the gx the next block handed on (None: the last block); gates (B, 2 Ch, T) = tanh | sigmoid as handed; gsig:
    only the sigmoid half is valid and tanh = z / sigmoid (gemm_common.h, GemmArgs::gsig); gh_in: the gh the backward-data
    GEMM reads (resblock_bwd_impl hands it the STORED gh_out; None: the gh computed here).  -> dict(gh, gx)."""
    Wd, g_skip, gates = _c(Wd, dtype), _c(g_skip, dtype), _c(gates, dtype)
    K = Wd.shape[2]
    Ch = gates.shape[1] // 2
    gz = np.matmul(np.ascontiguousarray(_c(Ws, dtype)[:, :, 0].T), g_skip)
    if g_res is not None:
        g_res = _c(g_res, dtype)
        gz = gz + np.matmul(np.ascontiguousarray(_c(Wr, dtype)[:, :, 0].T), g_res)
    sb = gates[:, Ch:]
    if gsig:
        zz = _c(z, dtype)
        ta = np.where(sb != 0, zz / np.where(sb != 0, sb, 1), 0).astype(dtype)
    else:
        ta = gates[:, :Ch]
    one = dtype(1)
    gh = np.concatenate([gz * sb * (one - ta * ta), gz * ta * sb * (one - sb)], 1)
    ghr = gh if gh_in is None else _c(gh_in, dtype)
    gx = None
    for j in range(K):
        t = np.matmul(np.ascontiguousarray(Wd[:, :, j].T), _unshift(ghr, (K - 1 - j) * dil))
        gx = t if gx is None else gx + t
    if g_res is not None:
        gx = gx + g_res
    return dict(gh=gh, gx=gx)


def _wgrad(g, x):
    """sum_{b, t} g[b, o, t] x[b, c, t] -> (o, c)."""
    return np.matmul(g, np.ascontiguousarray(np.swapaxes(x, 1, 2))).sum(axis=0, dtype=g.dtype)


def dil_wgrad(x, gh, dil, K=2, dtype=np.float64):
    """-> gWd (Cd, Cr, K), gbd (Cd,) from the block's input x and its gh."""
    x, gh = _c(x, dtype), _c(gh, dtype)
    gW = np.stack([_wgrad(gh, _shift(x, (K - 1 - j) * dil)) for j in range(K)], 2)
    return gW, gh.sum(axis=(0, 2), dtype=dtype)


def lin_wgrad(z, g, dtype=np.float64):
    """-> gW (Co, Ch, 1), gb (Co,) of a 1x1 conv over z under the output gradient g (res: gx of the next block; skip: g_skip)."""
    z, g = _c(z, dtype), _c(g, dtype)
    return _wgrad(g, z)[:, :, None], g.sum(axis=(0, 2), dtype=dtype)


def gcond_bwd(Wcs, ghs, dtype=np.float64):
    """sum_l Wc_l^T gh_l: the condition gradient of the materialised form."""
    y = None
    for W, g in zip(Wcs, ghs):
        t = np.matmul(np.ascontiguousarray(_c(W, dtype)[:, :, 0].T), _c(g, dtype))
        y = t if y is None else y + t
    return y


def pullback(gh, tab, Tl, dtype=np.float64):
    """The adjoint of the lerp over one block's gh (B, Cd, T) -> (B, Cd, Tl)."""
    return np.matmul(_c(gh, dtype), lerp_matrix(tab, Tl, dtype))


# ---------------------------------------------------------------------------------------------------------------------------
# the two metrics and the bar
# ---------------------------------------------------------------------------------------------------------------------------
def metrics(got, want):
    """(relative L2 error, max error over the tensor's scale) of `got` against the float64 `want`."""
    g, w = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    assert g.shape == w.shape, (g.shape, w.shape)
    d = g - w
    return (float(np.linalg.norm(d) / max(np.linalg.norm(w), 1e-300)), float(np.abs(d).max() / max(np.abs(w).max(), 1e-300)))


FACTOR, FLOOR = 3.0, 1e-7


def bar(e32):
    """err <= 3 e32 + 1e-7.  3: faithful split arithmetic measures within 1.1x of NumPy's float32 at the chain's K, the
    smallest defect worth catching (one of float32x3's six products lost) at 7x.  1e-7: a 512-term bias sum comes out at
    9e-8 in NumPy's pairwise sum, and a fixed-order device tree need not match that."""
    return FACTOR * e32 + FLOOR


def seq_error(K):
    """The rms relative error of a K-term sum kept in ONE fp32 accumulator that is rounded at every addition: each rounding is
    uniform within u = 2^-24 of the partial sum, which after k terms of variance s^2 has size s sqrt(k), so the variances add
    up to sum_k u^2 k s^2 / 3 = u^2 s^2 K^2 / 6 against a result of size s sqrt(K):  u sqrt(K / 6).  One rounding per term
    is the fp32 MFMA's arithmetic and an upper bound for the split modes (three or six roundings per 16-deep step plus
    whatever v_mfma_f32_32x32x16_* does inside a step, which nobody has measured).  NumPy's float32 matmul does NOT grow
    this way (BLAS sums in blocks), so e32 alone is no yardstick for the chain's longest contractions."""
    return 2.0 ** -24 * np.sqrt(K / 6.0)


# ---------------------------------------------------------------------------------------------------------------------------
# NumPy emulation of the split products (csrc/gemm_common.h: split3, split2), fp32 accumulation in 16-deep steps
# ---------------------------------------------------------------------------------------------------------------------------
def bf16_rne(a):
    a = np.ascontiguousarray(a, np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32)


def split3(x):
    """x = h + m + l, three bf16, each the RNE of the remainder."""
    x = np.asarray(x, np.float32)
    h = bf16_rne(x)
    r = x - h
    m = bf16_rne(r)
    return h, m, bf16_rne(r - m)


def split2(x, bound=None):
    """x 2^k = hi + lo (fp16 each), k = 14 - e(bound); bound defaults to the tensor's maximum.  -> (hi, lo, k)."""
    x = np.asarray(x, np.float32)
    k = 14 - int(np.floor(np.log2(float(np.abs(x).max() if bound is None else bound))))
    y = np.ldexp(x, k).astype(np.float32)
    hi = y.astype(np.float16)
    lo = (y - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float32), lo.astype(np.float32), k


def _mfma_chain(pairs, step=16):
    """acc (fp32) += one `step`-deep product block per (A, B) pair, in order, per K step: the products are exact in fp32
    (bf16 x bf16, fp16 x fp16), a block's sum is formed exactly (float64) and the accumulator is rounded once per block."""
    M, Kd = pairs[0][0].shape
    N = pairs[0][1].shape[1]
    assert Kd % step == 0
    S = Kd // step
    parts = [np.matmul(A.astype(np.float64).reshape(M, S, step).transpose(1, 0, 2), B.astype(np.float64).reshape(S, step, N))
             for A, B in pairs]
    acc = np.zeros((M, N), np.float32)
    for s in range(S):
        for p in parts:
            acc = (acc.astype(np.float64) + p[s]).astype(np.float32)
    return acc


X3_PRODUCTS = ('lh', 'hl', 'mm', 'mh', 'hm', 'hh')        # a_l*b_h + a_h*b_l + a_m*b_m + a_m*b_h + a_h*b_m + a_h*b_h


def emulate_x3(A, B, drop=None):
    """'float32x3': the six bf16 products of the exact three-way split, fp32 accumulate; drop: one of X3_PRODUCTS left out."""
    a, b = dict(zip('hml', split3(A))), dict(zip('hml', split3(B)))
    return _mfma_chain([(a[p[0]], b[p[1]]) for p in X3_PRODUCTS if p != drop])


def emulate_x2(A, B, bound_factor=1.0):
    """'float32x2': a_lo*b_hi + a_hi*b_lo + a_hi*b_hi of the scaled fp16 pieces, fp32 accumulate, times 2^-(ka + kb)."""
    ah, al, ka = split2(A, bound_factor * np.abs(A).max())
    bh, bl, kb = split2(B, bound_factor * np.abs(B).max())
    return np.ldexp(_mfma_chain([(al, bh), (ah, bl), (ah, bh)]).astype(np.float64), -(ka + kb))


# ---------------------------------------------------------------------------------------------------------------------------
# every call of one chain run, from what each call was handed
# ---------------------------------------------------------------------------------------------------------------------------
# the rows of tests/test_gpu_abi_contract_chain.py::ROWS that both chain-accuracy modules run: the smallest that reach every kernel form
ACC_ROWS = ('c256_T256', 'c256_T384_dil_ge_T', 'c256_T1000_up8', 'c512_T256', 'c384_Cs320', 'c256_Cs128')
FWD, SKIP, BWD = 'vqvae_resblock_fwd_packed', 'vqvae_resstack_skip_fwd', 'vqvae_resblock_bwd_packed'
DILW, RESW, SKIPW = 'vqvae_resstack_dil_wgrad', 'vqvae_resstack_res_wgrad', 'vqvae_resstack_skip_wgrad'
GCOND, PULL = 'vqvae_resstack_gcond_bwd', 'pullback'


def chain_refs(h, dtype):
    """h: the handed values of one run -- blocks (the parameter dicts), dils, tab, Tl, P_all (B, nb Cd, Tl; bd inside),
    gy, gsig[i], and per block x_dec[i] (block i's input; x_dec[i + 1] its res), gates[i], z_dec[i], gh_dec[i], gx_dec[i].
    -> {(entry point, quantity, block or None): array in `dtype`}."""
    blocks, dils, tab, Tl = h['blocks'], h['dils'], h['tab'], h['Tl']
    nb = len(dils)
    Cd = blocks[0]['conv'][0].shape[0]
    out = {}
    for i, (p, dil) in enumerate(zip(blocks, dils)):
        last = i == nb - 1
        f = resblock_fwd_packed(h['x_dec'][i], p['conv'][0], h['P_all'][:, i * Cd:(i + 1) * Cd], tab, dil,
                                None if last else p['res'][0], None if last else p['res'][1], z_in=h['z_dec'][i], dtype=dtype)
        for k, v in f.items():
            out[(FWD, k, i)] = v
        g_res = None if last else h['gx_dec'][i + 1]
        b = resblock_bwd_packed(p['conv'][0], p['res'][0], p['skip'][0], h['gy'], g_res, h['gates'][i], dil, z=h['z_dec'][i],
                                gsig=h['gsig'][i], gh_in=h['gh_dec'][i], dtype=dtype)
        out[(BWD, 'gh', i)], out[(BWD, 'gx', i)] = b['gh'], b['gx']
        out[(DILW, 'gWd', i)], out[(DILW, 'gbd', i)] = dil_wgrad(h['x_dec'][i], h['gh_dec'][i], dil, p['conv'][0].shape[2], dtype)
        if not last:
            out[(RESW, 'gWr', i)], out[(RESW, 'gbr', i)] = lin_wgrad(h['z_dec'][i], g_res, dtype)
        out[(SKIPW, 'gWs', i)], out[(SKIPW, 'gbs', i)] = lin_wgrad(h['z_dec'][i], h['gy'], dtype)
        out[(PULL, 'gP', i)] = pullback(h['gh_dec'][i], tab, Tl, dtype)
    out[(SKIP, 'skip', None)] = skip_fwd([p['skip'][0] for p in blocks], [p['skip'][1] for p in blocks], h['z_dec'], dtype)
    out[(GCOND, 'gcond', None)] = gcond_bwd([p['condition_proj'][0] for p in blocks], h['gh_dec'], dtype)
    return out
