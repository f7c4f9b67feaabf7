"""Per-call references of everything a training step runs OUTSIDE the decoder chain and the vector quantiser: the generic
conv in its three directions, the fused latent kernels (conv stack, stride-2 stage backward), the one-hot embed conv, the two
losses, the upsample adjoint and the embed-broadcast gradient.  Each is that call's mathematical function over the values the
call was handed, evaluated in `dtype` = float64 (the truth) or float32 (NumPy's own fp32 arithmetic: the yardstick `e32` of
tests/test_gpu_call_accuracy.py), operands cast first and every contraction np.matmul per tap -- the style, the two metrics
and the bar of tests/chain_accuracy_ref.py, which this module imports and does not copy.

Nothing here restates a kernel's arithmetic, with two exceptions that are what they are for:
  expected_forms   the predicates of prepare_gemm, select_gemm, plan_ksplit, phase_split_ok, plan_wgrad and select_wgrad restated,
                   so that vqvae_conv1d_forms is held against a second statement (tests/test_host_call_accuracy.py);
  two_stage_sum    the stated summation order of the two-stage scalar reduce (csrc/misc.hip) in NumPy float32, and
                   scalar_model, the error model a device scalar is judged against instead of e32."""
import numpy as np

from chain_accuracy_ref import bar, emulate_x2, emulate_x3, metrics, seq_error      # noqa: F401  (re-exported: one bar for both suites)


def _c(a, dtype):
    return np.ascontiguousarray(np.asarray(a).astype(dtype))


def conv_out_len(Tin, K, stride, pad, dil):
    return (Tin + 2 * pad - dil * (K - 1) - 1) // stride + 1


# ---------------------------------------------------------------------------------------------------------------------------
# generic conv: y[b, o, t] = bias[o] + sum_{c, j} W[o, c, j] x[b, c, t stride + j dil - pad], t < Tout (the crop)
# ---------------------------------------------------------------------------------------------------------------------------
def _taps(Tin, Tout, K, stride, pad, dil):
    """Per tap j: (the outputs t0 .. t1 whose input position lies inside the row, the first such input position)."""
    out = []
    for j in range(K):
        off = j * dil - pad
        t0 = max(0, -(off // stride)) if off < 0 else 0               # smallest t with t stride + off >= 0
        t1 = min(Tout, (Tin - 1 - off) // stride + 1) if Tin - 1 - off >= 0 else 0
        out.append((j, t0, max(t1, t0), t0 * stride + off))
    return out


def conv_fwd(x, W, b, stride, pad, dil, Tout=None, relu=False, dtype=np.float64):
    x, W = _c(x, dtype), _c(W, dtype)
    B, Cin, Tin = x.shape
    Cout, _, K = W.shape
    Tout = conv_out_len(Tin, K, stride, pad, dil) if Tout is None else Tout
    y = np.zeros((B, Cout, Tout), dtype)
    for j, t0, t1, p0 in _taps(Tin, Tout, K, stride, pad, dil):
        if t1 > t0:
            xs = np.ascontiguousarray(x[:, :, p0:p0 + (t1 - t0 - 1) * stride + 1:stride])
            y[:, :, t0:t1] += np.matmul(np.ascontiguousarray(W[:, :, j]), xs)
    if b is not None:
        y = y + _c(b, dtype)[None, :, None]
    return np.maximum(y, dtype(0)) if relu else y


def conv_bwd_data(W, gy, stride, pad, dil, Tin, x_relu=None, addend=None, dtype=np.float64):
    """gx (B, Cin, Tin) of the cropped conv under gy (B, Cout, Tout); x_relu: vqvae_conv1d_bwd_data_relu's mask (gx where the
    conv's input, the output of a ReLU, is positive); addend: accumulate = 1 (added in `dtype`)."""
    W, gy = _c(W, dtype), _c(gy, dtype)
    B, Cout, Tout = gy.shape
    _, Cin, K = W.shape
    gx = np.zeros((B, Cin, Tin), dtype)
    for j, t0, t1, p0 in _taps(Tin, Tout, K, stride, pad, dil):
        if t1 > t0:
            gx[:, :, p0:p0 + (t1 - t0 - 1) * stride + 1:stride] += np.matmul(np.ascontiguousarray(W[:, :, j].T),
                                                                             np.ascontiguousarray(gy[:, :, t0:t1]))
    if x_relu is not None:
        gx = gx * (np.asarray(x_relu) > 0)
    return gx if addend is None else gx + _c(addend, dtype)


def conv_bwd_weight(x, gy, K, stride, pad, dil, addend_W=None, addend_b=None, dtype=np.float64):
    """-> gW (Cout, Cin, K), gb (Cout,)."""
    x, gy = _c(x, dtype), _c(gy, dtype)
    B, Cin, Tin = x.shape
    _, Cout, Tout = gy.shape
    gW = np.zeros((Cout, Cin, K), dtype)
    for j, t0, t1, p0 in _taps(Tin, Tout, K, stride, pad, dil):
        if t1 > t0:
            xs = np.ascontiguousarray(np.swapaxes(x[:, :, p0:p0 + (t1 - t0 - 1) * stride + 1:stride], 1, 2))
            gW[:, :, j] = np.matmul(np.ascontiguousarray(gy[:, :, t0:t1]), xs).sum(axis=0, dtype=dtype)
    gb = gy.sum(axis=(0, 2), dtype=dtype)
    if addend_W is not None:
        gW = gW + _c(addend_W, dtype)
    if addend_b is not None:
        gb = gb + _c(addend_b, dtype)
    return gW, gb


# ---------------------------------------------------------------------------------------------------------------------------
# the fused latent kernels
# ---------------------------------------------------------------------------------------------------------------------------
def convstack_layer(h_prev, W, b, dil, dtype=np.float64):
    """h_l = relu(conv(h_{l-1}; W_l (C, C, 3), pad = dil, dilate = dil) + b_l) from the HANDED h_{l-1}."""
    return conv_fwd(h_prev, W, b, 1, dil, dil, relu=True, dtype=dtype)


def convstack_bwd(x, Ws, hs, dils, gy, dtype=np.float64):
    """The whole backward from the handed h's (hs[l] = h_{l+1}) -> gx, [gW_l], [gb_l]."""
    L = len(Ws)
    g = _c(gy, dtype)
    gWs, gbs = [None] * L, [None] * L
    for l in range(L - 1, -1, -1):
        g = g * (np.asarray(hs[l]) > 0)
        inp = x if l == 0 else hs[l - 1]
        gWs[l], gbs[l] = conv_bwd_weight(inp, g, 3, 1, dils[l], dils[l], dtype=dtype)
        g = conv_bwd_data(Ws[l], g, 1, dils[l], dils[l], g.shape[2], dtype=dtype)
    return g, gWs, gbs


def conv_s2_bwd(x, W, gy, mask, dtype=np.float64):
    """The backward of one encoder stage, Convolution2D(C, C, (4, 1), stride 2, pad 1): gx (times x > 0 under mask), gW, gb."""
    gx = conv_bwd_data(W, gy, 2, 1, 1, np.asarray(x).shape[2], x_relu=x if mask else None, dtype=dtype)
    gW, gb = conv_bwd_weight(x, gy, 4, 2, 1, 1, dtype=dtype)
    return gx, gW, gb


# ---------------------------------------------------------------------------------------------------------------------------
# the one-hot embed conv: the causal conv (pad K - 1, cropped to T) over x (B, q, T)
# ---------------------------------------------------------------------------------------------------------------------------
def embed_fwd(x, W, b, dtype=np.float64):
    K = np.asarray(W).shape[2]
    return conv_fwd(x, W, b, 1, K - 1, 1, Tout=np.asarray(x).shape[2], dtype=dtype)


def embed_wgrad(x, gy, K, dtype=np.float64):
    return conv_bwd_weight(x, gy, K, 1, K - 1, 1, dtype=dtype)


# ---------------------------------------------------------------------------------------------------------------------------
# losses
# ---------------------------------------------------------------------------------------------------------------------------
def xent(y, t, gloss=1.0, lse_in=None, dtype=np.float64):
    """-> dict(lse (B, T), loss, gy (B, q, T)); gy from the HANDED lse when given (vqvae_softmax_xent_bwd reads the stored one)."""
    y = _c(y, dtype)
    B, q, T = y.shape
    ti = np.asarray(t)[:, None, :].astype(np.int64)
    m = y.max(axis=1, keepdims=True)
    lse = np.log(np.exp(y - m).sum(axis=1, keepdims=True, dtype=dtype)) + m
    picked = np.take_along_axis(y, ti, 1)
    loss = (lse - picked).sum(dtype=dtype) / dtype(B * T)
    l_in = lse if lse_in is None else _c(lse_in, dtype)[:, None, :]
    p = np.exp(y - l_in)
    np.put_along_axis(p, ti, np.take_along_axis(p, ti, 1) - dtype(1), 1)
    return dict(lse=lse[:, 0, :], loss=loss, gy=p * (dtype(gloss) / dtype(B * T)))


def mol(y, t, gloss=1.0, dtype=np.float64):
    """The mixture-of-logistics loss and its gradient: the oracle's functions on `dtype` operands (they ARE the plain NumPy
    statement of modules.py:169-230 and run in the dtype they are handed)."""
    import vqvae_oracle as O
    y, t = _c(y, dtype), _c(t, dtype)
    return dict(loss=O.mol_loss_fwd(y, t), gy=O.mol_loss_bwd(y, t, gloss=gloss))


# ---------------------------------------------------------------------------------------------------------------------------
# resize adjoint, speaker-embedding gradient
# ---------------------------------------------------------------------------------------------------------------------------
def upsample_bwd(gy, tab, Tin, dtype=np.float64):
    """The adjoint of y[i] = w0[i] x[v0[i]] + w1[i] x[v1[i]] over the float32 tables the kernel is handed."""
    gy = _c(gy, dtype)
    Tout = gy.shape[-1]
    U = np.zeros((Tout, Tin), dtype)
    i = np.arange(Tout)
    np.add.at(U, (i, np.asarray(tab['v0'])), _c(tab['w0'], dtype))
    np.add.at(U, (i, np.asarray(tab['v1'])), _c(tab['w1'], dtype))
    return np.matmul(gy, U)


def embed_broadcast_bwd(gy, ids, n_id, addend=None, dtype=np.float64):
    """gE (n_id, G) = scatter over ids of sum_t gy[b, :, t]."""
    rows = _c(gy, dtype).sum(axis=2, dtype=dtype)
    gE = np.zeros((n_id, rows.shape[1]), dtype)
    np.add.at(gE, np.asarray(ids), rows)
    return gE if addend is None else gE + _c(addend, dtype)


# ---------------------------------------------------------------------------------------------------------------------------
# scalars: the two-stage reduce of csrc/misc.hip in its stated order, and the model a device scalar is judged against
# ---------------------------------------------------------------------------------------------------------------------------
def _block_sum_256(v):
    """block_sum_256: the 64-lane xor butterfly (offsets 32 .. 1) per wave, then (((w0 + w1) + w2) + w3); v (256,) float32."""
    v = np.asarray(v, np.float32).reshape(4, 64).copy()
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = (v + v[:, lane ^ off]).astype(np.float32)
    w = v[:, 0]
    return np.float32(np.float32(np.float32(w[0] + w[1]) + w[2]) + w[3])


def _strided_chains(terms, nthreads):
    """acc[i] = ((0 + terms[i]) + terms[i + nthreads]) + ... in float32: every thread's serial chain of a grid-stride loop."""
    terms = np.asarray(terms, np.float32)
    n = terms.size
    rounds = -(-n // nthreads)
    padded = np.zeros(rounds * nthreads, np.float32)
    padded[:n] = terms
    acc = np.zeros(nthreads, np.float32)
    for r in padded.reshape(rounds, nthreads):
        acc = (acc + r).astype(np.float32)
    return acc


def grid_for(n, block=256, cap=1024):
    return int(min(max(-(-n // block), 1), cap))


def two_stage_sum(terms, scale, leave_out=None):
    """sum_stage1 over grid_for(n) workgroups of 256 (grid-stride chains, block_sum_256), sum_stage2 over the partials, times
    scale; leave_out: the index of one workgroup whose partial is dropped (the defect the model has to see)."""
    terms = np.asarray(terms, np.float32).reshape(-1)
    nwg = grid_for(terms.size)
    acc = _strided_chains(terms, nwg * 256).reshape(nwg, 256)
    partial = np.array([_block_sum_256(a) for a in acc], np.float32)
    if leave_out is not None:
        partial[leave_out] = 0
    return np.float32(_block_sum_256(_strided_chains(partial, 256)) * np.float32(scale))


def scalar_model(nterms, lanes=256, cap=1024):
    """The error bound of a two-stage sum of `nterms` float32 terms, in units of sum |term|.  Stage 1: grid_for(nterms, lanes)
    workgroups in which `lanes` threads each keep a serial chain of ceil(nterms / (workgroups lanes)) terms (256 for vqvae_sum,
    vqvae_sqdiff_mean and the mixture loss; 64 for xent_fwd_kernel, whose first wave alone carries terms), then
    block_sum_256's six butterfly levels and the three adds of the four waves; stage 2 (sum_stage2): chains of
    ceil(workgroups / 256) partials, the same tree, one multiplication by the scale.  seq_error(chain) is the rms relative error
    of a chain; a tree level rounds a partial sum no larger than sum |term| once, 2^-24 each, added linearly (a bound, not an
    rms).  Times the 3 of `bar`."""
    nwg = grid_for(nterms, lanes, cap)
    chain1 = -(-nterms // (nwg * lanes))
    chain2 = -(-nwg // 256)
    return 3.0 * (seq_error(chain1) + seq_error(chain2) + (2 * (6 + 3) + 1) * 2.0 ** -24)


# ---------------------------------------------------------------------------------------------------------------------------
# the dispatch of the generic conv, restated (csrc/conv_api.hip, conv_gemm_x3.hip, wgrad.hip)
# ---------------------------------------------------------------------------------------------------------------------------
FAMILY, ROWS256, WIDE, NP_MASK, NP_SHIFT = 0x003, 0x004, 0x008, 0x030, 4
TAP2, LEAN, HALVED, SPLIT, STRIDED, PHASES = 0x040, 0x080, 0x100, 0x200, 0x400, 0x800
FORM_BITS = dict(FAMILY=FAMILY, ROWS256=ROWS256, WIDE=WIDE, NP=NP_MASK, NP_SHIFT=NP_SHIFT, TAP2=TAP2, LEAN=LEAN, HALVED=HALVED,
                 SPLIT=SPLIT, STRIDED=STRIDED, PHASES=PHASES)
GEMM_LIN128, GEMM_TILED, GEMM_FP32 = 0, 1, 2
WGRAD_W3, WGRAD_W2, WGRAD_GENERIC = 0, 1, 2
MODES = {'float32': 0, 'bfloat16': 1, 'float32x3': 2, 'float32x2': 3}
BK, BN, WBK, MAXTAPS, MAXSEG = 16, 128, 32, 4, 24


def _cdiv(a, b):
    return -(-a // b)


def _pad16(v):
    return _cdiv(v, 16) * 16


def _pad128(v):
    return _cdiv(v, 128) * 128


def plan_ksplit(M, Tout, B, nk):
    if M % 256 == 0:
        return 1
    tiles = _cdiv(M, 128) * _cdiv(Tout, BN) * B
    if tiles > 128 or nk < 32:
        return 1
    s = min(512 // tiles, nk // 8, 32)
    return 1 if s < 2 else s


def plan_wgrad(M, B, Tout, Cin, K):
    """plan_wgrad for K segments of Cin channels (never `wide`: the generic conv's plans) -> (splits, 32-position steps per split)."""
    tiles = _cdiv(M, 128) * K * _cdiv(Cin, BN)
    total = B * _cdiv(Tout, WBK)
    maxs = min(max(total // 4, 1), 256)
    slots = 512
    want, best = 1, -1.0
    for w in range(1, maxs + 1):
        sps = _cdiv(total, w)
        blocks = tiles * _cdiv(total, sps)
        eff = blocks / float(_cdiv(blocks, slots) * slots)
        if eff > best + 1e-9:
            best, want = eff, w
        if eff >= 0.92 and blocks >= slots:
            want = w
            break
    sps = _cdiv(total, want)
    return _cdiv(total, sps), sps


def plan_wgrad_nsplit(M, B, Tout, Cin, K):
    return plan_wgrad(M, B, Tout, Cin, K)[0]


def desc_of(row):
    """(B, Cin, Tin, Cout, K, stride, pad, dil, crop) -> (B, Cin, Tin, Cout, Tout, K, stride, pad, dil)."""
    B, Cin, Tin, Cout, K, stride, pad, dil, crop = row
    Tout = conv_out_len(Tin, K, stride, pad, dil) if crop is None else crop
    return (B, Cin, Tin, Cout, Tout, K, stride, pad, dil)


def expected_forms(desc, which, mode, min_gflop=0.0, relu=0):
    """vqvae_conv1d_forms(desc, which) under matmul dtype `mode` (a name or 0 .. 3) and the f32x2 threshold min_gflop."""
    B, Cin, Tin, Cout, Tout, K, stride, pad, dil = desc
    mode = MODES.get(mode, mode)
    if which not in (0, 1, 2) or min(B, Cin, Cout, Tin, Tout) <= 0 or not 1 <= K <= MAXTAPS or stride < 1 or dil < 1 or pad < 0:
        return -1
    if Tout > conv_out_len(Tin, K, stride, pad, dil):
        return -1
    f16 = mode == 3 and 2.0 * B * Tout * float(Cout) * Cin * K >= min_gflop * 1e9
    if which == 2:
        phases = stride == 2 and dil == 1 and K <= MAXSEG and Tout % 4 == 0 and Tin >= 8
        f16 = f16 and not phases and stride == 1
        tmul = 1 if phases else stride
        x_bstride = Cin * (((Tin + 1) // 2 + 3) & ~3) if phases else Cin * Tin
        fast = Tout % 4 == 0 and (Cout * Tout) % 4 == 0 and tmul == 1
        fast = fast and (mode == 0 or (B * Cout * Tout * 4 < 2 ** 31 and B * x_bstride * 4 < 2 ** 31))
        gm = (3 if f16 and fast else 2) if mode == 3 else mode
        if fast:
            family, np_ = (WGRAD_W2, 0) if gm == 0 else (WGRAD_W3, {3: 2, 2: 3, 1: 1}[gm])
        else:
            family, np_ = WGRAD_GENERIC, 1 if gm == 1 else 0
        r = family | np_ << NP_SHIFT
        if family != WGRAD_GENERIC and Cout % 256 == 0:
            r |= ROWS256
        if phases:
            r |= PHASES
        if plan_wgrad_nsplit(Cout, B, Tout, Cin, K) > 1:
            r |= SPLIT
        return r | (STRIDED if tmul != 1 else 0)
    gm = (3 if f16 else 2) if mode == 3 else mode
    if which == 0:
        M, To, cin, xT, tmul, tdiv, toffs = Cout, Tout, Cin, Tin, stride, 1, [j * dil - pad for j in range(K)]
    else:
        M, To, cin, xT, tmul, tdiv, toffs, relu = Cin, Tin, Cout, Tout, 1, stride, [pad - j * dil for j in range(K)], 0
    if gm != 0 and cin * xT * 4 >= 2 ** 31:
        return -1
    big = M % 256 == 0
    ksplit = 1 if big else plan_ksplit(M, To, B, K * _cdiv(cin, BK))
    nseg, halved = K, False
    if big and gm in (2, 3) and nseg == 1 and ksplit == 1 and cin >= 64 and cin % 32 == 0 and not (M == 256 and cin == 128) \
            and tmul == 1 and tdiv == 1:
        nseg, cin, halved = 2, cin // 2, True
    np_ = {0: 0, 1: 1, 2: 3, 3: 2}[gm]
    vec = tmul == 1 and tdiv == 1 and xT % 4 == 0 and (cin * xT) % 4 == 0
    if (gm != 0 and nseg == 1 and M == 256 and cin == 128 and not relu and tmul == 1 and tdiv == 1 and toffs[0] == 0 and xT == To
            and To % 64 == 0 and vec and _pad128(M) >= 256 and ksplit == 1):
        return GEMM_LIN128 | np_ << NP_SHIFT
    rp = _pad16(cin) * 3 // 2 if mode >= 2 else _pad16(cin)
    tap2 = gm != 0 and nseg == 2 and ksplit == 1 and cin % BK == 0 and (halved or rp * _pad128(M) * 4 < 2 ** 30)
    lean = tap2 and big
    wide = gm != 0 and big and not lean and _cdiv(M, 256) * _cdiv(To, 2 * BN) * B >= 256
    r = (GEMM_FP32 if gm == 0 else GEMM_TILED) | np_ << NP_SHIFT
    for bit, on in ((ROWS256, big), (WIDE, wide), (TAP2, tap2), (LEAN, lean), (HALVED, halved), (SPLIT, ksplit > 1),
                    (STRIDED, tmul != 1 or tdiv != 1)):
        if on:
            r |= bit
    return r


def describe(word):
    """A form word in words, for assertion messages."""
    if word < 0:
        return 'refused'
    names = [n for n, b in (('ROWS256', ROWS256), ('WIDE', WIDE), ('TAP2', TAP2), ('LEAN', LEAN), ('HALVED', HALVED), ('SPLIT', SPLIT),
                            ('STRIDED', STRIDED), ('PHASES', PHASES)) if word & b]
    return 'family %d NP %d %s' % (word & FAMILY, (word & NP_MASK) >> NP_SHIFT, ' '.join(names))


# ---------------------------------------------------------------------------------------------------------------------------
# the rows of tests/test_gpu_call_accuracy.py (both suites read them here)
# ---------------------------------------------------------------------------------------------------------------------------
# name, (B, Cin, Tin, Cout, K, stride, pad, dil, crop), options: relu (the forward's ReLU and vqvae_conv1d_bwd_data_relu are judged
# too), acc (accumulate = 1 of the three gradients is judged too), only (the directions judged; default all three)
CONV_ROWS = [
    ('enc1', (2, 1, 512, 64, 4, 2, 1, 1, 252), {}),            # cropped below the natural 256 (a multiple of 4: the phase split)
    ('enc_odd', (2, 64, 255, 64, 4, 2, 1, 1, None), {}),
    ('ragged', (2, 40, 77, 50, 3, 2, 2, 3, None), dict(acc=True)),
    ('splitk', (2, 1280, 120, 192, 1, 1, 0, 1, None), {}),
    ('splitk_t', (2, 192, 120, 1280, 1, 1, 0, 1, None), {}),
    ('cond_proj', (1, 192, 130, 256, 1, 1, 0, 1, None), {}),
    ('head', (2, 256, 256, 256, 1, 1, 0, 1, None), dict(relu=True)),
    ('lin128', (3, 128, 192, 256, 1, 1, 0, 1, None), {}),
    ('lin128_T200', (3, 128, 200, 256, 1, 1, 0, 1, None), {}),
    ('two_tap', (1, 256, 384, 256, 2, 1, 3, 3, 384), dict(acc=True)),
    ('three_tap', (1, 32, 300, 256, 3, 1, 2, 2, None), {}),
    ('wide', (4, 32, 16384, 256, 1, 1, 0, 1, None), dict(only=(0, 2))),
]
CONV_BY_NAME = dict((r[0], r) for r in CONV_ROWS)
ACC_MODES = ('float32x2', 'float32x3', 'float32')


# what each conv row is in the suite for: (which, mode or None for every mode) -> bits that must be set, bits that must be
# absent, family.  The GPU test asserts the same through the library before it runs a row.
ROW_FORMS = {
    'enc1': [(0, None, STRIDED, ROWS256, None), (1, None, STRIDED, ROWS256, None), (2, None, PHASES, STRIDED, None)],
    'enc_odd': [(0, None, STRIDED, ROWS256, None), (2, None, STRIDED, PHASES, WGRAD_GENERIC)],
    'ragged': [(0, None, STRIDED, ROWS256 | SPLIT, None), (2, None, STRIDED, PHASES, WGRAD_GENERIC)],
    'splitk': [(0, None, SPLIT, ROWS256, None), (2, 'float32x3', 0, ROWS256, WGRAD_W3), (2, 'float32x2', 0, ROWS256, WGRAD_W3),
               (2, 'float32', 0, ROWS256, WGRAD_W2)],
    'splitk_t': [(1, None, SPLIT, ROWS256, None)],
    'cond_proj': [(0, 'float32x3', ROWS256 | HALVED | TAP2 | LEAN, 0, GEMM_TILED),
                  (0, 'float32x2', ROWS256 | HALVED | TAP2 | LEAN, 0, GEMM_TILED),
                  (0, 'float32', ROWS256, HALVED, GEMM_FP32), (1, None, 0, ROWS256 | SPLIT, None),
                  (2, None, 0, STRIDED, WGRAD_GENERIC)],
    'head': [(w, m, ROWS256 | HALVED | TAP2 | LEAN, 0, GEMM_TILED) for w in (0, 1) for m in ('float32x3', 'float32x2')],
    'lin128': [(0, 'float32x3', 0, 0, GEMM_LIN128), (0, 'float32x2', 0, 0, GEMM_LIN128), (0, 'float32', ROWS256, 0, GEMM_FP32)],
    'lin128_T200': [(0, 'float32x3', ROWS256, HALVED | TAP2 | WIDE, GEMM_TILED),
                    (0, 'float32x2', ROWS256, HALVED | TAP2 | WIDE, GEMM_TILED)],
    'two_tap': [(w, m, ROWS256 | TAP2 | LEAN, HALVED, GEMM_TILED) for w in (0, 1) for m in ('float32x3', 'float32x2')],
    'three_tap': [(0, 'float32x3', ROWS256, TAP2 | WIDE | HALVED, GEMM_TILED),
                  (0, 'float32x2', ROWS256, TAP2 | WIDE | HALVED, GEMM_TILED)],
    'wide': [(0, 'float32x3', ROWS256 | WIDE, TAP2, GEMM_TILED), (0, 'float32x2', ROWS256 | WIDE, TAP2, GEMM_TILED),
             (2, 'float32x3', ROWS256 | SPLIT, PHASES, WGRAD_W3), (2, 'float32', ROWS256 | SPLIT, 0, WGRAD_W2)],
}


def check_row_forms(name, mode, forms_of):
    """forms_of(which) -> word; asserts what ROW_FORMS says of this row in this mode."""
    for which, m, on, off, family in ROW_FORMS[name]:
        if m in (None, mode):
            w = forms_of(which)
            assert w >= 0 and w & on == on and w & off == 0 and (family is None or w & FAMILY == family), \
                '%s %s which %d runs as "%s"' % (name, mode, which, describe(w))


def conv_inputs(name):
    """The handed values of a conv row: x, W, b, gy, and the addends of accumulate = 1."""
    import zlib
    _, row, opt = CONV_BY_NAME[name]
    B, Cin, Tin, Cout, Tout, K, stride, pad, dil = desc_of(row)
    rs = np.random.RandomState(zlib.crc32(repr(('call_acc', name)).encode()))
    f = lambda a: np.ascontiguousarray(a, np.float32)
    out = dict(x=f(rs.standard_normal((B, Cin, Tin))), W=f(rs.standard_normal((Cout, Cin, K)) / np.sqrt(Cin * K)),
               b=f(rs.standard_normal(Cout)), gy=f(rs.standard_normal((B, Cout, Tout))))
    if opt.get('acc'):
        out.update(ax=f(rs.standard_normal((B, Cin, Tin))), aW=f(rs.standard_normal((Cout, Cin, K))), ab=f(rs.standard_normal(Cout)))
    return out


def conv_refs(name, inp, dtype):
    """{quantity: array in dtype} of a conv row over its handed inputs: y, gx, gW, gb [, y_relu, gx_relu] [, gx+, gW+, gb+]."""
    _, row, opt = CONV_BY_NAME[name]
    B, Cin, Tin, Cout, Tout, K, stride, pad, dil = desc_of(row)
    only = opt.get('only', (0, 1, 2))
    out = {}
    if 0 in only:
        out['y'] = conv_fwd(inp['x'], inp['W'], inp['b'], stride, pad, dil, Tout, dtype=dtype)
        if opt.get('relu'):
            out['y_relu'] = conv_fwd(inp['x'], inp['W'], inp['b'], stride, pad, dil, Tout, relu=True, dtype=dtype)
    if 1 in only:
        out['gx'] = conv_bwd_data(inp['W'], inp['gy'], stride, pad, dil, Tin, dtype=dtype)
        if opt.get('relu'):
            out['gx_relu'] = conv_bwd_data(inp['W'], inp['gy'], stride, pad, dil, Tin, x_relu=np.maximum(inp['x'], 0), dtype=dtype)
        if opt.get('acc'):
            out['gx+'] = conv_bwd_data(inp['W'], inp['gy'], stride, pad, dil, Tin, addend=inp['ax'], dtype=dtype)
    if 2 in only:
        out['gW'], out['gb'] = conv_bwd_weight(inp['x'], inp['gy'], K, stride, pad, dil, dtype=dtype)
        if opt.get('acc'):
            out['gW+'], out['gb+'] = conv_bwd_weight(inp['x'], inp['gy'], K, stride, pad, dil, inp['aW'], inp['ab'], dtype=dtype)
    return out


def _rs(*key):
    import zlib
    return np.random.RandomState(zlib.crc32(repr(('call_acc',) + key).encode()))


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


# vqvae_convstack_fwd / _bwd (B, C, T, dils) and vqvae_conv_s2_bwd (B, Tin, mask; C = 64)
STACK_ROWS = [(3, 64, 120, (1, 2, 4, 8, 16)), (2, 32, 8, (1, 2, 4, 8, 16)), (1, 64, 128, (16, 1)), (4, 32, 37, (3,)),
              (1, 64, 5, (1, 2, 4, 8, 16, 1, 2, 4))]
S2_ROWS = [(1, 2, 0), (3, 127, 1), (2, 130, 1), (2, 256, 1), (1, 961, 0)]
# vqvae_embed_onehot_fwd / _wgrad (B, Cout, q, K, T) x the input kinds
ONEHOT_ROWS = [(2, 33, 50, 2, 64), (1, 5, 256, 2, 68), (3, 4, 7, 3, 10)]
ONEHOT_KINDS = ('onehot', 'dense', 'one_class')
# soft-max cross-entropy (q, B, T) and mixture of logistics (nm, B, T)
XENT_ROWS = [(256, 3, 63), (256, 2, 128), (50, 3, 21), (3, 1, 13), (16, 2, 40000)]
MOL_ROWS = [(10, 3, 63), (16, 1, 257), (10, 2, 1000), (2, 1, 300000)]
SCALAR_N = [1, 255, 257, 2 ** 20 + 3]
XENT_GLOSS = 0.5


def stack_inputs(row):
    B, C, T, dils = row
    rs = _rs('stack', row)
    return dict(x=_f32(rs.standard_normal((B, C, T))), gy=_f32(rs.standard_normal((B, C, T))),
                W=[_f32(rs.standard_normal((C, C, 3)) / np.sqrt(3 * C) * 1.4) for _ in dils], b=[_f32(0.3 * rs.standard_normal(C)) for _ in dils])


def s2_inputs(row, C=64):
    B, Tin, mask = row
    rs = _rs('s2', row)
    Tout = conv_out_len(Tin, 4, 2, 1, 1)
    x = _f32(rs.standard_normal((B, C, Tin)))
    return dict(x=np.maximum(x, 0) if mask else x, W=_f32(rs.standard_normal((C, C, 4)) / np.sqrt(4 * C)),
                gy=_f32(rs.standard_normal((B, C, Tout))), Tout=Tout)


def onehot_inputs(row, kind):
    B, Cout, q, K, T = row
    rs = _rs('onehot', row, kind)
    idx = rs.randint(0, q, (B, T)).astype(np.int32)
    if kind == 'one_class':
        idx[:] = q // 2                                       # every position in one class: the longest data-dependent sum
    x = _f32(np.identity(q, dtype=np.float32)[idx].transpose(0, 2, 1))
    if kind == 'dense':
        x = _f32(x + 0.25 * rs.standard_normal(x.shape))      # no column is one-hot: the dense conv
    return dict(x=x, idx=idx, W=_f32(rs.standard_normal((Cout, q, K)) / np.sqrt(K)), b=_f32(rs.standard_normal(Cout)),
                gy=_f32(rs.standard_normal((B, Cout, T))))


def xent_inputs(row):
    """3 N(0, 1) logits with the +-80 row and the equal-logits row of test_softmax_xent_contract."""
    q, B, T = row
    rs = _rs('xent', row)
    y = _f32(3 * rs.standard_normal((B, q, T)))
    t = rs.randint(0, q, (B, T)).astype(np.int32)
    y[0, :, 0] = 1.25
    t[0, 0] = q - 1
    y[B - 1, :, T - 1] = -80.0
    y[B - 1, q - 1, T - 1] = 80.0
    t[B - 1, T - 1] = 0
    y[0, 0, 1] = 80.0
    t[0, 1] = 0
    return dict(y=y, t=t)


def mol_inputs(row):
    """targets U(-0.99, 0.99), log-scales U(0.5, 3.5), means 127.5 t + exp(log-scale) N(0, 1): every mixture component within a
    few scales of the target, where cdf_plus - cdf_min does not cancel to nothing."""
    nm, B, T = row
    rs = _rs('mol', row)
    t = _f32(rs.uniform(-0.99, 0.99, (B, 1, T)))
    y = _f32(rs.standard_normal((B, 3 * nm, T)))
    ls = _f32(rs.uniform(0.5, 3.5, (B, nm, T)))
    y[:, 2 * nm:] = ls
    y[:, nm:2 * nm] = _f32(127.5 * t + np.exp(ls) * rs.standard_normal((B, nm, T)))
    return dict(y=y, t=t)


def mol_terms(y, t, dtype=np.float64):
    """The per-position negative log-likelihoods whose mean is the loss."""
    import vqvae_oracle as O
    return -O._mol_terms(_c(y, dtype), _c(t, dtype), 256, -40.0)['lse'][:, 0]


def scalar_inputs(n):
    rs = _rs('scalar', n)
    return dict(x=_f32(rs.standard_normal(n)), a=_f32(rs.standard_normal(n)), b=_f32(rs.standard_normal(n)))
