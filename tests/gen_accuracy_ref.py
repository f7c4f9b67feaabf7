"""References of the generation step forms (tests/test_host_gen_accuracy.py, tests/test_gpu_gen_accuracy.py).  NumPy only.

`step` is one generation step as a function of the values the call is handed, over the DEVICE's state layout (rings of
`dilation` slots, slot t % dilation the old tap; the two-sample embed queue as x_prev / x_cur): it restates
oracle/vqvae_oracle.wavenet_generate_step, calls the oracle's own conv1d_fwd on the two taps a block reads, and returns
every quantity vqvae_wavenet_gen_step leaves in caller memory.  In `dtype` = float64 it is the truth, in float32 NumPy's
own fp32 arithmetic, the yardstick e32 of chain_accuracy_ref.bar.  `run` is the teacher-forced run of the oracle.

ROWS is the table of shapes of both test files; every input is seeded and made here (`inputs`), nothing is stored.
Every decoder bias is 0.1 N(0, 1) (`bias_tweak`, the arithmetic of test_gpu_generate._random_biases).

`emulate` runs a row in float32 in the two device orders whose rounding differs most from NumPy's:
  'lockstep'    csrc/gen_lockstep_body.h, ls_gemm_body: K in 16-wide chunks, chunk c on wave c % 8 (the condition's chunks
                follow the conv's), each wave one fp32 accumulator fed k-ordered inside an MFMA (v_mfma_f32_16x16x4f32 j takes
                k = 4 g + j of the chunk from lane group g), the eight partials summed in wave order, biases after.
  'persistent'  csrc/generate.hip, gen_mega_kernel: element k = lane + 64 i of a vector sits in lane k % 64, a lane
                accumulates its i in order, mega_wave_sum adds the 64 lanes (xor 1, xor 2, mirror of 8, mirror of 16, then
                (r0 + r1) + (r2 + r3)); the helper wave's old tap + condition + (conv_b + cond_b); the composite
                M_l = Wc1_{l+1} Wr_l and cb = Wc1_{l+1} br_l accumulated in float64 and rounded once; the shadow term
                Wc1_{l+1} x_l; h = ((M z + u) + cb) + pre; mega_gate = (1 - 2 / (1 + exp(2 h0))) / (1 + exp(-h1)); the last
                block's residual output is not formed.
The MFMA's multiply-add is emulated as the float64 sum of the exact product, rounded to float32; the vector ALU code is
built with -ffp-contract=off, so there a product is rounded before it is added; exp and the division are NumPy's.
Mutations (value only): 'partial_half' -- wave 3's partial of every dilated conv rounded to half precision before the LDS
sum (lockstep order); 'cb_half' -- cb rounded to half precision (persistent order)."""
import numpy as np

import helpers as H
import vqvae_oracle as O

F32 = np.float32
T_RUN = 12                                     # > 2 x the largest dilation (4; the mixture rows' 8 is outrun once): every old tap is live
T_STEP = 5                                     # t % dilation = 0, 1, 1 for the dilations 1, 2, 4


# ---------------------------------------------------------------------------------------------------------------------------
# the rows
# ---------------------------------------------------------------------------------------------------------------------------
def _shape(residual, dilated, skip, out_dim, cond, **kw):
    cfg = dict(H.SMALL, residual=residual, dilated=dilated, skip=skip, out_dim=out_dim, local_dim=cond - 32, global_dim=32)
    cfg.update(kw)
    return cfg


_SMALL = _shape(64, 64, 64, 256, 64)
_ODD = _shape(72, 88, 56, 250, 63)
_K320 = _shape(320, 320, 288, 256, 200)

# name -> (kind 'step' | 'run', form, cfg, ns, mixture of logistics, seed)
ROWS = [
    ('mv_small', 'step', 'mv', _SMALL, (1, 4), False, 500),
    ('mv_odd', 'step', 'mv', _ODD, (3,), False, 502),
    ('mv_k320', 'step', 'mv', _K320, (2,), False, 504),
    ('mv_mol', 'step', 'mv', dict(H.MOL_SHALLOW), (2,), True, 506),
    ('ls_small', 'step', 'ls', _SMALL, (5, 16, 37), False, 508),
    ('ls_odd', 'step', 'ls', _ODD, (21,), False, 510),
    ('ls_k512', 'step', 'ls', _shape(512, 512, 256, 256, 640, n_loop=1), (17,), False, 512),
    ('ls_mol', 'step', 'ls', dict(H.MOL_SHALLOW), (9,), True, 514),
    ('ls_128', 'step', 'ls', _SMALL, (128,), False, 516),
    ('pn_small', 'run', 'pn', _SMALL, (1, 2, 3, 4), False, 520),
    ('pn_odd', 'run', 'pn', _ODD, (3,), False, 522),
    ('pn_256', 'run', 'pn', _shape(256, 256, 256, 256, 256), (2,), False, 524),
    ('pn_mol', 'run', 'pn', dict(H.MOL_SHALLOW), (2,), True, 526),
    ('pw_320', 'run', 'pw', _K320, (1,), False, 528),
    ('pw_512', 'run', 'pw', _shape(512, 512, 512, 256, 640, n_loop=1), (4,), False, 530),
]
BY_NAME = dict((r[0], r) for r in ROWS)
CASES = [(r[0], n) for r in ROWS for n in r[4]]                      # every (row, n) the tests run
STEP_CASES = [c for c in CASES if BY_NAME[c[0]][1] == 'step']
RUN_CASES = [c for c in CASES if BY_NAME[c[0]][1] == 'run']


def bias_tweak(seed):
    """Every decoder bias 0.1 N(0, 1), so that no bias term is a silent zero (test_gpu_generate._random_biases)."""
    def tweak(P):
        rs = np.random.RandomState(seed)
        dec = P['decoder']
        for name in ('embed', 'proj1', 'proj2'):
            dec[name] = (dec[name][0], (0.1 * rs.standard_normal(dec[name][1].shape)).astype(np.float32))
        for blk in dec['blocks']:
            for name in blk:
                blk[name] = (blk[name][0], (0.1 * rs.standard_normal(blk[name][1].shape)).astype(np.float32))
    return tweak


_PARAMS, _INPUTS = {}, {}


def params(name):
    """The decoder parameters of a row (float32, Chainer shapes): helpers.build_model(cfg, seed, tweak=bias_tweak(seed + 1))
    builds the same ones next to the device model."""
    if name not in _PARAMS:
        _, _, _, cfg, _, _, seed = BY_NAME[name]
        P = O.make_params(np.random.RandomState(seed), **cfg)
        bias_tweak(seed + 1)(P)
        _PARAMS[name] = P['decoder']
    return _PARAMS[name]


def dilations(name):
    cfg = BY_NAME[name][3]
    return O.wavenet_dilations(cfg['n_loop'], cfg['n_layer'])


def inputs(name, n):
    """The handed values of a (row, n), made once and never written to.
    'step': rings [(dilation, n, residual)] N(0, 1), x_prev / x_cur (n, input_dim) one-hot (mixture rows: a scalar in
    (-1, 1)), cond (n, condition) N(0, 1), t.  'run': cond (n, condition, T) N(0, 1), forced (T, n) with one -1 (mixture
    rows: floats in (-1, 1)), u the uniforms the sampler draws (their samples are not judged)."""
    key = (name, n)
    if key in _INPUTS:
        return _INPUTS[key]
    _, kind, _, cfg, _, mol, seed = BY_NAME[name]
    rs = np.random.RandomState(seed + 7 + 1000 * n)
    Cc, I, R = cfg['local_dim'] + cfg['global_dim'], cfg['input_dim'], cfg['residual']

    def feed(shape):
        if mol:
            return rs.uniform(-1, 1, shape + (1,)).astype(np.float32) * np.ones((I,), np.float32)
        x = np.zeros(shape + (I,), np.float32)
        idx = rs.randint(0, I, shape)
        np.put_along_axis(x, idx[..., None], 1.0, axis=-1)
        return x

    if kind == 'step':
        inp = dict(rings=[rs.standard_normal((d, n, R)).astype(np.float32) for d in dilations(name)],
                   x_prev=feed((n,)), x_cur=feed((n,)), cond=rs.standard_normal((n, Cc)).astype(np.float32), t=T_STEP)
    else:
        T = T_RUN
        cond = rs.standard_normal((n, Cc, T)).astype(np.float32)
        if mol:
            forced = rs.uniform(-1, 1, (T, n)).astype(np.float32)
            u = rs.uniform(0.02, 0.98, (T, n, cfg['out_dim'] // 3))
        else:
            forced = rs.randint(0, I, (T, n)).astype(np.int32)
            forced[3, n - 1] = -1                                   # an all-zero input vector
            u = rs.random_sample((T, n))
        inp = dict(cond=cond, forced=forced, u=u, T=T)
    _INPUTS[key] = inp
    return inp


# ---------------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------------
def _c(a, dtype):
    return np.ascontiguousarray(np.asarray(a).astype(dtype))


def cast_params(p, dtype):
    pair = lambda wb: (_c(wb[0], dtype), _c(wb[1], dtype))
    return dict(embed=pair(p['embed']), proj1=pair(p['proj1']), proj2=pair(p['proj2']),
                blocks=[dict((k, pair(v)) for k, v in blk.items()) for blk in p['blocks']])


def step(p, state, x_cur, cond_col, t, dtype):
    """One step (WaveNet/modules.py:246-255 over the device's state).  state: dict(rings=[(dilation, n, residual)],
    x_prev=(n, input_dim)); x_cur (n, input_dim); cond_col (n, condition).  Nothing is modified.
    -> dict: push[l] (n, residual) = block l's input, the new content of slot t % dilation of ring l (x_0 = the embed output,
    x_l = Wr z + br + x_{l-1}); h_final = the last block's residual output; pre[l] (n, dilated) the gate pre-activations;
    zs[l]; z = zs[-1]; skip_acc, s1, logits (n, .)."""
    p = cast_params(p, dtype)
    q = np.stack([_c(state['x_prev'], dtype), _c(x_cur, dtype)], axis=2)                 # the embed queue (modules.py:247)
    h = O.conv1d_fwd(q, p['embed'][0], p['embed'][1], stride=1, pad=0, dil=1)
    cond = _c(cond_col, dtype)[:, :, None]
    out = dict(push=[], pre=[], zs=[])
    skip_sum = None
    for blk, ring in zip(p['blocks'], state['rings']):
        dil = ring.shape[0]
        q = np.concatenate((_c(ring[t % dil], dtype)[:, :, None], h), axis=2)            # [x(t - dil), x(t)]
        hh = O.conv1d_fwd(q, blk['conv'][0], blk['conv'][1], stride=1, pad=0, dil=1)
        hh = hh + O.conv1d_fwd(cond, blk['condition_proj'][0], blk['condition_proj'][1])
        Ch = hh.shape[1] // 2
        z = np.tanh(hh[:, :Ch]) * O.sigmoid(hh[:, Ch:])
        out['push'].append(h[:, :, 0])
        out['pre'].append(hh[:, :, 0])
        out['zs'].append(z[:, :, 0])
        h = O.conv1d_fwd(z, blk['res'][0], blk['res'][1]) + q[:, :, -1:]
        skip = O.conv1d_fwd(z, blk['skip'][0], blk['skip'][1])
        skip_sum = skip if skip_sum is None else skip_sum + skip
    s = O.relu(skip_sum)
    z1 = O.relu(O.conv1d_fwd(s, p['proj1'][0], p['proj1'][1]))
    y = O.conv1d_fwd(z1, p['proj2'][0], p['proj2'][1])
    out.update(h_final=h[:, :, 0], z=out['zs'][-1], skip_acc=skip_sum[:, :, 0], s1=z1[:, :, 0], logits=y[:, :, 0])
    return out


def run(p, cond, forced, kind, dtype, n_loop=2, n_layer=3, uniforms=None):
    """The teacher-forced logits (T - 1, n, out_dim) of a whole run: the oracle's own loop on parameters and condition cast
    to `dtype`.  kind: 'softmax' | 'mol'.  The uniforms only decide samples that the forced values replace."""
    n, _, T = cond.shape
    if uniforms is None:
        uniforms = np.full((T, n) if kind == 'softmax' else (T, n, p['proj2'][0].shape[0] // 3), 0.5)
    return O.wavenet_generate(cast_params(p, dtype), _c(cond, dtype), uniforms, n_loop, n_layer, loss_kind=kind, forced=forced)[1]


def feed_vectors(forced, input_dim, mol):
    """(T, n) forced values -> the (T, n, input_dim) input vectors they stand for (generate.py:127, 139-141)."""
    forced = np.asarray(forced)
    if mol:
        return forced.astype(np.float32)[..., None] * np.ones((input_dim,), np.float32)
    x = np.zeros(forced.shape + (input_dim,), np.float32)
    for idx in np.ndindex(*forced.shape):
        if forced[idx] >= 0:
            x[idx + (int(forced[idx]),)] = 1
    return x


def run_by_steps(p, cond, forced, mol, dils, step_fn):
    """A teacher-forced run as T - 1 calls of `step_fn(state, x_cur, cond_col, t)` on rings this loop keeps.
    -> (logits (T - 1, n, out_dim), the list of what step_fn returned)."""
    n, _, T = cond.shape
    I, R = p['embed'][0].shape[1], p['embed'][0].shape[0]
    x = feed_vectors(forced, I, mol)
    # float64 rings hold a float32 push exactly
    state, x_cur, outs = dict(rings=[np.zeros((d, n, R)) for d in dils], x_prev=np.zeros((n, I), np.float32)), np.zeros((n, I), np.float32), []
    for t in range(T - 1):
        o = step_fn(state, x_cur, np.ascontiguousarray(cond[:, :, t]), t)
        for ring, push in zip(state['rings'], o['push']):
            ring[t % ring.shape[0]] = push
        state['x_prev'], x_cur = x_cur, x[t]
        outs.append(o)
    return np.stack([o['logits'] for o in outs]), outs


# ---------------------------------------------------------------------------------------------------------------------------
# float32 emulations of the two device orders
# ---------------------------------------------------------------------------------------------------------------------------
def _fma(acc, a, b):
    """The MFMA's multiply-add: the exact product added in float64, rounded to float32."""
    return (acc.astype(np.float64) + a.astype(np.float64) * b.astype(np.float64)).astype(F32)


def _mac(acc, a, b):
    """acc + a * b as the vector ALU code does it (csrc/Makefile: -ffp-contract=off): the product rounded, then the sum."""
    return _add(acc, (np.asarray(a, F32) * np.asarray(b, F32)).astype(F32))


def _add(a, b):
    return (np.asarray(a, F32) + np.asarray(b, F32)).astype(F32)


def _pad_k(a, mult):
    k = a.shape[-1]
    return a if k % mult == 0 else np.concatenate([a, np.zeros(a.shape[:-1] + (mult - k % mult,), a.dtype)], axis=-1)


def _two_tap(W, old, new):
    """(rows, Cin, 2), (n, Cin), (n, Cin) -> W (rows, 2 Cin), X (n, 2 Cin) with k = 2 c + tap."""
    return W.reshape(W.shape[0], -1), np.stack([old, new], axis=2).reshape(old.shape[0], -1)


def ls_gemm(parts, half_wave=None):
    """ls_gemm_body: parts = [(W (rows, K), X (n, K)), ...], each padded to whole 16-wide chunks and laid end to end (the
    conv's chunks, then the condition's) -> (n, rows), before the bias."""
    W = np.concatenate([_pad_k(w.astype(F32), 16) for w, _ in parts], axis=1)
    X = np.concatenate([_pad_k(x.astype(F32), 16) for _, x in parts], axis=1)
    W, X = _pad_k(W, 128), _pad_k(X, 128)                                # whole rounds of the eight waves: zeros add nothing
    rows, n, rounds = W.shape[0], X.shape[0], W.shape[1] // 128
    Wr, Xr = W.reshape(rows, rounds, 8, 4, 4), X.reshape(n, rounds, 8, 4, 4)          # [.., round, wave, lane group g, j]
    acc = np.zeros((8, n, rows), F32)
    for o in range(rounds):
        for j in range(4):
            for g in range(4):
                acc = _fma(acc, Xr[:, o, :, g, j].T[:, :, None], Wr[:, o, :, g, j].T[:, None, :])
    if half_wave is not None:
        acc[half_wave] = acc[half_wave].astype(np.float16).astype(F32)
    s = acc[0]
    for w in range(1, 8):
        s = _add(s, acc[w])
    return s


def _gate_exact(h0, h1):
    """tanhf(h0) * (1.f / (1.f + expf(-h1)))"""
    one = F32(1)
    return (np.tanh(h0) * (one / (one + np.exp(-h1)))).astype(F32)


def _emu_step_lockstep(p, state, x_cur, cond_col, t, mutation):
    out = dict(push=[])
    W, X = _two_tap(p['embed'][0], state['x_prev'], x_cur)
    h = _add(ls_gemm([(W, X)]), p['embed'][1])
    skip_acc = None
    for blk, ring in zip(p['blocks'], state['rings']):
        half = blk['conv'][0].shape[0] // 2
        W, X = _two_tap(blk['conv'][0], ring[t % ring.shape[0]].astype(F32), h)
        acc = ls_gemm([(W, X), (blk['condition_proj'][0][:, :, 0], cond_col)], 3 if mutation == 'partial_half' else None)
        hh = _add(_add(acc, blk['conv'][1]), blk['condition_proj'][1])
        z = _gate_exact(hh[:, :half], hh[:, half:])
        out['push'].append(h)
        rs = ls_gemm([(np.concatenate([blk['res'][0][:, :, 0], blk['skip'][0][:, :, 0]], axis=0), z)])
        R = blk['res'][0].shape[0]
        h = _add(_add(rs[:, :R], blk['res'][1]), h)
        sk = _add(rs[:, R:], blk['skip'][1])
        skip_acc = sk if skip_acc is None else _add(skip_acc, sk)
    s1 = np.maximum(_add(ls_gemm([(p['proj1'][0][:, :, 0], np.maximum(skip_acc, 0))]), p['proj1'][1]), 0)
    out['logits'] = _add(ls_gemm([(p['proj2'][0][:, :, 0], s1)]), p['proj2'][1])
    return out


_L = np.arange(64)
_DPP = (_L ^ 1, _L ^ 2, (_L & ~7) | (7 - (_L & 7)), (_L & ~15) | (15 - (_L & 15)))


def mega_wave_sum(v):
    """(.., 64) -> (..): four DPP adds inside each row of 16 lanes, then (r0 + r1) + (r2 + r3)."""
    for perm in _DPP:
        v = _add(v, v[..., perm])
    return _add(_add(v[..., 0], v[..., 16]), _add(v[..., 32], v[..., 48]))


def _lanes(a, per_lane):
    """(m, K) -> (m, per_lane, 64): element k = lane + 64 i."""
    a = _pad_k(a.astype(F32), 64 * per_lane)
    assert a.shape[1] == 64 * per_lane, (a.shape, per_lane)
    return a.reshape(a.shape[0], per_lane, 64)


def lane_dot(W, X, per_lane):
    """acc += w[i] * x[i] over a lane's elements in order, then the wave sum: (rows, K), (n, K) -> (n, rows)."""
    Wl, Xl = _lanes(W, per_lane), _lanes(X, per_lane)
    acc = np.zeros((X.shape[0], W.shape[0], 64), F32)
    for i in range(per_lane):
        acc = _mac(acc, Xl[:, None, i, :], Wl[None, :, i, :])
    return mega_wave_sum(acc)


def dot_z(W, Z, hv):
    """mega_dot_z and the wave sum: w0 z0 + w1 z1, or (w0 z0 + w1 z1) + (w2 z2 + w3 z3)."""
    Wl, Zl = _lanes(W, hv), _lanes(Z, hv)
    pair = lambda i: _add((Zl[:, None, i, :] * Wl[None, :, i, :]).astype(F32), (Zl[:, None, i + 1, :] * Wl[None, :, i + 1, :]).astype(F32))
    return mega_wave_sum(pair(0) if hv == 2 else _add(pair(0), pair(2)))


def mega_gate(h0, h1):
    """1 - 2 rcp(1 + exp(2 h0)) times rcp(1 + exp(-h1)), float32 throughout (NumPy's exp and division)."""
    one, two = F32(1), F32(2)
    with np.errstate(over='ignore'):
        th = one - two * (one / (one + np.exp(two * h0)))
        return (th * (one / (one + np.exp(-h1)))).astype(F32)


def mega_class(p, cond_dim):
    """(VI, CVI, HV) of the width class mega_class_of picks."""
    vec = max(p['embed'][0].shape[0], p['proj1'][0].shape[0], p['proj2'][0].shape[0])
    half = p['blocks'][0]['conv'][0].shape[0] // 2
    if vec <= 256 and cond_dim <= 256 and half <= 128:
        return 4, 4, 2
    assert vec <= 512 and cond_dim <= 640 and half <= 256
    return 8, 10, 4


_PACKED = {}


def mega_pack(p, mutation):
    """gen_mega_pack_kernel: per block l < L - 1 the composite M_l = Wc1_{l+1} Wr_l and cb_l = Wc1_{l+1} br_l, float64
    accumulation rounded once; per block conv_b + cond_b in float32."""
    key = (id(p), mutation)
    if key not in _PACKED:
        M, cb, bb = [], [], []
        for l, blk in enumerate(p['blocks']):
            bb.append(_add(blk['conv'][1], blk['condition_proj'][1]))
            if l + 1 < len(p['blocks']):
                w1 = p['blocks'][l + 1]['conv'][0][:, :, 1].astype(np.float64)
                M.append(np.matmul(w1, blk['res'][0][:, :, 0].astype(np.float64)).astype(F32))
                c = np.matmul(w1, blk['res'][1].astype(np.float64)).astype(F32)
                cb.append(c.astype(np.float16).astype(F32) if mutation == 'cb_half' else c)
        _PACKED[key] = (p, M, cb, bb)
    return _PACKED[key][1:]


def _emu_step_persistent(p, state, x_cur, cond_col, t, mutation):
    VI, CVI, HV = mega_class(p, cond_col.shape[1])
    M, cb, bb = mega_pack(p, mutation)
    L, out = len(p['blocks']), dict(push=[])
    We, be = p['embed']
    n = x_cur.shape[0]
    # embed: (e0 + e1) + b, e0 / e1 the selected (or scaled) column of each tap
    e = [np.zeros((n, We.shape[0]), F32), np.zeros((n, We.shape[0]), F32)]
    for tap, x in enumerate((state['x_prev'], x_cur)):
        for c in range(We.shape[1]):
            e[tap] = _mac(e[tap], x[:, c:c + 1], We[None, :, c, tap])
    x = _add(_add(e[0], e[1]), be)
    half = p['blocks'][0]['conv'][0].shape[0] // 2

    def pre(l):                                                        # the helper wave
        blk, ring = p['blocks'][l], state['rings'][l]
        Wl, Xl = _lanes(blk['conv'][0][:, :, 0], VI), _lanes(ring[t % ring.shape[0]], VI)
        Cl, Vl = _lanes(blk['condition_proj'][0][:, :, 0], CVI), _lanes(cond_col, CVI)
        acc = np.zeros((n, Wl.shape[0], 64), F32)
        for i in range(max(VI, CVI)):                                  # acc += w0 xo + wc cv: the two products first
            both = np.zeros_like(acc)
            if i < VI:
                both = (Xl[:, None, i, :] * Wl[None, :, i, :]).astype(F32)
            if i < CVI:
                cterm = (Vl[:, None, i, :] * Cl[None, :, i, :]).astype(F32)
                both = _add(both, cterm) if i < VI else cterm
            acc = _add(acc, both)
        return _add(mega_wave_sum(acc), bb[l])

    hh = _add(lane_dot(p['blocks'][0]['conv'][0][:, :, 1], x, VI), pre(0))
    z = mega_gate(hh[:, :half], hh[:, half:])
    sacc = None
    for l, blk in enumerate(p['blocks']):
        out['push'].append(x)
        if l + 1 < L:
            u = lane_dot(p['blocks'][l + 1]['conv'][0][:, :, 1], x, VI)                  # the shadow term Wc1_{l+1} x_l
            x = _add(_add(dot_z(blk['res'][0][:, :, 0], z, HV), blk['res'][1]), x)
            hh = _add(_add(_add(dot_z(M[l], z, HV), u), cb[l]), pre(l + 1))
            z_next = mega_gate(hh[:, :half], hh[:, half:])
        sk = _add(dot_z(blk['skip'][0][:, :, 0], z, HV), blk['skip'][1])
        sacc = sk if sacc is None else _add(sacc, sk)
        if l + 1 < L:
            z = z_next
    s1 = np.maximum(_add(lane_dot(p['proj1'][0][:, :, 0], np.maximum(sacc, 0), VI), p['proj1'][1]), 0)
    out['logits'] = _add(lane_dot(p['proj2'][0][:, :, 0], s1, VI), p['proj2'][1])
    return out


_P32 = {}
ORDERS = dict(lockstep=_emu_step_lockstep, persistent=_emu_step_persistent)
MUTATIONS = dict(lockstep='partial_half', persistent='cb_half')


def emulate(case, order, mutation=None):
    """The logits of a (row, n) in float32 in a device order: (n, out_dim) of the one step of a 'step' row, (T - 1, n, out_dim)
    of a 'run' row."""
    name, n = case
    _, kind, _, cfg, _, mol, _ = BY_NAME[name]
    if name not in _P32:
        _P32[name] = cast_params(params(name), F32)
    p, inp, fn = _P32[name], inputs(name, n), ORDERS[order]
    if kind == 'step':
        return fn(p, dict(rings=inp['rings'], x_prev=inp['x_prev']), inp['x_cur'], inp['cond'], inp['t'], mutation)['logits']
    return run_by_steps(p, inp['cond'], inp['forced'], mol, dilations(name),
                        lambda st, xc, cc, t: fn(p, st, xc, cc, t, mutation))[0]


def reference(case, dtype):
    """What `emulate` is judged against: the logits of the case from `step` / `run` in `dtype`."""
    name, n = case
    _, kind, _, cfg, _, mol, _ = BY_NAME[name]
    p, inp = params(name), inputs(name, n)
    if kind == 'step':
        return step(p, dict(rings=inp['rings'], x_prev=inp['x_prev']), inp['x_cur'], inp['cond'], inp['t'], dtype)['logits']
    return run(p, inp['cond'], inp['forced'], 'mol' if mol else 'softmax', dtype, cfg['n_loop'], cfg['n_layer'], inp['u'])
