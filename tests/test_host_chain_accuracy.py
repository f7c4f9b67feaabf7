"""CPU tests of tests/chain_accuracy_ref.py, the yardstick of tests/test_gpu_chain_accuracy.py:

  self-consistency   each float64 per-call function fed the float64 output of the one before it reproduces the oracle's
                     whole chain (oracle.resblock_fwd / resblock_bwd / upsample_bwd) to 1e-12 of scale, with the tanh half
                     of the gates read (GSIG off) and rebuilt as z / sigmoid (GSIG on);
  the reference      NumPy's float32 evaluation of every quantity is not exact (e32 > 0) and stays inside 1e-6 in both
                     metrics (3e-6 for the max metric of tanh / sigmoid / z: the pre-activation reaches ~5, and one float32
                     rounding of it is 2.4e-7 absolute on a value the non-linearity does not shrink), at every row of the GPU test;
  the emulation      split3 / split2 as csrc/gemm_common.h states them, products accumulated in fp32 in 16-deep steps, on
                     the gate GEMM's contraction of every row: the faithful arithmetic passes the GPU test's bar
                     err <= 3 e32 + 1e-7, float32x3 with a_l*b_h or with a_m*b_m dropped fails it."""
import numpy as np
import pytest

import chain_accuracy_ref as R
import vqvae_oracle as O
from test_gpu_abi_contract_chain import ROWS, _chain, _inputs

ACC_ROWS = R.ACC_ROWS
_BY_NAME = dict((p.values[0][0], p.values[0]) for p in ROWS)


def _row(name):
    return _BY_NAME[name]


def _P_all(inp, dtype=np.float64):
    """The latent-rate projection of every block with bd inside its bias (as tests/test_gpu_abi_contract_chain.py's Chain)."""
    lat = inp['lat'].astype(np.float64)
    P = [np.matmul(blk['condition_proj'][0][:, :, 0].astype(np.float64), lat)
         + (blk['condition_proj'][1].astype(np.float64) + blk['conv'][1])[None, :, None] for blk in inp['blocks']]
    return np.concatenate(P, 1).astype(dtype)


_REF64 = {}


def _ref64(name):
    if name not in _REF64:
        _REF64[name] = _chain(_row(name), _inputs(_row(name)))
    return _REF64[name]


def _scaled(got, want):
    return R.metrics(got, want)[1]


@pytest.mark.parametrize('gsig', [False, True], ids=['gates', 'gsig'])
@pytest.mark.parametrize('name', ['c256_T256', 'c512_T256'])
def test_references_reproduce_the_oracle_chain(name, gsig):
    row = _row(name)
    _, Cr, Cs, Cc, T, Tl, B, dils = row
    inp, ref = _inputs(row), _ref64(name)
    nb, Cd = len(dils), Cr
    v0, _, w0, w1 = O.resize_tables(Tl, T, np.float64)
    tab = dict(v0=v0, w0=w0, w1=w1)
    P = _P_all(inp)
    blocks = inp['blocks']
    worst = {}

    def same(got, want, what):
        e = _scaled(got, want)
        worst[what] = max(worst.get(what, 0.0), e)
        assert e <= 1e-12, '%s: %.3e of scale' % (what, e)

    x, gates, zs = [inp['x']], [], []
    for i, (p, dil) in enumerate(zip(blocks, dils)):
        f = R.resblock_fwd_packed(x[i], p['conv'][0], P[:, i * Cd:(i + 1) * Cd], tab, dil, p['res'][0], p['res'][1])
        same(np.concatenate([f['tanh'], f['sigmoid']], 1), ref['gates'][i], 'gates %d' % i)
        same(f['z'], ref['z'][i], 'z %d' % i)
        same(f['res'], ref['x'][i + 1], 'res %d' % i)
        gates.append(np.concatenate([np.full_like(f['tanh'], np.nan) if gsig else f['tanh'], f['sigmoid']], 1))
        zs.append(f['z'])
        x.append(f['res'])
    same(R.skip_fwd([p['skip'][0] for p in blocks], [p['skip'][1] for p in blocks], zs), ref['skip'], 'skip')
    g_res, ghs = None, [None] * nb
    for i in range(nb - 1, -1, -1):
        p = blocks[i]
        b = R.resblock_bwd_packed(p['conv'][0], p['res'][0], p['skip'][0], inp['gy'], g_res, gates[i], dils[i], z=zs[i], gsig=gsig)
        same(b['gh'], ref['gh'][i], 'gh %d' % i)
        same(b['gx'], ref['gx'][i], 'gx %d' % i)
        gW, gb = R.dil_wgrad(x[i], b['gh'], dils[i])
        same(gW, ref['grads'][i]['conv'][0], 'gWd %d' % i)
        same(gb, ref['grads'][i]['conv'][1], 'gbd %d' % i)
        if g_res is not None:
            gW, gb = R.lin_wgrad(zs[i], g_res)
            same(gW, ref['grads'][i]['res'][0], 'gWr %d' % i)
            same(gb, ref['grads'][i]['res'][1], 'gbr %d' % i)
        gW, gb = R.lin_wgrad(zs[i], inp['gy'])
        same(gW, ref['grads'][i]['skip'][0], 'gWs %d' % i)
        same(gb, ref['grads'][i]['skip'][1], 'gbs %d' % i)
        same(R.pullback(b['gh'], tab, Tl), ref['gP'][:, i * Cd:(i + 1) * Cd], 'gP %d' % i)
        ghs[i], g_res = b['gh'], b['gx']
    same(R.gcond_bwd([p['condition_proj'][0] for p in blocks], ghs), ref['gcond'], 'gcond')
    print('CHAIN_SELF %s gsig %d: worst %.3e of scale' % (name, gsig, max(worst.values())))


def test_a_swapped_tap_or_lerp_index_is_seen():
    """The 1e-12 bar above is not vacuous: the same functions with the taps in the other order, or with the lerp's two weights
    swapped, are off by O(1)."""
    row = _row('c256_T256')
    _, Cr, Cs, Cc, T, Tl, B, dils = row
    inp, ref = _inputs(row), _ref64('c256_T256')
    v0, _, w0, w1 = O.resize_tables(Tl, T, np.float64)
    P = _P_all(inp)[:, :Cr]
    p = inp['blocks'][0]
    good = R.resblock_fwd_packed(inp['x'], p['conv'][0], P, dict(v0=v0, w0=w0, w1=w1), dils[0])
    assert _scaled(good['z'], ref['z'][0]) <= 1e-12
    flip = R.resblock_fwd_packed(inp['x'], p['conv'][0][:, :, ::-1], P, dict(v0=v0, w0=w0, w1=w1), dils[0])
    assert _scaled(flip['z'], ref['z'][0]) > 1e-2
    off = R.resblock_fwd_packed(inp['x'], p['conv'][0], P, dict(v0=v0, w0=w1, w1=w0), dils[0])
    assert _scaled(off['z'], ref['z'][0]) > 1e-2


def _handed_from_ref(name):
    """What a faultless device run would hand each call: the float64 chain's tensors rounded to float32."""
    row = _row(name)
    _, Cr, Cs, Cc, T, Tl, B, dils = row
    inp, ref = _inputs(row), _ref64(name)
    from vqvae_amd.functions import resize_tables_host
    f = lambda a: np.ascontiguousarray(a, np.float32)
    return dict(blocks=inp['blocks'], dils=dils, tab=resize_tables_host(Tl, T), Tl=Tl, P_all=_P_all(inp, np.float32), gy=inp['gy'],
                gsig=[False] * len(dils), x_dec=[f(a) for a in ref['x']], gates=[f(a) for a in ref['gates']],
                z_dec=[f(a) for a in ref['z']], gh_dec=[f(a) for a in ref['gh']], gx_dec=[f(a) for a in ref['gx']])


GATE_QUANTITIES = ('tanh', 'sigmoid', 'z')


@pytest.mark.parametrize('name', ACC_ROWS)
def test_float32_reference_error_is_positive_and_inside_its_caps(name):
    h = _handed_from_ref(name)
    r64, r32 = R.chain_refs(h, np.float64), R.chain_refs(h, np.float32)
    assert sorted(map(repr, r64)) == sorted(map(repr, r32))
    for key in sorted(r64, key=repr):
        assert r32[key].dtype == np.float32 and r64[key].dtype == np.float64, key
        l2, mx = R.metrics(r32[key], r64[key])
        print('CHAIN_REF %s %s %s %s: e32 l2 %.3e max %.3e' % (name, key[0], key[1], key[2], l2, mx))
        assert l2 > 0 and mx > 0, key
        assert l2 <= 1e-6, (key, l2)
        assert mx <= (3e-6 if key[1] in GATE_QUANTITIES else 1e-6), (key, mx)


def _gate_contraction(name, M=64, N=96):
    """The gate GEMM's contraction of a row's first block: A = [Wd tap 0 | Wd tap 1] (M of its rows), B = [x[t - dil]; x[t]]
    (N columns from t = 64 on; the shift is the block's dilation, 64 at most, so that both windows lie inside the row), K = 2 Cr."""
    row = _row(name)
    _, Cr, Cs, Cc, T, Tl, B, dils = row
    inp = _inputs(row)
    Wd, x, dil = inp['blocks'][0]['conv'][0], inp['x'][0], min(dils[0], 64)
    A = np.ascontiguousarray(np.concatenate([Wd[:M, :, 0], Wd[:M, :, 1]], 1))
    Bm = np.ascontiguousarray(np.concatenate([x[:, 64 - dil:64 - dil + N], x[:, 64:64 + N]], 0))
    return A, Bm


@pytest.mark.parametrize('name', ACC_ROWS)
def test_emulated_split_products_pass_the_bar_and_emulated_defects_fail_it(name):
    A, Bm = _gate_contraction(name)
    assert A.shape[1] == Bm.shape[0] and A.shape[1] % 16 == 0
    want = np.matmul(A.astype(np.float64), Bm.astype(np.float64))
    e32 = R.metrics(np.matmul(A, Bm), want)
    assert A.dtype == np.float32 and all(e > 0 for e in e32)
    forms = dict(x3=R.emulate_x3(A, Bm), x2=R.emulate_x2(A, Bm), x2_bound32=R.emulate_x2(A, Bm, 32.0),
                 x3_no_lh=R.emulate_x3(A, Bm, 'lh'), x3_no_mm=R.emulate_x3(A, Bm, 'mm'))
    for form, got in sorted(forms.items()):
        err = R.metrics(got, want)
        print('CHAIN_EMU %s K %d %s: l2 %.3e (e32 %.3e) max %.3e (e32 %.3e)' % (name, A.shape[1], form, err[0], e32[0], err[1], e32[1]))
        ok = [e <= R.bar(r) for e, r in zip(err, e32)]
        if form.startswith('x3_no'):
            assert not any(ok), '%s: the defect passes the bar: %r against e32 %r' % (form, err, e32)
        else:
            assert all(ok), '%s: faithful arithmetic misses the bar: %r against e32 %r' % (form, err, e32)
