"""ResidualNet's chain (wavenet.ResidualStackFunction) against a float64 reference, one row per edge of the shape
predicates that decide what it launches: the storage queries of csrc/conv_api.hip (z_bf16, bf16_storage_supported,
f16x2_storage_supported: T % 64, T % 128, dil < T, the two channel classes, Cs), vqvae_get_fused_pullback, the kernel
selection behind them (lin128_shape, lin_wide_shape, the lerp fold T >= 26 Tl, the fused pull-back T >= 64 Tl) and the
Python side (_plan_storage, _begin_sweep's fused / batched / per-block pull-back, _groups, DIL_WGRAD_GROUP,
DEFER_DIL_BLOCKS, PB_REDUCE_GROUP, one or two streams).  The other oracle-compared chain tests all sit at 256 or 512
channels, up-sampling 64 and T in {1024, 2048, 7680}, where every block of a chain gets the same answer.

The reference is oracle.resblock_fwd / resblock_bwd / upsample_fwd / upsample_bwd block by block on the same float32
values cast to float64.  Every row asserts the branch facts visible from Python (the storage bits each block ran with,
which pull-back form the sweep took), restated here from the predicates and not read from the planner, so a row that
drifts onto another branch fails instead of passing vacuously."""
import zlib

import numpy as np
import pytest

import vqvae_oracle as O
from helpers import assert_close, assert_close_scaled, to4
from test_gpu_kernels import _rb_params

pytestmark = pytest.mark.gpu

ORDER = ['conv', 'condition_proj', 'res', 'skip']
X16, RES16, GX16, GRES16, GH16 = 2, 4, 8, 16, 1             # VQVAE_STORE_*_BF16
GHX2, XX2, RESX2, GSIG = 32, 64, 128, 256                   # VQVAE_STORE_*_F16X2, VQVAE_STORE_GATES_SIG
NSPK = 7


def _row(name, Cr, Cs, Cl, G, T, up, dils, B=2):
    return pytest.param((name, Cr, Cs, Cl, G, T, up, tuple(dils), B), id=name)


DEEP12 = [2 ** (i % 10) for i in range(12)]
DEEP25 = [2 ** (i % 5) for i in range(25)]
# name, Cr = Cd, Cs, local + speaker condition channels, T, up-sampling, dilations, B
ROW_DIL_GE_T = _row('dil_ge_T_inside', 256, 256, 64, 128, 384, 64, DEEP12)       # blocks 8 -> 9 (dil 512 >= T) -> 10
ROW_DEEP25 = _row('blocks25', 256, 256, 64, 128, 256, 64, DEEP25, B=1)           # two _groups / PB_REDUCE_GROUPs, five dil-wgrad groups, deferred blocks
ROWS = [
    ROW_DIL_GE_T,
    _row('unsupported_second', 256, 256, 64, 128, 256, 64, [1, 512, 1, 2]),
    _row('unsupported_first', 256, 256, 64, 128, 256, 64, [512, 1, 2, 4]),       # (the pack call's descriptor is block 0's)
    _row('wide_unsupported_third', 512, 256, 64, 64, 256, 64, [1, 2, 256, 1]),   # lin_wide_shape, per-block upsample_linear_bwd_f16x2
    _row('one_tile_Tl2', 256, 256, 64, 128, 128, 64, [1, 2, 4]),                 # Tl >= 3 false: no batched pull-back
    _row('T1000_up8', 256, 256, 64, 128, 1000, 8, [1, 2, 4]),                    # T % 64 != 0: nothing stored, lin128_shape false, T = 8 Tl
    _row('T192', 256, 256, 64, 128, 192, 64, [1, 2, 4]),                         # T % 64 == 0, % 128 != 0
    _row('Cs512', 256, 512, 64, 128, 512, 64, [1, 2, 4]),                        # Cs != Cr, skip GEMM with 512 rows
    _row('Cs128', 256, 128, 64, 128, 512, 64, [1, 2, 4]),                        # Cs % 256 != 0, skip GEMM on 128-row tiles
    _row('Cc64_odd_dils', 256, 256, 40, 24, 512, 64, [1, 3, 5]),
    _row('Cc40_odd_dils', 256, 256, 30, 10, 512, 64, [1, 3, 5]),                 # Cc not a multiple of 32
    _row('up32', 256, 256, 64, 128, 1024, 32, [1, 2, 4]),                        # 26 Tl <= T < 64 Tl: lerp fold on, fused pull-back off
    _row('up16', 256, 256, 64, 128, 1024, 16, [1, 2, 4]),                        # T < 26 Tl: fold off
    _row('up4', 256, 256, 64, 128, 1024, 4, [1, 2, 4]),                          # T < 8 Tl: per-block pull-back in every mode
    ROW_DEEP25,
    _row('one_block', 256, 256, 64, 128, 256, 64, [1]),                          # first block == last block
    _row('six_blocks', 256, 256, 64, 128, 256, 64, [1] * 6),                     # DEFER_DIL_BLOCKS + 1
    _row('wide_Cs512', 512, 512, 64, 64, 384, 64, [1, 2, 4]),
    _row('generic_384', 384, 320, 64, 32, 256, 64, [1, 2, 4]),                   # neither class: the generic packed chain
]
BF16_ROWS = [
    _row('bf16_dil_ge_T', 256, 256, 64, 128, 384, 64, [256, 512, 1]),
    _row('bf16_T192', 256, 256, 64, 128, 192, 64, [1, 2, 4]),
    _row('bf16_Cs512', 256, 512, 64, 128, 512, 64, [1, 2, 4]),
    _row('bf16_Cs128', 256, 128, 64, 128, 512, 64, [1, 2, 4]),
]


def _dev(gpu, a):
    return gpu.to_device(np.ascontiguousarray(a))


_INPUTS, _REF = {}, {}


def _inputs(row):
    if row not in _INPUTS:
        name, Cr, Cs, Cl, G, T, up, dils, B = row
        assert T % up == 0 and B <= 3
        rs = np.random.RandomState(zlib.crc32(repr(row).encode()))
        _INPUTS[row] = dict(
            blocks=[_rb_params(rs, Cr, Cr, Cs, Cl + G, 2) for _ in dils],
            x=rs.standard_normal((B, Cr, T)).astype(np.float32),
            local=rs.standard_normal((B, Cl, T // up)).astype(np.float32),
            E=rs.standard_normal((NSPK, G)).astype(np.float32),
            ids=rs.randint(0, NSPK, B).astype(np.int32),
            gy=rs.standard_normal((B, Cs, T)).astype(np.float32))
    return _INPUTS[row]


def _chain_oracle(row, dtype, round_gres=False):
    """The chain block by block on the oracle (modules.py:89-96) over the materialised condition (net.py:54-63), every
    value cast to ``dtype`` -> outputs under the names _run_chain uses.  ``round_gres``: the oracle's bf16 mode with the
    stored gradient stream, as oracle.wavenet_bwd restates it (VQVAE_STORE_GX_BF16)."""
    name, Cr, Cs, Cl, G, T, up, dils, B = row
    inp = _inputs(row)
    c = lambda a: a.astype(dtype)
    blocks = [{n: (c(W), c(b)) for n, (W, b) in blk.items()} for blk in inp['blocks']]
    x, local, E, gy, ids = c(inp['x']), c(inp['local']), c(inp['E']), c(inp['gy']), inp['ids']
    cond = np.concatenate([O.upsample_fwd(local, T), np.repeat(E[ids][:, :, None], T, axis=2)], axis=1)
    assert cond.dtype == dtype
    h, caches, skip = x, [], None
    for blk, d in zip(blocks, dils):
        h, sk, cch = O.resblock_fwd(blk, h, cond, d)
        caches.append(cch)
        skip = sk if skip is None else skip + sk
    g_res, gcond, out = None, np.zeros(cond.shape, np.float64), {'skip': skip}
    for i in range(len(dils) - 1, -1, -1):
        g_res, gc, bg = O.resblock_bwd(blocks[i], caches[i], cond, dils[i], g_res, gy)
        if round_gres and i >= 1 and Cs == Cr and T % 128 == 0 and O.gh_saved_as_bf16(Cr // 2, Cr, Cs, T, 2):
            g_res = O.bf16_round(g_res)
        gcond += gc
        for j, n in enumerate(ORDER):
            if bg[n] is not None:
                out['p%d' % (8 * i + 2 * j)], out['p%d' % (8 * i + 2 * j + 1)] = bg[n]
    out['gx'] = g_res
    out['glocal'] = O.upsample_bwd(np.ascontiguousarray(gcond[:, :Cl]), T // up)
    gE = np.zeros(E.shape, np.float64)
    np.add.at(gE, ids, gcond[:, Cl:].sum(axis=2))
    out['gE'] = gE
    return out


def _reference(row):
    if row not in _REF:
        _REF[row] = _chain_oracle(row, np.float64)
    return _REF[row]


def _run_chain(gpu, row):
    """ResidualStackFunction(dils) forward and backward over F.condition_assemble(local, E, ids, up) -> (skip, gx,
    g local, g speaker embedding and every block's eight parameter gradients by name; the branch facts: the storage
    bits of every block after the forward and after the backward, which pull-back form the sweep chose)."""
    from vqvae_amd import functions as F
    from vqvae_amd.core import Variable
    from vqvae_amd.wavenet import ResidualStackFunction
    name, Cr, Cs, Cl, G, T, up, dils, B = row
    inp = _inputs(row)
    vx = Variable(_dev(gpu, to4(inp['x'])))
    vlocal, vE = Variable(_dev(gpu, to4(inp['local']))), Variable(_dev(gpu, inp['E']))
    vcond = F.condition_assemble(vlocal, vE, _dev(gpu, inp['ids']), up)
    assert isinstance(vcond.data, F.LazyUpsampled) == F.LAZY_CONDITION
    pv = []
    for blk in inp['blocks']:
        for n in ORDER:
            pv += [Variable(_dev(gpu, to4(blk[n][0]))), Variable(_dev(gpu, blk[n][1]))]
    fn = ResidualStackFunction(list(dils))
    facts = {}
    begin = fn._begin_sweep

    def spy(indexes, gys):
        s = begin(indexes, gys)
        facts.update(pb_part=s.pb_part is not None, gh_all=s.gh_all is not None, overlap=s.overlap)
        return s
    fn._begin_sweep = spy
    skip = fn.apply([vx, vcond] + pv)[0]
    facts['fwd'] = [d.storage for d in fn.descs]
    out = {'skip': skip.data.get()[..., 0]}
    skip.grad = _dev(gpu, to4(inp['gy']))
    skip.backward()
    facts['bwd'] = [d.storage for d in fn.descs]
    out['gx'] = vx.grad.get()[..., 0]
    out['glocal'] = vlocal.grad.get()[..., 0]
    out['gE'] = vE.grad.get()
    for i, v in enumerate(pv):
        if v.grad is not None:
            out['p%d' % i] = v.grad.get()
    return out, facts


def _expected_facts(row, mode, presplit=7, lazy=True, overlap=False, bf16_storage=True):
    """The branch facts of a row, restated from the predicates of csrc/conv_api.hip and wavenet._begin_sweep."""
    name, Cr, Cs, Cl, G, T, up, dils, B = row
    nb, Tl = len(dils), T // up
    fwd, bwd = [0] * nb, [0] * nb
    pb_part = lazy and mode == 'float32x2' and Cr == 256 and T % 128 == 0 and T >= 64 * Tl
    segmented = Tl >= 3 and T >= 8 * Tl and T % 4 == 0 and T // 4 <= 2048      # the only pull-back kernel that reads a stored gh
    if lazy and mode == 'float32x2' and presplit:
        shape = (Cr == 256 or (Cr == 512 and Cs in (256, 512))) and T % 128 == 0
        sup = [shape and d < T for d in dils]
        for l in range(nb):
            own = (GSIG if presplit & 4 else 0) if sup[l] else 0
            gh = GHX2 if (sup[l] and presplit & 1 and (pb_part or segmented)) else 0
            # x_{l+1} crosses l | l + 1 pre-split only if no block from l on is refused (a stored x needs a stored output)
            res = RESX2 if (presplit & 2 and l < nb - 1 and all(sup[l:])) else 0
            xin = XX2 if (presplit & 2 and l >= 1 and all(sup[l - 1:])) else 0
            fwd[l], bwd[l] = own | res | xin, own | res | xin | gh
    if lazy and mode == 'bfloat16' and bf16_storage and Cr == 256 and Cs % 256 == 0 and T % 64 == 0:
        for l in range(nb):
            stream = T % 128 == 0
            fwd[l] = ((RES16 if l < nb - 1 else 0) | (X16 if l >= 1 else 0)) if stream else 0
            grad = stream and Cs == Cr
            bwd[l] = fwd[l] | (GH16 if segmented else 0) | (((GRES16 if l < nb - 1 else 0) | (GX16 if l >= 1 else 0)) if grad else 0)
    gh_all = lazy and not pb_part and not overlap and not any(b & GHX2 for b in bwd) and segmented
    return dict(fwd=fwd, bwd=bwd, pb_part=pb_part, gh_all=gh_all, overlap=overlap)


def _errors(out, ref):
    """[(tensor name, error, 'abs1' | 'scaled')]: skip as helpers.assert_close measures it, gradients as assert_close_scaled."""
    assert set(out) == set(ref), sorted(set(out) ^ set(ref))
    errs = []
    for k in sorted(ref):
        got, want = np.asarray(out[k], np.float64).reshape(-1), np.asarray(ref[k], np.float64).reshape(-1)
        assert got.shape == want.shape, k
        if k == 'skip':
            errs.append((k, float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max()), 'abs1'))
        else:
            errs.append((k, float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30)), 'scaled'))
    return errs


def _tensor_name(k):
    if not k.startswith('p'):
        return {'skip': 'skip_connections', 'gx': 'gx', 'glocal': 'g local condition', 'gE': 'g speaker embedding'}[k]
    i = int(k[1:])
    return 'block %d g%s %s' % (i // 8, 'b' if i % 2 else 'W', ORDER[(i % 8) // 2])


def _check(row, tag, out):
    """The project's bar against the float64 reference: 1e-4 (max(1, |want|)) for skip, 1e-4 of scale for every gradient;
    the worst figure is printed first."""
    ref = _reference(row)
    last = len(row[7]) - 1
    assert 'p%d' % (8 * last + 4) not in out and 'p%d' % (8 * last + 5) not in out       # the last block's unused res conv
    errs = _errors(out, ref)
    k, e, _ = max(errs, key=lambda t: t[1])
    print('CHAIN_DOMAIN %s %s worst %.3e %s' % (row[0], tag, e, _tensor_name(k)))
    for k in sorted(ref):
        want = ref[k]
        if k == 'skip':
            assert_close(out[k], want, 1e-4, '%s %s: skip_connections' % (row[0], tag))
        else:
            assert_close_scaled(np.asarray(out[k]).reshape(want.shape), want, 1e-4, '%s %s: %s' % (row[0], tag, _tensor_name(k)))


def _assert_facts(facts, want, what):
    for k in ('fwd', 'bwd', 'pb_part', 'gh_all', 'overlap'):
        assert facts[k] == want[k], '%s: %s is %s, the predicates say %s' % (what, k, facts[k], want[k])


def _run_row(gpu, row, mode, lazy=True):
    """One row in the current matmul mode: the branch facts, then every output against the reference."""
    out, facts = _run_chain(gpu, row)
    _assert_facts(facts, _expected_facts(row, mode, lazy=lazy), '%s %s' % (row[0], mode))
    _check(row, mode, out)
    return out, facts


@pytest.mark.parametrize('row', ROWS)
def test_chain_row_vs_float64(gpu, matmul_mode, row):
    from vqvae_amd import backend
    if matmul_mode != 'float32x2':
        _run_row(gpu, row, matmul_mode)
        return
    try:
        backend.f32x2_contract_violations(reset=True)
        _, facts = _run_row(gpu, row, matmul_mode)
        rep = backend.f32x2_contract_violations()
        presplit = sum(1 for b in facts['bwd'] if b & XX2) + sum(1 for b in facts['bwd'] if b & GHX2)
        assert rep['violations'] == 0 and rep['checked'] == presplit, (rep, presplit)
        gpu.set_presplit(0)
        out0, facts0 = _run_chain(gpu, row)
        _assert_facts(facts0, _expected_facts(row, matmul_mode, presplit=0), row[0] + ' presplit 0')
        assert all(b == 0 for b in facts0['bwd'])
        _check(row, 'float32x2/presplit0', out0)
    finally:
        gpu.set_presplit(7)


def test_dil_ge_T_row_storage_facts(gpu):
    """The first row in 'float32x2', spelled out: block 9 (dil 512 >= T = 384) runs without any stored tensor, block 8
    writes an fp32 residual output and block 10 reads an fp32 input -- no block reads a format its producer did not
    write -- the stream is pre-split again across 10 | 11, and every block but 9 keeps its own gh pre-split.  The blocks
    in front of 9 keep an fp32 stream as well: the library has no kernel that reads a stored x and writes an fp32
    residual output (rb_formats), so the fp32 boundary 8 | 9 reaches back to block 0."""
    row = ROW_DIL_GE_T.values[0]
    gpu.set_matmul_dtype('float32x2')
    gpu.set_f32x2_min_gflop(0.0)
    try:
        out, facts = _run_chain(gpu, row)
    finally:
        gpu.set_f32x2_min_gflop(8.0)
        gpu.set_matmul_dtype(gpu.default_matmul_dtype())
    fwd, bwd = facts['fwd'], facts['bwd']
    assert not bwd[8] & RESX2 and bwd[9] & (XX2 | RESX2 | GHX2) == 0 and not bwd[10] & XX2, bwd
    assert bwd[9] == 0 and bwd[10] & RESX2 and bwd[11] & XX2, bwd
    for l in range(11):
        assert bool(bwd[l] & RESX2) == bool(bwd[l + 1] & XX2), (l, bwd)
        assert not bwd[l] & XX2 or bwd[l] & RESX2, (l, bwd)
    assert all(bwd[l] & GHX2 and bwd[l] & GSIG for l in range(12) if l != 9), bwd
    assert fwd == [b & ~GHX2 for b in bwd], (fwd, bwd)
    assert facts['pb_part'] and not facts['gh_all']
    _check(row, 'float32x2/facts', out)


def test_materialised_condition_row(gpu, matmul_mode):
    """The first row with functions.LAZY_CONDITION = False: the condition arrives at the full rate, the blocks run
    unpacked (nothing stored in any mode) and the condition gradient is vqvae_resstack_gcond_bwd's."""
    from vqvae_amd import functions as F
    row = ROW_DIL_GE_T.values[0]
    was = F.LAZY_CONDITION
    F.LAZY_CONDITION = False
    try:
        _, facts = _run_row(gpu, row, matmul_mode, lazy=False)
    finally:
        F.LAZY_CONDITION = was
    assert all(b == 0 for b in facts['bwd']) and not facts['pb_part'] and not facts['gh_all']


@pytest.mark.parametrize('row', [ROW_DIL_GE_T, ROW_DEEP25])
def test_two_stream_rows_equal_one_stream_bitwise(gpu, row):
    """'float32x2' with backend.set_overlap(True): the side stream runs the weight gradients and the pull-back; every
    output and gradient equals the one-stream result bit for bit (as test_two_stream_backward_is_deterministic_and_
    equals_single_stream holds at its shape), and meets the reference."""
    from vqvae_amd import backend
    was = backend.overlap_enabled()
    gpu.set_matmul_dtype('float32x2')
    gpu.set_f32x2_min_gflop(0.0)
    try:
        backend.set_overlap(False)
        one, facts1 = _run_chain(gpu, row)
        backend.set_overlap(True)
        two, facts2 = _run_chain(gpu, row)
    finally:
        backend.set_overlap(was)
        gpu.set_f32x2_min_gflop(8.0)
        gpu.set_matmul_dtype(gpu.default_matmul_dtype())
    _assert_facts(facts1, _expected_facts(row, 'float32x2'), row[0] + ' one stream')
    _assert_facts(facts2, _expected_facts(row, 'float32x2', overlap=True), row[0] + ' two streams')
    _check(row, 'float32x2/two-stream', two)
    assert set(one) == set(two)
    for k in one:
        assert np.array_equal(one[k], two[k]), '%s: %s differs between the schedules' % (row[0], _tensor_name(k))


@pytest.fixture
def bf16_mode(gpu):
    gpu.set_matmul_dtype('bfloat16')
    O.set_bf16(True)
    yield
    O.set_bf16(False)
    gpu.set_matmul_dtype(gpu.default_matmul_dtype())


def _rel_l2(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.mark.parametrize('storage', [True, False], ids=['stored', 'operand_rounding_only'])
@pytest.mark.parametrize('row', BF16_ROWS)
def test_chain_row_bf16_vs_operand_rounding_oracle(gpu, bf16_mode, row, storage):
    """'bfloat16' at the shapes where its three storage predicates part (GH alone; X / RES without GX / GRES; nothing)
    and with a dilation beyond the sequence (no bf16 predicate reads the dilation: stored like any other), with
    wavenet.BF16_STORAGE on and off, against the oracle's operand-rounding mode, which restates those rules.  The bar of
    test_config4_as_configured_bf16_step_vs_oracle, per tensor, e_ref = the bf16 oracle's relative L2 distance from the
    float64 reference: device vs bf16 oracle <= 2 e_ref + 1e-2, device vs float64 reference <= 1.5 e_ref + 1e-2."""
    from vqvae_amd import wavenet
    was = wavenet.BF16_STORAGE
    wavenet.BF16_STORAGE = storage
    try:
        O.set_bf16(True, storage=storage)
        ref16 = _chain_oracle(row, np.float32, round_gres=storage)
        out, facts = _run_chain(gpu, row)
    finally:
        wavenet.BF16_STORAGE = was
        O.set_bf16(True)
    _assert_facts(facts, _expected_facts(row, 'bfloat16', bf16_storage=storage), row[0])
    ref = _reference(row)
    assert set(out) == set(ref) == set(ref16)
    pair, ratio, fails = [], [], []
    for k in sorted(ref):
        e_pair, e_dev, e_ref = _rel_l2(out[k], ref16[k]), _rel_l2(out[k], ref[k]), _rel_l2(ref16[k], ref[k])
        pair.append(e_pair)
        ratio.append(e_dev / max(e_ref, 1e-12))
        if not e_pair <= 2.0 * e_ref + 1e-2:
            fails.append('%s: relative L2 vs the bf16 oracle %.3e (e_ref %.3e)' % (_tensor_name(k), e_pair, e_ref))
        if not e_dev <= 1.5 * e_ref + 1e-2:
            fails.append('%s: device %.3e from the float64 reference, bf16 oracle %.3e' % (_tensor_name(k), e_dev, e_ref))
    print('CHAIN_DOMAIN %s bfloat16/%s vs bf16 oracle median %.3e max %.3e; distance ratio median %.2f max %.2f'
          % (row[0], 'stored' if storage else 'operands', np.median(pair), np.max(pair), np.median(ratio), np.max(ratio)))
    assert not fails, fails
