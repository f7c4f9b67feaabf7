"""C ABI contract tests: three promises of include/vqvae_hip.h that the value suite takes on trust.

  zones        writes stay inside outputs of exactly the stated shape and workspaces of EXACTLY *_workspace_bytes()
               bytes (tests/zoned.py: NaN red zones around every buffer of the call);
  inputs_only  the result depends on the inputs only: outputs and workspaces that start as zeros (plain pool buffers) and
               as NaN (zoned buffers, inputs surrounded by NaN) give the same bits, and no NaN;
  maxima       the VQVAE_AMAX_SLOTS words a producer publishes bound the tensor they describe (bit patterns), are equal
               to max |tensor| where the header says "max |y|", and feed the consuming entry point in `float32x2`.

Every case also compares the result with float64 / the oracle at the bar the entry point's existing test uses.

CONTRACTS lists every compute export of the header (tests/test_host_zoned.py fails when one has no row) with the tests
of this file -- or, for the packed chain, of tests/test_gpu_abi_contract_chain.py -- that apply each contract to it -- an empty tuple means NOT applied here, and says where the entry point is
covered by value instead -- and, under `init`, who initialises what the entry point keeps in caller memory.  That column is
the record of the reading that has to precede a poisoned workspace: a counter, cursor or flag word in a workspace may only
start as NaN when the entry point's own host code initialises it.

Shown able to fail (one-line mutations built into a scratch copy of csrc/ and run once; never committed):
  zones:       test_harness_reports_planted_writes plants four writes inside the helper's own allocation and runs an
               overrunning and an incomplete "entry point" through run_contract;
  inputs_only: `ew_kernel` storing `v + 0.f * out[i]` instead of `v` (a read of the old output, invisible on zeroed
               buffers): test_elementwise_every_op fails at all three sizes with "non-finite at flat index 0";
  maxima:      `amax_commit` skipping the atomicMax of a launch's LAST workgroup: test_conv1d_contract fails in every
               matmul mode with "published max |y|" / "published max |gx|" (words 0 against 8.96), and
               test_published_maximum_conv fails for the spike in the last tile of the last batch item (`last_all`).
The same three mutations planted in code of the packed chain are recorded in tests/test_gpu_abi_contract_chain.py.
"""
import ctypes as C
import zlib

import numpy as np
import pytest

import vqvae_oracle as O
import zoned as Z
from helpers import assert_close, assert_close_scaled
from zoned import In, Out, Ws, run_contract

pytestmark = pytest.mark.gpu

_CONV = ('test_conv1d_contract',)
_CHAIN = ('test_packed_chain_contract', 'test_packed_chain_contract_bf16')       # tests/test_gpu_abi_contract_chain.py
_CHAIN_MAX = ('test_packed_chain_contract', 'test_published_maximum_chain')
_NONE = ()


def _row(zones=_NONE, inputs_only=None, maxima=_NONE, init=''):
    return dict(zones=tuple(zones), inputs_only=tuple(zones if inputs_only is None else inputs_only), maxima=tuple(maxima),
                init=init)


_QUERY = 'size / capability query: no device memory; its value is what the zoned workspace of its entry point is cut to'
CONTRACTS = {
    # ---- optimiser / element-wise / reductions
    'vqvae_absmax': _row(['test_absmax_and_contract_check'], maxima=['test_absmax_and_contract_check'],
                         init='amax words: zeroed by the entry point (hipMemsetAsync), then raised'),
    'vqvae_adam_step': _row(['test_adam_ema_contract'], init='p, m, v: caller state, updated in place'),
    'vqvae_adam_step_dev': _row(['test_adam_ema_contract'], init='step: caller; advanced by one per call'),
    'vqvae_ema_step': _row(['test_adam_ema_contract'], init='ema: caller state'),
    'vqvae_elementwise': _row(['test_elementwise_every_op'], init='out: fully written (n elements)'),
    'vqvae_sum': _row(['test_reductions_contract'], init='ws (4096 floats): partials written by stage 1 before stage 2 reads np of them'),
    'vqvae_sqdiff_mean': _row(['test_reductions_contract'], init='ws as vqvae_sum'),
    'vqvae_sqdiff_mean_bwd': _row(['test_reductions_contract'], init='ga / gb fully written; either may be NULL'),
    'vqvae_f32x2_contract_check': _row(['test_absmax_and_contract_check'],
                                       init='report: THREE words, zeroed by the caller when it starts counting; accumulated into'),
    # ---- losses
    'vqvae_softmax_xent_workspace_bytes': _row(init=_QUERY),
    'vqvae_softmax_xent_fwd': _row(['test_softmax_xent_contract'], init='ws: per-workgroup partials, written before read'),
    'vqvae_softmax_xent_bwd': _row(['test_softmax_xent_contract'], init='gy fully written'),
    'vqvae_softmax_xent_bwd_amax': _row(['test_softmax_xent_contract'], maxima=['test_softmax_xent_contract'],
                                        init='amax_out: zeroed by the caller; raised to the documented bound'),
    'vqvae_mol_nll_fwd': _row(['test_mol_nll_contract'], init='ws: partials written before read'),
    'vqvae_mol_nll_bwd': _row(['test_mol_nll_contract'], init='gy fully written'),
    # ---- resize / condition
    'vqvae_upsample_linear_fwd': _row(['test_upsample_fwd_and_embed_broadcast_contract'], init='y rows of C * Tout inside y_bstride'),
    'vqvae_upsample_linear_bwd': _row(['test_upsample_bwd_contract'], init='gx rows of C * Tin inside gx_bstride; no workspace'),
    'vqvae_upsample_linear_bwd_bf16': _row(['test_upsample_bwd_stored_forms_contract']),
    'vqvae_upsample_linear_bwd_f16x2': _row(['test_upsample_bwd_stored_forms_contract'], init='scale words: input'),
    'vqvae_upsample_linear_bwd_blocks': _row(['test_upsample_bwd_stored_forms_contract'], init='L results gx_lstride apart'),
    'vqvae_embed_broadcast_fwd': _row(['test_upsample_fwd_and_embed_broadcast_contract']),
    'vqvae_embed_broadcast_bwd': _row(['test_upsample_fwd_and_embed_broadcast_contract'], init='ws (B * G floats): row sums written before the scatter reads them'),
    'vqvae_concat': _row(['test_concat_split_copy_list_contract']),
    'vqvae_split': _row(['test_concat_split_copy_list_contract'], init='accumulate = 1: destinations are the addend'),
    'vqvae_copy_list': _row(['test_concat_split_copy_list_contract']),
    # ---- input / embed
    'vqvae_mulaw_bins': _row(['test_input_pipeline_contract']),
    'vqvae_onehot': _row(['test_input_pipeline_contract']),
    'vqvae_embed_gather_fwd': _row(['test_embed_gather_contract']),
    'vqvae_embed_gather_bound': _row(['test_embed_gather_contract'], maxima=['test_embed_gather_contract'],
                                     init='amax_out: SET by the entry point (memset, then raised): the caller need not zero it'),
    'vqvae_embed_onehot_workspace_bytes': _row(init=_QUERY),
    'vqvae_embed_onehot_fwd': _row(['test_embed_onehot_contract'],
                                   init='flag: set to 1 by the entry point, cleared by the scan; idx fully written; ws: the dense conv\'s'),
    'vqvae_embed_onehot_wgrad': _row(['test_embed_onehot_contract'],
                                     init='ws: per-row histograms | sorted positions + class offsets (written by embed_sort_kernel of the '
                                          'same call before embed_gathersum_kernel reads them) | dense conv; LDS counters only'),
    # ---- generic conv
    'vqvae_conv1d_workspace_bytes': _row(init=_QUERY),
    'vqvae_conv1d_packed_bytes': _row(init=_QUERY),
    'vqvae_conv1d_uses_f32x2': _row(init=_QUERY),
    'vqvae_conv1d_forms': _row(init=_QUERY),
    'vqvae_conv1d_fwd': _row(_CONV, init='ws: weight slab, split-K partial slabs (every slab element is stored before the reduce '
                                         'reads it: no memset, no atomics), operand maxima (memset by the entry point)'),
    'vqvae_conv1d_fwd_amax': _row(_CONV, maxima=['test_published_maximum_conv'], init='amax.out: zeroed by the caller'),
    'vqvae_conv1d_fwd_cond': _row(['test_embed_onehot_contract'], init='skip_flag: input'),
    'vqvae_conv1d_bwd_data': _row(_CONV, init='accumulate = 0: gx fully written; 1: gx is the addend'),
    'vqvae_conv1d_bwd_data_amax': _row(_CONV, maxima=['test_published_maximum_conv'], init='amax.out: zeroed by the caller'),
    'vqvae_conv1d_bwd_data_relu': _row(_CONV, init='gx fully written (there is no accumulate)'),
    'vqvae_conv1d_bwd_weight': _row(_CONV, init='accumulate = 0: gW, gb fully written; gb may be NULL'),
    'vqvae_conv1d_bwd_weight_amax': _row(_CONV),
    'vqvae_conv1d_bwd_weight_cond': _row(['test_embed_onehot_contract'], init='skip_flag: input'),
    'vqvae_conv1d_pack': _row(_CONV, init='packed slabs of vqvae_conv1d_packed_bytes each, fully written'),
    # ---- latent-rate fusions
    'vqvae_convstack_supported': _row(init=_QUERY),
    'vqvae_convstack_workspace_bytes': _row(init=_QUERY),
    'vqvae_convstack_fwd': _row(['test_latent_fusions_contract']),
    'vqvae_convstack_bwd': _row(['test_latent_fusions_contract'], init='ws: per-sample weight-gradient shares, written before the ordered sum'),
    'vqvae_conv_s2_bwd_supported': _row(init=_QUERY),
    'vqvae_conv_s2_bwd_workspace_bytes': _row(init=_QUERY),
    'vqvae_conv_s2_bwd': _row(['test_conv_s2_bwd_contract'], init='ws: per-workgroup shares, written before the ordered sum'),
    # ---- vector quantiser
    'vqvae_vq_workspace_bytes': _row(init=_QUERY),
    'vqvae_vq_nearest_fwd': _row(['test_vq_contract'],
                                 init='ws: wmax | nflag | noverflow share one 256-B block the entry point memsets; ccount memset by the '
                                      'entry point when the candidate pass runs (k >= 1024 and N >= 1024); flagged / cand / overflow lists '
                                      'are written below the counters before they are read; n_rechecked: written'),
    'vqvae_vq_grad_w': _row(['test_vq_contract'], init='ws: cursor memset by the entry point; base / sorted / part64 written before read'),
    'vqvae_vq_paths': _row(init=_QUERY),
    # ---- residual block / stack.  The packed latent-rate-condition chain (the twelve entry points from vqvae_resblock_fwd_packed
    # on) is driven entry point by entry point in tests/test_gpu_abi_contract_chain.py (_CHAIN*: tests of that module).  The
    # workspaces hold weight slabs and split-K partials, no counters (no global atomics in conv_gemm_*.hip / wgrad.hip
    # besides the profiling totals)
    'vqvae_resblock_workspace_bytes': _row(init=_QUERY),
    'vqvae_resblock_bf16_storage': _row(init=_QUERY),
    'vqvae_resblock_f16x2_storage': _row(init=_QUERY),
    'vqvae_resstack_workspace_bytes': _row(init=_QUERY),
    'vqvae_resstack_packed_bytes': _row(init=_QUERY),
    'vqvae_resstack_dil_wgrad_workspace_bytes': _row(init=_QUERY),
    'vqvae_resblock_fwd': _row(['test_resblock_unpacked_contract'], init='ws: weight slabs + gate scratch, written by the call'),
    'vqvae_resblock_bwd': _row(['test_resblock_unpacked_contract'], init='grads_accumulate = 0: every given gradient fully written'),
    'vqvae_resblock_wgrad': _row(['test_resblock_unpacked_contract']),
    'vqvae_resblock_fwd_packed': _row(_CHAIN, maxima=_CHAIN_MAX,
                                      init='amax->res, amax->res_scale: zeroed by the caller, raised / word 0 set; gates: the tanh half is left '
                                           'unwritten under VQVAE_STORE_GATES_SIG; bf16-stored tensors: the first half of the buffer; ws: unused '
                                           'beside its size check (the slabs are `packed`)'),
    'vqvae_resblock_bwd_packed': _row(_CHAIN, maxima=_CHAIN_MAX,
                                      init='amax->gh, amax->gx, amax->gh_scale: zeroed by the caller; gh, gx, pb_part fully written (pb_part: '
                                           'all four latent positions of every tile)'),
    'vqvae_resstack_pack': _row(_CHAIN, init='packed: the slabs the packed chain reads and the maxima / norm words of each block are written; '
                                             'the condition-projection slabs and the res slabs of a block with has_res = 0 are not (compared '
                                             'through the entry points that read the image)'),
    'vqvae_resstack_skip_fwd': _row(_CHAIN, maxima=_CHAIN_MAX, init='skip_amax_out: zeroed by the caller; accumulate = 1: skip is the addend; '
                                                                   'ws: slabs, bias sums, weight maxima written before the GEMM reads them'),
    'vqvae_resstack_skip_prepare': _row(_CHAIN, init='ws: slabs | bias sums | weight maxima written; the tail of the shared workspace is not'),
    'vqvae_resstack_skip_fwd_prepared': _row(_CHAIN, maxima=_CHAIN_MAX, init='ws: input (as vqvae_resstack_skip_prepare left it); '
                                                                            'skip_amax_out: zeroed by the caller'),
    'vqvae_resstack_gcond_bwd': _row(['test_packed_chain_contract'], init='accumulate = 1: gcond is the addend; ws: slabs written before read'),
    'vqvae_resstack_skip_wgrad': _row(_CHAIN, init='accumulate = 1: gWs, gbs are the addends; ws: split-K partials written before the reduce'),
    'vqvae_resstack_res_wgrad': _row(_CHAIN, init='as skip_wgrad; blocks with g_res[l] == NULL are skipped'),
    'vqvae_resstack_dil_wgrad': _row(_CHAIN + ('test_dil_wgrad_dma_contract_presplit', 'test_dil_wgrad_dma_contract_bf16'),
                                     init='as skip_wgrad; NULL gWd[l] / gbd[l] are skipped'),
    'vqvae_pullback_reduce': _row(['test_packed_chain_contract'], init='gP fully written (every output starts from 0.f)'),
    'vqvae_pullback_reduce_into': _row(['test_packed_chain_contract'], init='the rows of the group inside gP_bstride; the rest keeps its bits'),
    # ---- generation: zones only by design, and never a poisoned workspace (vqvae_wavenet_gen_run's workspace holds the
    # flags its workgroups wait on; the call zero-fills it at t0 == 0).  Not applied here: tests/test_gpu_generate*.py.
    'vqvae_wavenet_gen_step': _row(init='device state zero-filled by the caller ("initialize")'),
    'vqvae_wavenet_gen_run': _row(init='ws zero-filled by the call at t0 == 0; never to be poisoned'),
    'vqvae_wavenet_gen_run_workspace_bytes': _row(init=_QUERY),
    'vqvae_wavenet_gen_run_concurrency': _row(init=_QUERY),
}


# --------------------------------------------------------------------------- #
def _L():
    from vqvae_amd import _lib
    return _lib


def _call(gpu, name, *args):
    _L().call(name, *(args + (gpu.stream(),)))


def _rs(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()))


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _amax_of(words):
    return float(np.asarray(words, np.uint32).max().reshape(1).view(np.float32)[0])


def _bits32(x):
    return int(np.float32(x).reshape(1).view(np.uint32)[0])


ZERO_WORDS = np.zeros(16, np.uint32)


@pytest.fixture
def bf16_mode(gpu):
    gpu.set_matmul_dtype('bfloat16')
    O.set_bf16(True)
    yield 'bfloat16'
    O.set_bf16(False)
    gpu.set_matmul_dtype(gpu.default_matmul_dtype())


# --------------------------------------------------------------------------- #
# the harness itself
# --------------------------------------------------------------------------- #
def test_harness_reports_planted_writes(gpu):
    """Four writes planted with vqvae_memcpy_d2d INSIDE the helper's own allocation -- one byte before and after the
    payload, and the far end of each zone -- must each fail the check at the right offset; an untouched buffer passes."""
    L = _L()
    host = np.arange(1000, dtype=np.float32)
    host.view(np.uint32)[1] = 0xA5A5A5A5                     # the byte that is planted
    for shift in (0, 4):
        z = Z.ZonedArray(gpu, host=host, shift_bytes=shift, name='victim')
        z.check()
        np.testing.assert_array_equal(z.get().view(np.uint32), host.view(np.uint32))
        assert z.ptr % 256 == shift
        lay = z.layout
        for pos in (lay.start - 1, lay.end, 0, lay.total - 1):
            assert Z.pattern_bytes(lay)[pos] != 0xA5
            z = Z.ZonedArray(gpu, host=host, shift_bytes=shift, name='victim')
            L.call('vqvae_memcpy_d2d', z.block.ptr + pos, z.ptr + 4, 1, gpu.stream())
            gpu.synchronize()
            found = z.corruption()
            assert len(found) == 1 and found[0].first == found[0].last == pos - lay.start, [str(c) for c in found]
            with pytest.raises(AssertionError, match='victim: (front|back) zone corrupted'):
                z.check()

    def overrun(b):           # an "entry point" that stores one float too many, through run_contract
        L.call('vqvae_memcpy_d2d', b.y.ptr, b.x.ptr, 4 * 11, gpu.stream())
    with pytest.raises(AssertionError, match='write outside a buffer'):
        run_contract(gpu, overrun, dict(x=In(np.ones(16, np.float32)), y=Out((10,))))

    def lazy(b):              # ... and one that leaves the last element unwritten
        L.call('vqvae_memcpy_d2d', b.y.ptr, b.x.ptr, 4 * 9, gpu.stream())
    with pytest.raises(AssertionError, match='non-finite at flat index 9'):
        run_contract(gpu, lazy, dict(x=In(np.ones(16, np.float32)), y=Out((10,))))


# --------------------------------------------------------------------------- #
# optimiser, element-wise, reductions
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize('n', [1, 255, 100003])
def test_elementwise_every_op(gpu, n):
    L = _L()
    rs = _rs('ew', n)
    a, b = _f32(rs.standard_normal(n)), _f32(rs.standard_normal(n))
    al, be = np.float32(0.75), np.float32(-1.5)
    want = {L.EW_ADD: a + b, L.EW_SUB: a - b, L.EW_MUL: a * b, L.EW_AXPBY: al * a + be * b, L.EW_SCALE: al * a,
            L.EW_SQUARE: a * a, L.EW_RELU: np.maximum(a, 0), L.EW_RELU_BWD: a * (b > 0), L.EW_FILL: np.full(n, al),
            L.EW_MUL_SCALAR_DEV: (a * b[0]) * al}
    assert len(want) == 10
    for op, ref in want.items():
        r = run_contract(gpu, lambda q: _call(gpu, 'vqvae_elementwise', op, n, q.a.ptr, q.b.ptr, q.out.ptr, float(al), float(be)),
                         dict(a=In(a), b=In(b), out=Out((n,))))
        np.testing.assert_array_equal(r['out'], _f32(ref), 'op %d' % op)


@pytest.mark.parametrize('n', [1, 255, 257, (1 << 20) + 3])
def test_reductions_contract(gpu, n):
    rs = _rs('red', n)
    a, b = _f32(rs.standard_normal(n)), _f32(rs.standard_normal(n))
    g = _f32([1.75])
    r = run_contract(gpu, lambda q: _call(gpu, 'vqvae_sum', q.a.ptr, n, 0.5, q.out.ptr, q.ws.ptr, 4096 * 4),
                     dict(a=In(a), out=Out((1,)), ws=Ws(4096 * 4)))
    assert_close(r['out'], 0.5 * a.astype(np.float64).sum(), 1e-6 * max(1.0, np.sqrt(n)), 'sum')
    r = run_contract(gpu, lambda q: _call(gpu, 'vqvae_sqdiff_mean', q.a.ptr, q.b.ptr, n, q.out.ptr, q.ws.ptr, 4096 * 4),
                     dict(a=In(a), b=In(b), out=Out((1,)), ws=Ws(4096 * 4)))
    assert_close(r['out'], ((a.astype(np.float64) - b) ** 2).mean(), 1e-6, 'sqdiff_mean')
    want = 2.0 * (a.astype(np.float64) - b) * 1.75 / n
    r = run_contract(gpu, lambda q: _call(gpu, 'vqvae_sqdiff_mean_bwd', q.a.ptr, q.b.ptr, q.g.ptr, n, q.ga.ptr, q.gb.ptr),
                     dict(a=In(a), b=In(b), g=In(g), ga=Out((n,)), gb=Out((n,))))
    assert_close_scaled(r['ga'], want, 1e-5, 'ga')
    np.testing.assert_array_equal(r['gb'], -r['ga'])
    r = run_contract(gpu, lambda q: _call(gpu, 'vqvae_sqdiff_mean_bwd', q.a.ptr, q.b.ptr, q.g.ptr, n, None, q.gb.ptr),
                     dict(a=In(a), b=In(b), g=In(g), gb=Out((n,))))
    assert_close_scaled(r['gb'], -want, 1e-5, 'gb alone')


@pytest.mark.parametrize('n', [1, 255, 100003])
def test_adam_ema_contract(gpu, n):
    rs = _rs('adam', n)
    p, g, m = [_f32(rs.standard_normal(n)) for _ in range(3)]
    v = _f32(rs.uniform(0.1, 1.0, n))
    lr = 2e-4 * np.sqrt(1 - 0.999 ** 3) / (1 - 0.9 ** 3)
    p0, m0, v0 = p.copy(), m.copy(), v.copy()
    # the oracle's update rule on the same state (rounded where NumPy rounds), written out
    m1 = m0 + np.float32(1 - 0.9) * (g - m0)
    v1 = v0 + np.float32(1 - 0.999) * (g * g - v0)
    p1 = p0 - np.float32(lr) * m1 / (np.sqrt(v1) + np.float32(1e-8))
    r = run_contract(gpu, lambda q: _call(gpu, 'vqvae_adam_step', q.p.ptr, q.g.ptr, q.m.ptr, q.v.ptr, n, lr, 0.9, 0.999, 1e-8),
                     dict(g=In(g), p=Out(init=p), m=Out(init=m), v=Out(init=v)))
    np.testing.assert_array_equal(r['m'], m1)
    np.testing.assert_array_equal(r['v'], v1)
    assert_close(r['p'], p1, 1e-7, 'adam p')
    table = _f32([9.0, 9.0, lr, 9.0])
    r2 = run_contract(gpu, lambda q: _call(gpu, 'vqvae_adam_step_dev', q.p.ptr, q.g.ptr, q.m.ptr, q.v.ptr, n, q.table.ptr,
                                            q.step.ptr, 0.9, 0.999, 1e-8),
                      dict(g=In(g), table=In(table), p=Out(init=p), m=Out(init=m), v=Out(init=v),
                           step=Out(init=np.array([2], np.int32))))
    assert int(r2['step'][0]) == 3
    for k in 'pmv':
        np.testing.assert_array_equal(r2[k], r[k], 'adam_step_dev == adam_step: ' + k)
    e, t = _f32(rs.standard_normal(n)), _f32(rs.standard_normal(n))
    r = run_contract(gpu, lambda q: _call(gpu, 'vqvae_ema_step', q.e.ptr, q.t.ptr, n, 0.9999), dict(t=In(t), e=Out(init=e)))
    want = e.copy()
    O.ema_update(want, t, 0.9999)
    np.testing.assert_array_equal(r['e'], want)


def test_absmax_and_contract_check(gpu):
    """vqvae_absmax zeroes and raises its words (a poisoned group must come out right); vqvae_f32x2_contract_check reads and
    writes exactly THREE report words, batches 64 pairs per launch and skips NULL pairs and all-zero groups."""
    for n in (1, 255, 100003):
        x = _f32(_rs('absmax', n).standard_normal(n))
        x[n - 1] = -64.0                                     # the maximum is the LAST element, and negative
        r = run_contract(gpu, lambda q: _call(gpu, 'vqvae_absmax', q.x.ptr, n, q.words.ptr),
                         dict(x=In(x), words=Out((16,), np.uint32)))
        assert int(r['words'].max()) == _bits32(64.0)
    for npairs in (1, 64, 65):
        scale = [np.zeros(16, np.uint32) for _ in range(npairs)]
        amax = [np.zeros(16, np.uint32) for _ in range(npairs)]
        for i in range(npairs):
            scale[i][0] = _bits32(8.0)
            amax[i][(i * 5) % 16] = _bits32(4.0 if i != npairs - 1 else 8.0 / 1024)     # the LAST pair breaks log2_limit = 8
        amax[0][:] = 0                                       # an all-zero tensor: skipped
        null = 1 if npairs > 2 else None                     # a NULL pair: skipped
        specs = dict(report=Out(init=np.array([1, 0, 2], np.uint32)))
        for i in range(npairs):
            specs['s%d' % i] = In(scale[i])
            specs['a%d' % i] = In(amax[i])

        def fn(q):
            sp = (C.c_void_p * npairs)(*[None if i == null else q['s%d' % i].ptr for i in range(npairs)])
            ap = (C.c_void_p * npairs)(*[q['a%d' % i].ptr for i in range(npairs)])
            _call(gpu, 'vqvae_f32x2_contract_check', npairs, sp, ap, 8, q.report.ptr)
        r = run_contract(gpu, fn, specs)
        checked = npairs - 1 - (1 if null is not None else 0)
        viol = 1 if npairs > 1 else 0
        worst = 1024.0 if npairs > 1 else 0.0
        assert r['report'].tolist() == [1 + viol, _bits32(worst), 2 + checked], (npairs, r['report'])


# --------------------------------------------------------------------------- #
# losses
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize('q,B,T', [(3, 1, 1), (50, 3, 21), (256, 1, 65), (50, 1, 20001), (256, 3, 63), (3, 5, 13),
                                     (3, 1, 4), (50, 3, 20), (256, 2, 128)])       # T % 4 == 0: xent_bwd4_kernel
def test_softmax_xent_contract(gpu, q, B, T):
    """Class counts that do not divide by four, row counts around the 64-row workgroup, logits of +-80, a row of equal
    logits, targets 0 and q - 1; the bound published beside gy against the looseness the header states for it."""
    lib = _L().load()
    rs = _rs('xent', q, B, T)
    y = _f32(3 * rs.standard_normal((B, q, T)))
    t = rs.randint(0, q, (B, T)).astype(np.int32)
    y[0, :, 0] = 1.25                                        # equal logits
    t[0, 0] = q - 1
    if T > 2:
        y[B - 1, :, T - 1] = -80.0
        y[B - 1, q - 1, T - 1] = 80.0                        # the last row of the last batch item: +-80
        t[B - 1, T - 1] = 0
        y[0, 0, 1] = 80.0
        t[0, 1] = 0
    y64 = y.astype(np.float64)
    mx = y64.max(axis=1, keepdims=True)
    lse64 = (mx + np.log(np.exp(y64 - mx).sum(axis=1, keepdims=True)))
    logp = y64 - lse64
    loss64 = -np.take_along_axis(logp, t[:, None, :].astype(np.int64), 1).mean()
    ws_bytes = lib.vqvae_softmax_xent_workspace_bytes(B, q, T)
    r = run_contract(gpu, lambda b: _call(gpu, 'vqvae_softmax_xent_fwd', b.y.ptr, b.t.ptr, B, q, T, b.lse.ptr, b.loss.ptr,
                                          b.ws.ptr, ws_bytes),
                     dict(y=In(y), t=In(t, index_range=(0, q)), lse=Out((B, T)), loss=Out((1,)), ws=Ws(ws_bytes)))
    assert_close(r['loss'], loss64, 1e-5, 'loss')
    assert_close(r['lse'], lse64[:, 0, :], 1e-5, 'lse')
    gl = _f32([0.5])
    gy64 = np.exp(logp)
    np.put_along_axis(gy64, t[:, None, :].astype(np.int64), np.take_along_axis(gy64, t[:, None, :].astype(np.int64), 1) - 1, 1)
    gy64 *= 0.5 / (B * T)
    lse = r['lse']
    r = run_contract(gpu, lambda b: _call(gpu, 'vqvae_softmax_xent_bwd', b.y.ptr, b.t.ptr, b.lse.ptr, b.gl.ptr, B, q, T, b.gy.ptr),
                     dict(y=In(y), t=In(t, index_range=(0, q)), lse=In(lse), gl=In(gl), gy=Out((B, q, T))))
    assert_close_scaled(r['gy'], gy64, 1e-4, 'gy')
    r2 = run_contract(gpu, lambda b: _call(gpu, 'vqvae_softmax_xent_bwd_amax', b.y.ptr, b.t.ptr, b.lse.ptr, b.gl.ptr, B, q, T,
                                           b.gy.ptr, b.words.ptr),
                      dict(y=In(y), t=In(t, index_range=(0, q)), lse=In(lse), gl=In(gl), gy=Out((B, q, T)),
                           words=Out(init=ZERO_WORDS)))
    np.testing.assert_array_equal(r2['gy'], r['gy'])
    bound, true_max = _amax_of(r2['words']), float(np.abs(r2['gy']).max())
    assert bound >= true_max, (bound, true_max)
    assert bound <= 0.5 / (B * T) * 1.005, 'the bound is |gloss| / (B T) within a few 1e-3: %r' % bound


@pytest.mark.parametrize('nm,B,T', [(1, 1, 1), (10, 3, 63), (16, 1, 257), (10, 2, 1000)])
def test_mol_nll_contract(gpu, nm, B, T):
    rs = _rs('mol', nm, B, T)
    t = _f32(rs.uniform(-1, 1, (B, 1, T)))
    t[0, 0, 0] = -1.0
    t[B - 1, 0, T - 1] = 1.0
    y = _f32(rs.standard_normal((B, 3 * nm, T)))
    y[:, nm:2 * nm] = 127.5 * t + 30 * _f32(rs.standard_normal((B, nm, T)))
    y[:, 2 * nm:] = _f32(rs.uniform(0.5, 3.5, (B, nm, T)))
    gl = _f32([1.0])
    r = run_contract(gpu, lambda b: _call(gpu, 'vqvae_mol_nll_fwd', b.y.ptr, b.t.ptr, B, nm, T, 256, -40.0, b.loss.ptr, b.ws.ptr, 4096 * 4),
                     dict(y=In(y), t=In(t), loss=Out((1,)), ws=Ws(4096 * 4)))
    assert_close(r['loss'], O.mol_loss_fwd(y, t), 1e-4, 'mol loss')
    r = run_contract(gpu, lambda b: _call(gpu, 'vqvae_mol_nll_bwd', b.y.ptr, b.t.ptr, b.gl.ptr, B, nm, T, 256, -40.0, b.gy.ptr),
                     dict(y=In(y), t=In(t), gl=In(gl), gy=Out((B, 3 * nm, T))))
    assert_close_scaled(r['gy'], O.mol_loss_bwd(y, t), 1e-4, 'mol grad')


# --------------------------------------------------------------------------- #
# resize / condition
# --------------------------------------------------------------------------- #
def _tables(Tin, Tout):
    from vqvae_amd.functions import resize_tables_host
    return resize_tables_host(Tin, Tout)


def _upsample_bwd64(gy, tab, Tin):
    """float64 adjoint of y[i] = w0[i] x[v0[i]] + w1[i] x[v1[i]] over the (float32) tables the kernel is handed."""
    B, C, Tout = gy.shape
    g = gy.reshape(B * C, Tout).astype(np.float64)
    out = np.zeros((B * C, Tin))
    np.add.at(out.T, tab['v0'], (g * tab['w0'].astype(np.float64)).T)
    np.add.at(out.T, tab['v1'], (g * tab['w1'].astype(np.float64)).T)
    return out.reshape(B, C, Tin)


UPS_BWD_CASES = [
    # B, C, Tin, Tout, gy row pad (floats), gx row pad, shift of gy (bytes): what the dispatch of vqvae_upsample_linear_bwd sees
    (1, 1, 3, 24, 0, 0, 0),          # segmented kernel, its smallest Tin and ratio
    (3, 5, 15, 960, 0, 0, 0),        # segmented, ratio 64
    (1, 513, 15, 120, 8, 4, 0),      # segmented, more rows than persistent workgroups, both strides padded
    (2, 550, 120, 7684, 0, 0, 0),    # segmented, non-integral ratio, B * C = 1100
    (1, 3, 120, 8192, 0, 0, 0),      # segmented: Tout / 4 == 2048 exactly
    (1, 3, 120, 8196, 0, 0, 0),      # one column group above: the rows kernel (float4 staging, two passes)
    (2, 3, 120, 960, 0, 0, 4),       # gy shifted by 4 B: the rows kernel, scalar staging
    (2, 3, 15, 962, 0, 0, 0),        # Tout % 4 != 0: rows kernel, scalar staging
    (1, 2, 15, 961, 3, 1, 0),        # odd everything, odd strides
    (3, 4, 64, 256, 0, 0, 0),        # ratio 4: rows kernel, pipelined staging
    (1, 600, 32, 128, 0, 0, 0),      # ... with more rows than persistent workgroups
    (2, 3, 1, 64, 0, 0, 0),          # Tin = 1 (its own branch of the host tables)
    (2, 3, 2, 64, 0, 0, 0),          # Tin = 2
    (1, 2, 3, 9000, 0, 0, 0),        # above the LDS limit of the rows kernel: the grid-stride kernel
    (1, 2, 2000, 9001, 0, 0, 0),     # ... with short ranges
]


@pytest.mark.parametrize('case', UPS_BWD_CASES, ids=lambda c: 'B%d_C%d_%dto%d_pad%d_%d_shift%d' % c)
def test_upsample_bwd_contract(gpu, case):
    B, C, Tin, Tout, gpad, xpad, shift = case
    rs = _rs('upsb', case)
    tab = _tables(Tin, Tout)
    gyb, gxb = C * Tout + gpad, C * Tin + xpad
    gy_full = _f32(rs.standard_normal((B, gyb)))             # the padding holds finite junk the kernel must not sum
    gy = gy_full[:, :C * Tout].reshape(B, C, Tout)
    valid = np.zeros((B, gxb), bool)
    valid[:, :C * Tin] = True
    specs = dict(gy=In(gy_full, shift=shift), gx=Out((B, gxb), valid=valid))
    for k in ('w0', 'w1'):
        specs[k] = In(tab[k])
    for k in ('lo0', 'hi0', 'lo1', 'hi1'):
        specs[k] = In(tab[k], index_range=(0, Tout))
    r = run_contract(gpu, lambda b: _call(gpu, 'vqvae_upsample_linear_bwd', b.gy.ptr, gyb, B, C, Tin, Tout, b.w0.ptr, b.w1.ptr,
                                          b.lo0.ptr, b.hi0.ptr, b.lo1.ptr, b.hi1.ptr, b.gx.ptr, gxb), specs)
    got = r['gx'][:, :C * Tin].reshape(B, C, Tin)
    assert_close_scaled(got, _upsample_bwd64(gy, tab, Tin), 1e-5, 'gx')
    if Tin > 1:
        assert_close_scaled(got, O.upsample_bwd(gy.astype(np.float64), Tin), 1e-5, 'gx against the oracle')


def _bf16_round(a):
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return u.astype(np.uint16)


def _presplit(v, bound):
    """float32x2's pre-split storage: one dword per element = fp16 hi | fp16 lo << 16 of v * 2^(14 - e(bound))."""
    e = int(np.floor(np.log2(np.float64(np.float32(bound)))))
    y = np.ldexp(v.astype(np.float32), 14 - e)
    hi = y.astype(np.float16)
    lo = (y - hi.astype(np.float32)).astype(np.float16)
    words = hi.view(np.uint16).astype(np.uint32) | (lo.view(np.uint16).astype(np.uint32) << 16)
    scale = np.zeros(16, np.uint32)
    scale[0] = _bits32(bound)
    return words, scale, np.ldexp(hi.astype(np.float64) + lo.astype(np.float64), e - 14)


@pytest.mark.parametrize('B,C,Tin,Tout,L', [(1, 1, 3, 24, 1), (2, 5, 15, 960, 3), (1, 520, 15, 120, 3), (1, 3, 120, 8192, 1),
                                            (2, 7, 120, 7684, 1)])
def test_upsample_bwd_stored_forms_contract(gpu, B, C, Tin, Tout, L):
    """gy stored as bf16, pre-split, and L tensors in one launch with padded layer and batch strides."""
    rs = _rs('upss', B, C, Tin, Tout, L)
    tab = _tables(Tin, Tout)
    tabs = dict((k, In(tab[k])) for k in ('w0', 'w1'))
    tabs.update((k, In(tab[k], index_range=(0, Tout))) for k in ('lo0', 'hi0', 'lo1', 'hi1'))

    def targs(b):
        return (b.w0.ptr, b.w1.ptr, b.lo0.ptr, b.hi0.ptr, b.lo1.ptr, b.hi1.ptr)
    gy = _f32(rs.standard_normal((L, B, C, Tout)))
    gy[L - 1, B - 1, C - 1, Tout - 1] = 40.0                  # the very last element carries weight
    # bf16
    h = _bf16_round(gy[0])
    dec = (h.astype(np.uint32) << 16).view(np.float32).reshape(B, C, Tout)
    r = run_contract(gpu, lambda b: _call(gpu, 'vqvae_upsample_linear_bwd_bf16', b.gy.ptr, C * Tout, B, C, Tin, Tout, *(targs(b) + (b.gx.ptr, C * Tin))),
                     dict(tabs, gy=In(h), gx=Out((B, C, Tin))))
    assert_close_scaled(r['gx'], _upsample_bwd64(dec, tab, Tin), 1e-5, 'gx from bf16')
    # pre-split
    words, scale, dec = _presplit(gy[0], 50.0)
    r = run_contract(gpu, lambda b: _call(gpu, 'vqvae_upsample_linear_bwd_f16x2', b.gy.ptr, C * Tout, B, C, Tin, Tout,
                                          *(targs(b) + (b.gx.ptr, C * Tin, b.scale.ptr))),
                     dict(tabs, gy=In(words), scale=In(scale), gx=Out((B, C, Tin))))
    assert_close_scaled(r['gx'], _upsample_bwd64(dec, tab, Tin), 1e-5, 'gx from pre-split')
    # L tensors, fp32 and bf16, every stride padded
    gyb, gyl = C * Tout + 4, B * (C * Tout + 4) + 8
    gxb, gxl = C * Tin + 3, B * (C * Tin + 3) + 5
    full = _f32(rs.standard_normal((L, gyl)))
    valid = np.zeros((L, gxl), bool)
    for l in range(L):
        for bi in range(B):
            full[l, bi * gyb: bi * gyb + C * Tout] = gy[l, bi].reshape(-1)
            valid[l, bi * gxb: bi * gxb + C * Tin] = True
    want = np.stack([_upsample_bwd64(gy[l], tab, Tin) for l in range(L)])
    wantb = np.stack([_upsample_bwd64((_bf16_round(gy[l]).astype(np.uint32) << 16).view(np.float32).reshape(B, C, Tout), tab, Tin)
                      for l in range(L)])
    for bf16, src, ref in ((0, full, want), (1, _bf16_round(full), wantb)):
        r = run_contract(gpu, lambda b: _call(gpu, 'vqvae_upsample_linear_bwd_blocks', b.gy.ptr, bf16, gyl, gyb, L, B, C, Tin, Tout,
                                              *(targs(b) + (b.gx.ptr, gxl, gxb))),
                         dict(tabs, gy=In(src), gx=Out((L, gxl), valid=valid)))
        got = np.stack([np.stack([r['gx'][l, bi * gxb: bi * gxb + C * Tin].reshape(C, Tin) for bi in range(B)]) for l in range(L)])
        assert_close_scaled(got, ref, 1e-5, 'gx of %d tensors (bf16 = %d)' % (L, bf16))


@pytest.mark.parametrize('B,C,Tin,Tout,G', [(1, 1, 1, 5, 1), (3, 5, 15, 961, 7), (2, 24, 120, 7680, 10)])
def test_upsample_fwd_and_embed_broadcast_contract(gpu, B, C, Tin, Tout, G):
    """Both write a channel slice of the (B, C + G, Tout) condition tensor: the rows between the slices must keep their bits."""
    rs = _rs('upf', B, C, Tin, Tout, G)
    tab = _tables(Tin, Tout)
    x = _f32(rs.standard_normal((B, C, Tin)))
    n_id = 6
    E = _f32(rs.standard_normal((n_id, G)))
    ids = rs.randint(0, n_id, B).astype(np.int32)
    ybs = (C + G) * Tout
    vup = np.zeros((B, C + G, Tout), bool)
    vup[:, :C] = True
    specs = dict(x=In(x), y=Out((B, C + G, Tout), valid=vup), v0=In(tab['v0'], index_range=(0, Tin)),
                 v1=In(tab['v1'], index_range=(0, Tin)), w0=In(tab['w0']), w1=In(tab['w1']))
    r = run_contract(gpu, lambda b: _call(gpu, 'vqvae_upsample_linear_fwd', b.x.ptr, B, C, Tin, Tout, b.v0.ptr, b.v1.ptr, b.w0.ptr,
                                          b.w1.ptr, b.y.ptr, ybs), specs)
    want = tab['w0'] * x[:, :, tab['v0']] + tab['w1'] * x[:, :, tab['v1']]
    np.testing.assert_array_equal(r['y'][:, :C], want)
    # the speaker slice: y + C * Tout, same batch stride; the zoned payload is the slice-to-end view of the tensor
    n = B * ybs - C * Tout
    vb = np.zeros(n, bool)
    for bi in range(B):
        vb[bi * ybs: bi * ybs + G * Tout] = True
    r = run_contract(gpu, lambda b: _call(gpu, 'vqvae_embed_broadcast_fwd', b.E.ptr, b.ids.ptr, B, G, Tout, b.y.ptr, ybs),
                     dict(E=In(E), ids=In(ids, index_range=(0, n_id)), y=Out((n,), valid=vb)))
    for bi in range(B):
        np.testing.assert_array_equal(r['y'][bi * ybs: bi * ybs + G * Tout].reshape(G, Tout), np.repeat(E[ids[bi]][:, None], Tout, 1))
    gy = _f32(rs.standard_normal((B, C + G, Tout)))
    gflat = gy.reshape(-1)[C * Tout:]
    want = np.zeros((n_id, G))
    np.add.at(want, ids, gy[:, C:].astype(np.float64).sum(axis=2))
    for acc in (0, 1):
        init = _f32(rs.standard_normal((n_id, G)))
        r = run_contract(gpu, lambda b: _call(gpu, 'vqvae_embed_broadcast_bwd', b.gy.ptr, ybs, b.ids.ptr, B, G, Tout, n_id, b.gE.ptr, acc,
                                              b.ws.ptr, B * G * 4),
                         dict(gy=In(gflat), ids=In(ids, index_range=(0, n_id)), ws=Ws(B * G * 4),
                              gE=Out(init=init) if acc else Out((n_id, G))))
        assert_close_scaled(r['gE'], want + (init if acc else 0), 1e-5, 'gE accumulate = %d' % acc)


def test_concat_split_copy_list_contract(gpu):
    L = _L()
    rs = _rs('concat')
    for n, count in ((1, 1), (32, 5), (3, 4099), (32, 4099)):
        srcs = [_f32(rs.standard_normal(count)) for _ in range(n)]
        specs = dict(('s%d' % i, In(srcs[i])) for i in range(n))
        specs['dst'] = Out((n * count,))
        r = run_contract(gpu, lambda b: _call(gpu, 'vqvae_concat', b.dst.ptr, (C.c_void_p * n)(*[b['s%d' % i].ptr for i in range(n)]), n, count), specs)
        np.testing.assert_array_equal(r['dst'], np.concatenate(srcs))
        src = np.concatenate(srcs)
        skip = n // 2 if n > 1 else None                     # a NULL destination is skipped
        for acc in (0, 1):
            init = [_f32(rs.standard_normal(count)) for _ in range(n)]
            specs = dict(src=In(src))
            for i in range(n):
                if i != skip:
                    specs['d%d' % i] = Out(init=init[i]) if acc else Out((count,))
            r = run_contract(gpu, lambda b: _call(gpu, 'vqvae_split', b.src.ptr,
                                                  (C.c_void_p * n)(*[None if i == skip else b['d%d' % i].ptr for i in range(n)]), n, count, acc), specs)
            for i in range(n):
                if i != skip:
                    np.testing.assert_array_equal(r['d%d' % i], srcs[i] + init[i] if acc else srcs[i])
    # 33 arrays: an error code, and nothing is launched (the destination keeps its bits)
    d = Z.ZonedArray(gpu, shape=(33,), name='dst')
    one = gpu.to_device(np.ones(1, np.float32))
    ptrs = (C.c_void_p * 33)(*[one.ptr] * 33)
    lib = L.load()
    assert lib.vqvae_concat(d.ptr, ptrs, 33, 1, gpu.stream()) == -1
    assert lib.vqvae_split(one.ptr, (C.c_void_p * 33)(*[d.ptr + 4 * i for i in range(33)]), 33, 1, 0, gpu.stream()) == -1
    gpu.synchronize()
    d.check()
    assert (d.get().view(np.uint32) == Z.POISON_WORD).all()
    for n in (1, 64, 65, 130):                               # 64 jobs per launch; unequal counts, some empty
        counts = [int(c) for c in rs.randint(0, 3000, n)]
        counts[0], counts[-1] = 2999, 1
        srcs = [_f32(rs.standard_normal(max(c, 1))) for c in counts]
        specs = {}
        for i in range(n):
            specs['s%d' % i] = In(srcs[i])
            specs['d%d' % i] = Out((max(counts[i], 1),), valid=np.arange(max(counts[i], 1)) < counts[i])
        r = run_contract(gpu, lambda b: _call(gpu, 'vqvae_copy_list', n, (C.c_void_p * n)(*[b['d%d' % i].ptr for i in range(n)]),
                                              (C.c_void_p * n)(*[b['s%d' % i].ptr for i in range(n)]), (C.c_size_t * n)(*counts)), specs)
        for i in range(n):
            np.testing.assert_array_equal(r['d%d' % i][:counts[i]], srcs[i][:counts[i]])


# --------------------------------------------------------------------------- #
# input / embed
# --------------------------------------------------------------------------- #
def test_input_pipeline_contract(gpu):
    from vqvae_amd.inputs import DeviceInputPipeline
    rs = _rs('input')
    for mu, n in ((256, 1), (256, 100003), (50, 255)):
        thr = _f32(DeviceInputPipeline(mu)._thr_host)
        x = _f32(rs.uniform(-1, 1, n))
        x[n - 1] = 1.0
        r = run_contract(gpu, lambda b: _call(gpu, 'vqvae_mulaw_bins', b.x.ptr, n, b.thr.ptr, thr.size, b.q.ptr),
                         dict(x=In(x), thr=In(thr), q=Out((n,), np.int32)))
        np.testing.assert_array_equal(r['q'], O.MuLaw(mu).transform(x))
    for B, q, T, pad in ((1, 1, 1, 0), (3, 50, 63, 5), (2, 256, 65, 0), (1, 1025, 7, 3)):
        idx = rs.randint(0, q, (B, T + pad)).astype(np.int32)
        idx[B - 1, T - 1] = q - 1
        r = run_contract(gpu, lambda b: _call(gpu, 'vqvae_onehot', b.idx.ptr, T + pad, B, q, T, b.out.ptr),
                         dict(idx=In(idx, index_range=(0, q)), out=Out((B, q, T))))
        np.testing.assert_array_equal(r['out'], np.identity(q, dtype=np.float32)[idx[:, :T]].transpose(0, 2, 1))


def _embed_ref(idx, W, b):
    """y[b, co, t] = b[co] + sum_tap W[co, idx[b, t - (K - 1 - tap)], tap] in float64 (taps before the row start: nothing)."""
    B, T = idx.shape
    Cout, q, K = W.shape
    y = np.tile(b.astype(np.float64)[None, :, None], (B, 1, T))
    for tap in range(K):
        sh = K - 1 - tap
        if sh < T:
            y[:, :, sh:] += W.astype(np.float64)[:, idx[:, :T - sh], tap].transpose(1, 0, 2)
    return y


EMBED_CASES = [
    # B, T, pad of the index rows, Cout, q, K, shift of idx, shift of y
    (1, 1, 0, 1, 50, 2, 0, 0),
    (3, 63, 0, 33, 50, 2, 0, 0),          # T % 4 != 0: the scalar kernel
    (2, 64, 4, 33, 256, 2, 0, 0),         # idx_bstride != T: the scalar kernel
    (2, 64, 0, 33, 256, 2, 0, 0),         # the 2 x 4 kernel
    (2, 64, 0, 33, 256, 2, 4, 0),         # idx shifted by 4 B: scalar
    (2, 64, 0, 33, 256, 2, 0, 4),         # y shifted by 4 B: scalar
    (2, 1028, 0, 5, 1025, 2, 0, 0),       # the LDS form (T >= 1024)
    (2, 68, 0, 7, 50, 1, 0, 0),           # K = 1
    (1, 5, 0, 3, 7, 3, 0, 0),             # K = 3
]


@pytest.mark.parametrize('case', EMBED_CASES, ids=lambda c: 'B%d_T%d_pad%d_Co%d_q%d_K%d_si%d_sy%d' % c)
def test_embed_gather_contract(gpu, case):
    B, T, pad, Cout, q, K, si, sy = case
    rs = _rs('embg', case)
    idx = rs.randint(0, q, (B, T + pad)).astype(np.int32)
    W = _f32(rs.standard_normal((Cout, q, K)))
    W[Cout - 1, q - 1, K - 1] = 64.0                          # the bound's maximum sits in the last class of the last channel
    b = _f32(rs.standard_normal(Cout))
    r = run_contract(gpu, lambda a: _call(gpu, 'vqvae_embed_gather_fwd', a.idx.ptr, T + pad, B, T, a.W.ptr, a.b.ptr, Cout, q, K, a.y.ptr),
                     dict(idx=In(idx, shift=si, index_range=(0, q)), W=In(W), b=In(b), y=Out((B, Cout, T), shift=sy)))
    assert_close(r['y'], _embed_ref(idx[:, :T], W, b), 1e-6, 'y')
    r2 = run_contract(gpu, lambda a: _call(gpu, 'vqvae_embed_gather_bound', a.W.ptr, a.b.ptr, Cout, q, K, a.words.ptr),
                      dict(W=In(W), b=In(b), words=Out((16,), np.uint32)))          # poisoned: the entry point sets the words itself
    bound = _amax_of(r2['words'])
    true = float((np.abs(b.astype(np.float64)) + np.abs(W.astype(np.float64)).max(axis=1).sum(axis=1)).max())
    assert bound >= true and bound >= float(np.abs(r['y']).max()) and bound <= true * 1.0011, (bound, true)


@pytest.mark.parametrize('B,Cout,q,K,T,sx', [(2, 33, 50, 2, 64, 0), (2, 33, 50, 2, 63, 0), (1, 5, 256, 2, 68, 4), (3, 4, 7, 3, 10, 0),
                                             (1, 3, 50, 2, 1028, 0)])
@pytest.mark.parametrize('onehot', [True, False])
def test_embed_onehot_contract(gpu, matmul_mode, B, Cout, q, K, T, sx, onehot):
    """The one-hot float input of the embed conv: device-side scan, gather form or dense conv, bincount or dense weight
    gradient, over the exactly-sized workspace (per-row histograms | sorted positions | dense conv)."""
    lib = _L().load()
    rs = _rs('embo', B, Cout, q, K, T, sx, onehot)
    idx = rs.randint(0, q, (B, T)).astype(np.int32)
    idx[B - 1, T - 1] = q - 1
    x = _f32(np.identity(q, dtype=np.float32)[idx].transpose(0, 2, 1))
    if not onehot:
        x[B - 1, q - 1, T - 1] = 0.5                          # the LAST column is not one-hot: the dense path
    W = _f32(rs.standard_normal((Cout, q, K)) / np.sqrt(q * K))
    b = _f32(rs.standard_normal(Cout))
    ws_bytes = lib.vqvae_embed_onehot_workspace_bytes(B, Cout, q, K, T)
    r = run_contract(gpu, lambda a: _call(gpu, 'vqvae_embed_onehot_fwd', a.x.ptr, a.W.ptr, a.b.ptr, B, Cout, q, K, T, a.y.ptr, a.idx.ptr,
                                          a.flag.ptr, a.ws.ptr, ws_bytes),
                     dict(x=In(x, shift=sx), W=In(W), b=In(b), y=Out((B, Cout, T)), idx=Out((B, T), np.int32), flag=Out((1,), np.int32),
                          ws=Ws(ws_bytes)))
    assert int(r['flag'][0]) == int(onehot)
    want = O.conv1d_fwd(x.astype(np.float64), W.astype(np.float64), b.astype(np.float64), 1, K - 1, 1)[:, :, :T]
    assert_close(r['y'], want, 1e-4, 'y')
    if onehot:
        np.testing.assert_array_equal(r['idx'], idx)
    gy = _f32(rs.standard_normal((B, Cout, T)))
    gfull = np.zeros((B, Cout, T + K - 1))
    gfull[:, :, :T] = gy
    _, gW64, gb64 = O.conv1d_bwd(x.astype(np.float64), W.astype(np.float64), gfull, 1, K - 1, 1)
    for acc in (0, 1):
        iW, ib = _f32(rs.standard_normal((Cout, q, K))), _f32(rs.standard_normal(Cout))
        r2 = run_contract(gpu, lambda a: _call(gpu, 'vqvae_embed_onehot_wgrad', a.x.ptr, a.idx.ptr, a.flag.ptr, a.gy.ptr, B, Cout, q, K, T,
                                               a.gW.ptr, a.gb.ptr, acc, a.ws.ptr, ws_bytes),
                          dict(x=In(x, shift=sx), idx=In(r['idx'], index_range=(0, q)), flag=In(r['flag']), gy=In(gy), ws=Ws(ws_bytes),
                               gW=Out(init=iW) if acc else Out((Cout, q, K)), gb=Out(init=ib) if acc else Out((Cout,))))
        assert_close_scaled(r2['gW'], gW64 + (iW if acc else 0), 1e-4 if not onehot else 1e-5, 'gW accumulate = %d' % acc)
        assert_close_scaled(r2['gb'], gb64 + (ib if acc else 0), 1e-4 if not onehot else 1e-5, 'gb accumulate = %d' % acc)


# --------------------------------------------------------------------------- #
# generic convolution
# --------------------------------------------------------------------------- #
CONV_CASES = [
    # B, Cin, Tin, Cout, K, stride, pad, dil, Tout (None: natural)
    (1, 1, 129, 1, 2, 1, 1, 1, 129),        # one channel each way, cropped causal
    (3, 3, 127, 33, 4, 2, 1, 1, None),      # stride 2 over an odd Tin -> Tout = 63
    (1, 48, 65, 257, 1, 1, 0, 1, None),     # Cout = 257: one row in the third 128-row tile
    (3, 130, 1000, 33, 2, 1, 3, 3, 1000),   # Tout = 1000, ragged channels both ways
    (2, 48, 5, 33, 3, 1, 8, 8, None),       # dilation above Tin
    (1, 3, 1, 33, 1, 1, 0, 1, None),        # Tout = 1
    (3, 48, 140, 33, 2, 1, 1, 1, 65),       # cropped well below the natural length
    (2, 1280, 120, 192, 1, 1, 0, 1, None),  # latent rate: the forward's split-K
    (2, 192, 120, 1280, 1, 1, 0, 1, None),  # ... and the backward-data's
]


def _conv_refs(mode, x, W, b, gy, stride, pad, dil, Tout, relu):
    """y, gx, gW, gb of the cropped conv: float64, or (bf16 operands) the oracle in its bf16 mode on float32."""
    f = (lambda a: a) if mode == 'bfloat16' else (lambda a: a.astype(np.float64))
    y = O.conv1d_fwd(f(x), f(W), f(b), stride, pad, dil)
    nat = y.shape[2]
    y = y[:, :, :Tout]
    g = gy * (y > 0) if relu else gy
    gfull = np.zeros((gy.shape[0], gy.shape[1], nat), y.dtype)
    gfull[:, :, :Tout] = g
    gx, gW, gb = O.conv1d_bwd(f(x), f(W), gfull, stride, pad, dil)
    return (np.maximum(y, 0) if relu else y), gx, gW, gb


def _conv_contract(gpu, mode, case):
    L = _L()
    lib = L.load()
    B, Cin, Tin, Cout, K, stride, pad, dil, Tout = case
    nat = O.conv_out_len(Tin, K, stride, pad, dil)
    Tout = nat if Tout is None else Tout
    rs = _rs('conv', case)
    x = _f32(rs.standard_normal((B, Cin, Tin)))
    W = _f32(rs.standard_normal((Cout, Cin, K)) / np.sqrt(Cin * K))
    b = _f32(rs.standard_normal(Cout))
    gy = _f32(rs.standard_normal((B, Cout, Tout)))
    for relu in (0, 1):
        d = L.Conv1dDesc(B, Cin, Tin, Cout, Tout, K, stride, pad, dil, relu)
        ws_bytes = lib.vqvae_conv1d_workspace_bytes(C.byref(d))
        y64, gx64, gW64, gb64 = _conv_refs(mode, x, W, b, gy, stride, pad, dil, Tout, relu)
        if relu:
            gy = gy.copy()
            gy[np.abs(y64) < 1e-5] = 0                       # a pre-activation within rounding of 0 may fall on either side
            y64, gx64, gW64, gb64 = _conv_refs(mode, x, W, b, gy, stride, pad, dil, Tout, relu)
        io = dict(x=In(x), W=In(W), b=In(b), ws=Ws(ws_bytes))
        r = run_contract(gpu, lambda a: _call(gpu, 'vqvae_conv1d_fwd', C.byref(d), a.x.ptr, a.W.ptr, a.b.ptr, a.y.ptr, a.ws.ptr, ws_bytes),
                         dict(io, y=Out((B, Cout, Tout))))
        assert_close(r['y'], y64, 1e-4, 'y relu = %d' % relu)

        def fwd_amax(a):
            am = L.Conv1dAmax(None, None, a.words.ptr, None)
            _call(gpu, 'vqvae_conv1d_fwd_amax', C.byref(d), a.x.ptr, a.W.ptr, a.b.ptr, a.y.ptr, a.ws.ptr, ws_bytes, C.byref(am))
        r2 = run_contract(gpu, fwd_amax, dict(io, y=Out((B, Cout, Tout)), words=Out(init=ZERO_WORDS)))
        np.testing.assert_array_equal(r2['y'], r['y'])
        assert int(r2['words'].max()) == _bits32(np.abs(r2['y']).max()), 'published max |y|'
        y_dev = r['y']
        # packed ahead == packed inline
        pk = lib.vqvae_conv1d_packed_bytes(C.byref(d), 0)
        if pk:
            def packed(a):
                _call(gpu, 'vqvae_conv1d_pack', 1, C.byref(d), (C.c_void_p * 1)(a.W.ptr), (C.c_int * 1)(0), (C.c_void_p * 1)(a.slab.ptr))
                am = L.Conv1dAmax(None, None, None, a.slab.ptr)
                _call(gpu, 'vqvae_conv1d_fwd_amax', C.byref(d), a.x.ptr, a.W.ptr, a.b.ptr, a.y.ptr, a.ws.ptr, ws_bytes, C.byref(am))
            r3 = run_contract(gpu, packed, dict(io, y=Out((B, Cout, Tout)), slab=Ws(pk)))
            np.testing.assert_array_equal(r3['y'], r['y'])
        if relu:
            # the backward of THIS conv sees gy already masked by its caller; what the library offers is the mask of the conv's
            # INPUT: x_relu = relu(x) as the producing layer left it
            xr = np.maximum(x, 0)
            _, gxr64, _, _ = _conv_refs(mode, xr, W, b, gy, stride, pad, dil, Tout, 0)
            d0 = L.Conv1dDesc(B, Cin, Tin, Cout, Tout, K, stride, pad, dil, 0)
            r = run_contract(gpu, lambda a: _call(gpu, 'vqvae_conv1d_bwd_data_relu', C.byref(d0), a.W.ptr, a.gy.ptr, a.xr.ptr, a.gx.ptr, a.ws.ptr,
                                                  ws_bytes, None),
                             dict(W=In(W), gy=In(gy), xr=In(xr), ws=Ws(ws_bytes), gx=Out((B, Cin, Tin))))
            assert_close_scaled(r['gx'], gxr64 * (xr > 0), 1e-4, 'gx through the input ReLU')
            continue
        gym = gy
        for acc in (0, 1):
            ix, iW, ib = _f32(rs.standard_normal(x.shape)), _f32(rs.standard_normal(W.shape)), _f32(rs.standard_normal(Cout))
            r = run_contract(gpu, lambda a: _call(gpu, 'vqvae_conv1d_bwd_data', C.byref(d), a.W.ptr, a.gy.ptr, a.gx.ptr, acc, a.ws.ptr, ws_bytes),
                             dict(W=In(W), gy=In(gym), ws=Ws(ws_bytes), gx=Out(init=ix) if acc else Out((B, Cin, Tin))))
            assert_close_scaled(r['gx'], gx64 + (ix if acc else 0), 1e-4, 'gx accumulate = %d' % acc)

            def bwd_amax(a):
                am = L.Conv1dAmax(None, None, a.words.ptr, None)
                _call(gpu, 'vqvae_conv1d_bwd_data_amax', C.byref(d), a.W.ptr, a.gy.ptr, a.gx.ptr, acc, a.ws.ptr, ws_bytes, C.byref(am))
            r2 = run_contract(gpu, bwd_amax, dict(W=In(W), gy=In(gym), ws=Ws(ws_bytes), words=Out(init=ZERO_WORDS),
                                                  gx=Out(init=ix) if acc else Out((B, Cin, Tin))))
            np.testing.assert_array_equal(r2['gx'], r['gx'])
            assert _amax_of(r2['words']) >= float(np.abs(r2['gx']).max()), 'published max |gx| accumulate = %d' % acc
            if not acc:
                assert int(r2['words'].max()) == _bits32(np.abs(r2['gx']).max()), 'published max |gx|'
            r = run_contract(gpu, lambda a: _call(gpu, 'vqvae_conv1d_bwd_weight', C.byref(d), a.x.ptr, a.gy.ptr, a.gW.ptr, a.gb.ptr, acc,
                                                  a.ws.ptr, ws_bytes),
                             dict(x=In(x), gy=In(gym), ws=Ws(ws_bytes), gW=Out(init=iW) if acc else Out(W.shape),
                                  gb=Out(init=ib) if acc else Out((Cout,))))
            assert_close_scaled(r['gW'], gW64 + (iW if acc else 0), 1e-4, 'gW accumulate = %d' % acc)
            assert_close_scaled(r['gb'], gb64 + (ib if acc else 0), 1e-4, 'gb accumulate = %d' % acc)

            def wgrad_amax(a):                               # gb = NULL, maxima handed in
                am = L.Conv1dAmax(a.ax.ptr, a.ag.ptr, None, None)
                _call(gpu, 'vqvae_conv1d_bwd_weight_amax', C.byref(d), a.x.ptr, a.gy.ptr, a.gW.ptr, None, acc, a.ws.ptr, ws_bytes, C.byref(am))
            ax, ag = ZERO_WORDS.copy(), ZERO_WORDS.copy()
            ax[3], ag[15] = _bits32(np.abs(x).max()), _bits32(np.abs(gym).max())
            r2 = run_contract(gpu, wgrad_amax, dict(x=In(x), gy=In(gym), ax=In(ax), ag=In(ag), ws=Ws(ws_bytes),
                                                    gW=Out(init=iW) if acc else Out(W.shape)))
            assert_close_scaled(r2['gW'], gW64 + (iW if acc else 0), 1e-4, 'gW with maxima handed in, gb = NULL')
    return y_dev


@pytest.mark.parametrize('case', CONV_CASES, ids=lambda c: 'B%d_Ci%d_T%d_Co%d_K%d_s%d_p%d_d%d_To%s' % c)
def test_conv1d_contract(gpu, matmul_mode, case):
    _conv_contract(gpu, matmul_mode, case)


@pytest.mark.parametrize('case', [CONV_CASES[1], CONV_CASES[2], CONV_CASES[3], CONV_CASES[7]],
                         ids=lambda c: 'B%d_Ci%d_T%d_Co%d_K%d_s%d_p%d_d%d_To%s' % c)
def test_conv1d_contract_bf16(gpu, bf16_mode, case):
    _conv_contract(gpu, 'bfloat16', case)


SPIKES = ['first', 'tail_column', 'last_channel', 'last_batch', 'last_all']


@pytest.mark.parametrize('mode', ['float32x2', 'float32x3', 'float32', 'bfloat16'])
@pytest.mark.parametrize('spike', SPIKES)
@pytest.mark.parametrize('relu', [0, 1])
def test_published_maximum_conv(gpu, mode, spike, relu):
    """Magnitudes ~1 everywhere except ONE output of 64x, placed where an epilogue is most likely to miss it; relu = 1 also
    plants a large NEGATIVE pre-activation, which must not be published.  The words then scale the operand of the
    consuming conv in float32x2 (an understated maximum overflows fp16 there)."""
    L = _L()
    lib = L.load()
    gpu.set_matmul_dtype(mode)
    gpu.set_f32x2_min_gflop(0.0)
    try:
        B, Cin, Tin, Cout, K = 3, 48, 1000, 161, 1          # Tout = 1000: a tail tile of 104 columns; 161 = 128 + 33 channels
        rs = _rs('pubmax', spike, relu)
        x = _f32(rs.uniform(-1, 1, (B, Cin, Tin)))
        W = _f32(rs.uniform(-1, 1, (Cout, Cin, K)) / Cin)    # |y| <= 1 + |b|
        b = _f32(rs.uniform(-0.5, 0.5, Cout))
        bb, co, t = {'first': (0, 0, 0), 'tail_column': (0, 5, Tin - 1), 'last_channel': (1, Cout - 1, 500),
                     'last_batch': (B - 1, 77, 901), 'last_all': (B - 1, Cout - 1, Tin - 1)}[spike]
        # one input element of batch item bb meets a weight that only channel co has: y[bb, co, t] ~ 64, nothing else moves
        c0 = 7
        W[:, c0, 0] *= np.float32(0.01)
        W[co, c0, 0] = np.float32(1.0 / Cin)
        x[bb, c0, t] = np.float32(64.0 * Cin)
        if relu:
            W[(co + 40) % Cout, c0, 0] = np.float32(-1.0 / Cin)       # a pre-activation of ~ -64: gone after the ReLU
        d = L.Conv1dDesc(B, Cin, Tin, Cout, Tin, K, 1, 0, 1, relu)
        ws_bytes = lib.vqvae_conv1d_workspace_bytes(C.byref(d))

        def fwd(a):
            am = L.Conv1dAmax(None, None, a.words.ptr, None)
            _call(gpu, 'vqvae_conv1d_fwd_amax', C.byref(d), a.x.ptr, a.W.ptr, a.b.ptr, a.y.ptr, a.ws.ptr, ws_bytes, C.byref(am))
        r = run_contract(gpu, fwd, dict(x=In(x), W=In(W), b=In(b), ws=Ws(ws_bytes), y=Out((B, Cout, Tin)), words=Out(init=ZERO_WORDS)))
        y = r['y']
        assert 60.0 < np.abs(y).max() < 70.0 and np.abs(y[bb, co, t]) == np.abs(y).max()
        assert np.sort(np.abs(y).reshape(-1))[-2] < 3.0, 'one spike only'
        assert int(r['words'].max()) == _bits32(np.abs(y).max()), (_amax_of(r['words']), np.abs(y).max())
        # the consumer: a 1x1 conv over y with the published words as max |x|, and its backward-data publishing max |gx|
        C2 = 33
        W2 = _f32(rs.standard_normal((C2, Cout, 1)) / np.sqrt(Cout))
        b2 = _f32(rs.standard_normal(C2))
        d2 = L.Conv1dDesc(B, Cout, Tin, C2, Tin, 1, 1, 0, 1, 0)
        ws2 = lib.vqvae_conv1d_workspace_bytes(C.byref(d2))

        def consume(a):
            am = L.Conv1dAmax(a.words.ptr, None, None, None)
            _call(gpu, 'vqvae_conv1d_fwd_amax', C.byref(d2), a.x.ptr, a.W.ptr, a.b.ptr, a.y.ptr, a.ws.ptr, ws2, C.byref(am))
        r2 = run_contract(gpu, consume, dict(x=In(y), words=In(r['words']), W=In(W2), b=In(b2), ws=Ws(ws2), y=Out((B, C2, Tin))))
        if mode == 'bfloat16':
            O.set_bf16(True)
            want = O.conv1d_fwd(y, W2, b2, 1, 0, 1)
            O.set_bf16(False)
        else:
            want = O.conv1d_fwd(y.astype(np.float64), W2.astype(np.float64), b2.astype(np.float64), 1, 0, 1)
        assert_close(r2['y'], want, 1e-4, 'consumer of the published maximum')
        gy2 = _f32(rs.uniform(-1, 1, (B, C2, Tin)))
        gy2[bb, C2 - 1, t] = 64.0

        def bwd(a):
            am = L.Conv1dAmax(None, None, a.words.ptr, None)
            _call(gpu, 'vqvae_conv1d_bwd_data_amax', C.byref(d2), a.W.ptr, a.gy.ptr, a.gx.ptr, 0, a.ws.ptr, ws2, C.byref(am))
        r3 = run_contract(gpu, bwd, dict(W=In(W2), gy=In(gy2), ws=Ws(ws2), gx=Out((B, Cout, Tin)), words=Out(init=ZERO_WORDS)))
        assert int(r3['words'].max()) == _bits32(np.abs(r3['gx']).max())
    finally:
        O.set_bf16(False)
        gpu.set_f32x2_min_gflop(8.0)
        gpu.set_matmul_dtype(gpu.default_matmul_dtype())


# --------------------------------------------------------------------------- #
# latent-rate fusions
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize('B,Cc,T,dils', [(1, 32, 1, (1,)), (3, 64, 128, (1, 2, 4, 8, 16)), (2, 32, 127, (16, 1, 3)), (1, 64, 5, (1, 2, 4, 8, 16, 1, 2, 4))])
def test_latent_fusions_contract(gpu, B, Cc, T, dils):
    L = _L()
    lib = L.load()
    nl = len(dils)
    cd = (C.c_int * nl)(*dils)
    assert lib.vqvae_convstack_supported(nl, Cc, T, cd) == 1
    rs = _rs('cstack', B, Cc, T, dils)
    x = _f32(rs.standard_normal((B, Cc, T)))
    Ws_ = [_f32(rs.standard_normal((Cc, Cc, 3)) / np.sqrt(3 * Cc)) for _ in dils]
    bs = [_f32(0.1 * rs.standard_normal(Cc)) for _ in dils]
    specs = dict(x=In(x))
    for l in range(nl):
        specs['W%d' % l], specs['b%d' % l], specs['h%d' % l] = In(Ws_[l]), In(bs[l]), Out((B, Cc, T))

    def pa(a, k):
        return (C.c_void_p * nl)(*[a['%s%d' % (k, l)].ptr for l in range(nl)])
    r = run_contract(gpu, lambda a: _call(gpu, 'vqvae_convstack_fwd', nl, B, Cc, T, cd, a.x.ptr, pa(a, 'W'), pa(a, 'b'), pa(a, 'h')), specs)
    h64 = [x.astype(np.float64)]
    for l in range(nl):
        h64.append(np.maximum(O.conv1d_fwd(h64[-1], Ws_[l].astype(np.float64), bs[l].astype(np.float64), 1, dils[l], dils[l]), 0))
        assert_close(r['h%d' % l], h64[-1], 1e-4, 'h%d' % l)
    hs = [r['h%d' % l] for l in range(nl)]
    gy = _f32(rs.standard_normal((B, Cc, T)))
    gy[np.abs(h64[-1]) < 1e-5] = 0
    g = gy.astype(np.float64)
    gW64, gb64 = [None] * nl, [None] * nl
    for l in reversed(range(nl)):
        g = g * (hs[l] > 0)
        g, gW64[l], gb64[l] = O.conv1d_bwd(h64[l], Ws_[l].astype(np.float64), g, 1, dils[l], dils[l])
    ws_bytes = lib.vqvae_convstack_workspace_bytes(nl, B, Cc)
    for acc in (0, 1):
        specs = dict(x=In(x), gy=In(gy), ws=Ws(ws_bytes), gx=Out((B, Cc, T)))
        init = {}
        for l in range(nl):
            init['gW%d' % l], init['gb%d' % l] = _f32(rs.standard_normal((Cc, Cc, 3))), _f32(rs.standard_normal(Cc))
            specs['W%d' % l], specs['h%d' % l] = In(Ws_[l]), In(hs[l])
            specs['gW%d' % l] = Out(init=init['gW%d' % l]) if acc else Out((Cc, Cc, 3))
            specs['gb%d' % l] = Out(init=init['gb%d' % l]) if acc else Out((Cc,))
        r = run_contract(gpu, lambda a: _call(gpu, 'vqvae_convstack_bwd', nl, B, Cc, T, cd, a.x.ptr, pa(a, 'W'), pa(a, 'h'), a.gy.ptr, a.gx.ptr,
                                              pa(a, 'gW'), pa(a, 'gb'), acc, a.ws.ptr, ws_bytes), specs)
        assert_close_scaled(r['gx'], g, 1e-4, 'gx')
        for l in range(nl):
            assert_close_scaled(r['gW%d' % l], gW64[l] + (init['gW%d' % l] if acc else 0), 1e-4, 'gW%d accumulate = %d' % (l, acc))
            assert_close_scaled(r['gb%d' % l], gb64[l] + (init['gb%d' % l] if acc else 0), 1e-4, 'gb%d accumulate = %d' % (l, acc))


@pytest.mark.parametrize('B,Tin,mask', [(1, 2, 0), (3, 127, 1), (2, 130, 1), (1, 961, 0)])
def test_conv_s2_bwd_contract(gpu, B, Tin, mask):
    lib = _L().load()
    Cc, K = 64, 4
    Tout = O.conv_out_len(Tin, K, 2, 1, 1)
    assert lib.vqvae_conv_s2_bwd_supported(Cc, Cc, K, 2, 1, 1, Tin, Tout) == 1
    rs = _rs('s2', B, Tin, mask)
    x = _f32(rs.standard_normal((B, Cc, Tin)))
    if mask:
        x = np.maximum(x, 0)
    W = _f32(rs.standard_normal((Cc, Cc, K)) / np.sqrt(Cc * K))
    gy = _f32(rs.standard_normal((B, Cc, Tout)))
    gx64, gW64, gb64 = O.conv1d_bwd(x.astype(np.float64), W.astype(np.float64), gy.astype(np.float64), 2, 1, 1)
    if mask:
        gx64 = gx64 * (x > 0)
    ws_bytes = lib.vqvae_conv_s2_bwd_workspace_bytes(B, Cc, Tin)
    for acc in (0, 1):
        iW, ib = _f32(rs.standard_normal(W.shape)), _f32(rs.standard_normal(Cc))
        r = run_contract(gpu, lambda a: _call(gpu, 'vqvae_conv_s2_bwd', B, Cc, Tin, Tout, a.x.ptr, a.W.ptr, a.gy.ptr, mask, a.gx.ptr, a.gW.ptr,
                                              a.gb.ptr, acc, a.ws.ptr, ws_bytes),
                         dict(x=In(x), W=In(W), gy=In(gy), ws=Ws(ws_bytes), gx=Out((B, Cc, Tin)),
                              gW=Out(init=iW) if acc else Out(W.shape), gb=Out(init=ib) if acc else Out((Cc,))))
        assert_close_scaled(r['gx'], gx64, 1e-4, 'gx')
        assert_close_scaled(r['gW'], gW64 + (iW if acc else 0), 1e-4, 'gW accumulate = %d' % acc)
        assert_close_scaled(r['gb'], gb64 + (ib if acc else 0), 1e-4, 'gb accumulate = %d' % acc)


# --------------------------------------------------------------------------- #
# vector quantiser
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize('B,T,k,d', [(1, 1, 16, 32), (1, 63, 512, 64), (3, 21, 16, 128), (1, 8193, 512, 64), (2, 1030, 8192, 128),
                                     (1, 8193, 16, 32)])
def test_vq_contract(gpu, matmul_mode, B, T, k, d):
    """Both search modes and the codebook gradient over the exactly-sized, poisoned workspace (the counters in it are
    initialised by the entry points: CONTRACTS); idx, the gathered codes and the re-check count are zoned outputs."""
    lib = _L().load()
    rs = _rs('vq', B, T, k, d)
    W = _f32(rs.standard_normal((k, d)))
    z = _f32(rs.standard_normal((B, d, T)))
    z[B - 1, :, T - 1] = W[k - 1] + np.float32(1e-3)          # the last row's answer is the last code
    ws_bytes = lib.vqvae_vq_workspace_bytes(B, d, T, k)
    out = {}
    for mode in (0, 1):
        out[mode] = run_contract(gpu, lambda a: _call(gpu, 'vqvae_vq_nearest_fwd', a.z.ptr, a.W.ptr, B, d, T, k, mode, a.idx.ptr, a.e.ptr, a.nre.ptr,
                                                       a.ws.ptr, ws_bytes),
                                 dict(z=In(z), W=In(W), ws=Ws(ws_bytes), idx=Out((B, T), np.int32), e=Out((B, d, T)), nre=Out((1,), np.int32)))
    idx = out[1]['idx']
    np.testing.assert_array_equal(out[0]['idx'], idx)
    assert idx[B - 1, T - 1] == k - 1 and idx.min() >= 0 and idx.max() < k
    rows = np.unique(np.concatenate([np.arange(min(256, B * T)), np.arange(max(B * T - 256, 0), B * T)]))
    zr, W64 = z.transpose(0, 2, 1).reshape(-1, d)[rows].astype(np.float64), W.astype(np.float64)
    dist = (zr ** 2).sum(1)[:, None] - 2 * zr @ W64.T + (W64 ** 2).sum(1)[None]
    assert (dist[np.arange(rows.size), idx.reshape(-1)[rows]] <= dist.min(axis=1) + 1e-5 * np.abs(dist).max()).all()
    for mode in (0, 1):
        np.testing.assert_array_equal(out[mode]['e'], W[idx].transpose(0, 2, 1))
    assert 0 <= int(out[0]['nre'][0]) <= B * T and int(out[1]['nre'][0]) == 0
    gy = _f32(rs.standard_normal((B, d, T)))
    want = np.zeros((k, d))
    np.add.at(want, idx.reshape(-1), gy.transpose(0, 2, 1).reshape(-1, d).astype(np.float64))
    for acc in (0, 1):
        iW = _f32(rs.standard_normal((k, d)))
        r = run_contract(gpu, lambda a: _call(gpu, 'vqvae_vq_grad_w', a.idx.ptr, a.gy.ptr, B, d, T, k, a.gW.ptr, acc, a.ws.ptr, ws_bytes),
                         dict(idx=In(idx, index_range=(0, k)), gy=In(gy), ws=Ws(ws_bytes), gW=Out(init=iW) if acc else Out((k, d))))
        assert_close_scaled(r['gW'], want + (iW if acc else 0), 1e-6, 'gW accumulate = %d' % acc)


# --------------------------------------------------------------------------- #
# residual block (unpacked entry points)
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize('B,T,dil', [(1, 128, 1), (3, 200, 64), (2, 100, 64), (1, 1000, 512)])
def test_resblock_unpacked_contract(gpu, matmul_mode, B, T, dil):
    """vqvae_resblock_fwd / _bwd / _wgrad with the full-rate condition: T above and below 2 dil, T not a multiple of 128,
    every optional output given, the workspace exactly as queried."""
    L = _L()
    lib = L.load()
    Cr, Cd, Cs, Cc, K = 96, 64, 33, 20, 2
    Ch = Cd // 2
    d = L.ResblockDesc(B, T, Cr, Cd, Cs, Cc, K, dil, 0)
    ws_bytes = lib.vqvae_resblock_workspace_bytes(C.byref(d))
    rs = _rs('rb', B, T, dil)
    P = dict(Wd=_f32(rs.standard_normal((Cd, Cr, K)) / np.sqrt(Cr * K)), bd=_f32(0.1 * rs.standard_normal(Cd)),
             Wc=_f32(rs.standard_normal((Cd, Cc, 1)) / np.sqrt(Cc)), bc=_f32(0.1 * rs.standard_normal(Cd)),
             Wr=_f32(rs.standard_normal((Cr, Ch, 1)) / np.sqrt(Ch)), br=_f32(0.1 * rs.standard_normal(Cr)),
             Ws=_f32(rs.standard_normal((Cs, Ch, 1)) / np.sqrt(Ch)), bs=_f32(0.1 * rs.standard_normal(Cs)))
    x, cond = _f32(rs.standard_normal((B, Cr, T))), _f32(rs.standard_normal((B, Cc, T)))
    f64 = lambda a: a.astype(np.float64)
    h = O.conv1d_fwd(f64(x), f64(P['Wd']), f64(P['bd']), 1, dil * (K - 1), dil)[:, :, :T] + O.conv1d_fwd(f64(cond), f64(P['Wc']), f64(P['bc']))
    ta, sg = np.tanh(h[:, :Ch]), 1 / (1 + np.exp(-h[:, Ch:]))
    z64 = ta * sg
    res64 = O.conv1d_fwd(z64, f64(P['Wr']), f64(P['br'])) + x
    skip64 = O.conv1d_fwd(z64, f64(P['Ws']), f64(P['bs']))
    pin = dict((k, In(v)) for k, v in P.items())

    def params(a):
        return L.ResblockParams(*[a[k].ptr for k in ('Wd', 'bd', 'Wc', 'bc', 'Wr', 'br', 'Ws', 'bs')])
    skip0 = _f32(rs.standard_normal((B, Cs, T)))
    r = run_contract(gpu, lambda a: _call(gpu, 'vqvae_resblock_fwd', C.byref(d), C.byref(params(a)), a.x.ptr, a.cond.ptr, None, a.res.ptr, a.skip.ptr, 1,
                                          a.gates.ptr, a.z.ptr, a.ws.ptr, ws_bytes),
                     dict(pin, x=In(x), cond=In(cond), ws=Ws(ws_bytes), res=Out((B, Cr, T)), skip=Out(init=skip0), gates=Out((B, Cd, T)),
                          z=Out((B, Ch, T))))
    assert_close(r['res'], res64, 1e-4, 'res')
    assert_close(r['skip'], skip64 + skip0, 1e-4, 'skip (accumulated)')
    assert_close(r['gates'], np.concatenate([ta, sg], 1), 1e-4, 'gates')
    gates, z = r['gates'], r['z']
    g_res, g_skip = _f32(rs.standard_normal((B, Cr, T))), _f32(rs.standard_normal((B, Cs, T)))
    gz = np.einsum('oc,bot->bct', f64(P['Wr'][:, :, 0]), f64(g_res)) + np.einsum('oc,bot->bct', f64(P['Ws'][:, :, 0]), f64(g_skip))
    gh64 = np.concatenate([gz * sg * (1 - ta * ta), gz * ta * sg * (1 - sg)], 1)
    gfull = np.zeros((B, Cd, T + dil * (K - 1)))
    gfull[:, :, :T] = gh64
    gxd, gWd64, gbd64 = O.conv1d_bwd(f64(x), f64(P['Wd']), gfull, 1, dil * (K - 1), dil)
    gcond64, gWc64, gbc64 = O.conv1d_bwd(f64(cond), f64(P['Wc']), gh64)
    _, gWr64, gbr64 = O.conv1d_bwd(z64, f64(P['Wr']), f64(g_res))
    _, gWs64, gbs64 = O.conv1d_bwd(z64, f64(P['Ws']), f64(g_skip))
    gnames = ('gWd', 'gbd', 'gWc', 'gbc', 'gWr', 'gbr', 'gWs', 'gbs')
    gouts = dict((g, Out(P[g[1:]].shape)) for g in gnames)
    r = run_contract(gpu, lambda a: _call(gpu, 'vqvae_resblock_bwd', C.byref(d), C.byref(params(a)), a.x.ptr, a.cond.ptr, a.gates.ptr, a.z.ptr,
                                          a.g_res.ptr, a.g_skip.ptr, a.gx.ptr, a.gcond.ptr, 0, a.gh.ptr,
                                          C.byref(L.ResblockGrads(*[a[g].ptr for g in gnames])), 0, a.ws.ptr, ws_bytes),
                     dict(pin, x=In(x), cond=In(cond), gates=In(gates), z=In(z), g_res=In(g_res), g_skip=In(g_skip), ws=Ws(ws_bytes),
                          gx=Out((B, Cr, T)), gcond=Out((B, Cc, T)), gh=Out((B, Cd, T)), **gouts))
    assert_close_scaled(r['gh'], gh64, 1e-4, 'gh')
    assert_close_scaled(r['gx'], gxd + g_res, 1e-4, 'gx')
    assert_close_scaled(r['gcond'], gcond64, 1e-4, 'gcond')
    for g, want in zip(gnames, (gWd64, gbd64, gWc64, gbc64, gWr64, gbr64, gWs64, gbs64)):
        assert_close_scaled(r[g], want, 1e-4, g)
    gh = r['gh']
    for acc in (0, 1):
        iW, ib = _f32(rs.standard_normal(P['Wd'].shape)), _f32(rs.standard_normal(Cd))
        r = run_contract(gpu, lambda a: _call(gpu, 'vqvae_resblock_wgrad', C.byref(d), a.x.ptr, a.gh.ptr, a.gWd.ptr, a.gbd.ptr, acc, a.ws.ptr, ws_bytes),
                         dict(x=In(x), gh=In(gh), ws=Ws(ws_bytes), gWd=Out(init=iW) if acc else Out(iW.shape), gbd=Out(init=ib) if acc else Out((Cd,))))
        assert_close_scaled(r['gWd'], gWd64 + (iW if acc else 0), 1e-4, 'gWd accumulate = %d' % acc)
        assert_close_scaled(r['gbd'], gbd64 + (ib if acc else 0), 1e-4, 'gbd accumulate = %d' % acc)
