"""CPU checks of time alignment (vqvae_amd.alignment, include/vqvae_align.h): the two NumPy restatements of the rule
against each other and against answers known by construction, the host side of the rule (chunk plan, refusals), and what
is this header's own in the registry of vqvae_amd/_lib.py -- its literal names, structs and limits, the workspace
queries and the source's place in the Makefile; the table against the header text, the library and the compiler's layout
is tests/test_host_abi.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import abi_headers as A
import alignment_ref as R

HEADER = 'vqvae_align.h'
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (5, 9), (9, 5), (64, 64), (63, 65), (40, 33)]
N_MELS, N_MCEP = 12, 5


def _cfg(**kw):
    from vqvae_amd.metrics import MelConfig
    a = dict(sr=16000, n_fft=64, hop=16, n_mels=N_MELS, n_mcep=N_MCEP)
    a.update(kw)
    return MelConfig(**a)


def _dct():
    from vqvae_amd.metrics import tables
    return tables(_cfg())[2]


def _log_mel(F, seed, coarse=False):
    """(n_mels, F) float32; ``coarse``: every column is one of three, so the local cost takes four values (zero among
    them) and many candidates of the recurrence tie exactly."""
    rs = np.random.RandomState(seed)
    if coarse:
        return (np.random.RandomState(0).standard_normal((N_MELS, 3)) - 5.0).astype(np.float32)[:, rs.randint(0, 3, F)]
    return (rs.standard_normal((N_MELS, F)) - 5.0).astype(np.float32)


def _same_result(p, q):
    return (np.array_equal(np.float64(p[0]).view(np.uint64), np.float64(q[0]).view(np.uint64)) and p[1:3] == q[1:3] and
            np.array_equal(p[3], q[3]) and np.array_equal(p[4], q[4]) and p[3].dtype == q[3].dtype == np.int32)


def _valid(ia, ib, Fa, Fb):
    steps = set(zip(np.diff(ia).tolist(), np.diff(ib).tolist()))
    return (ia[0], ib[0]) == (0, 0) and (ia[-1], ib[-1]) == (Fa - 1, Fb - 1) and steps <= {(1, 1), (1, 0), (0, 1)}


# ---- the restatement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('coarse', [False, True], ids=['noise', 'ties'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_the_two_restatements_agree_in_every_bit(shape, coarse):
    Fa, Fb = shape
    dct = _dct()
    d = R.local_cost(R.cepstra(_log_mel(Fa, 1, coarse), dct), R.cepstra(_log_mel(Fb, 2, coarse), dct))
    assert d.shape == shape and d.dtype == np.float64
    loops, diagonals = R.dtw_loops(d), R.dtw_diagonals(d)
    assert _same_result(loops, diagonals), (loops, diagonals)
    cost, K, G, ia, ib = loops
    assert _valid(ia, ib, Fa, Fb) and len(ia) == len(ib) == K and max(Fa, Fb) <= K <= Fa + Fb - 1
    assert G == sum(1 for s in zip(np.diff(ia), np.diff(ib)) if s == (1, 1))
    assert np.float64(R.path_sum(d, ia, ib)).view(np.uint64) == np.float64(cost).view(np.uint64)
    if coarse and min(shape) >= 5:
        assert 0 < (d == 0).sum() < d.size and len(np.unique(d)) <= 4             # the ties are there


def test_cepstra_and_the_local_cost_are_the_written_sums():
    dct = _dct()
    la, lb = _log_mel(4, 5), _log_mel(3, 6)
    ca, cb = R.cepstra(la, dct), R.cepstra(lb, dct)
    assert ca.shape == (4, N_MCEP) and ca.dtype == np.float64
    for f in range(4):
        for q in range(N_MCEP):
            c = 0.0
            for m in range(N_MELS):
                c += float(dct[q, m]) * float(la[m, f])
            assert c == ca[f, q]
    d = R.local_cost(ca, cb)
    for i in range(4):
        for j in range(3):
            s = 0.0
            for q in range(N_MCEP):
                h = 0.5 * (ca[i, q] - cb[j, q])
                s += h * h
            assert d[i, j] == R.C_DB * np.sqrt(2.0 * s)
    assert R.C_DB == 10.0 / np.log(10.0)


def test_repeated_columns_give_the_repetition_map():
    dct = _dct()
    a = _log_mel(9, 7)
    assert all((a[:, i] != a[:, i + 1]).any() for i in range(8))
    reps = [1, 3, 1, 2, 1, 1, 4, 1, 2]
    src = np.repeat(np.arange(9), reps)
    b = a[:, src]
    r = R.align(a, b, dct, R.dtw_loops)
    assert r['cost'] == 0.0 and r['path_len'] == b.shape[1] == 16 and r['mcd_dtw_db'] == 0.0 and r['log_mel_mae_dtw'] == 0.0
    assert r['ia'].tolist() == src.tolist() and r['ib'].tolist() == list(range(16)) and r['diagonal_steps'] == 8
    t = R.align(b, a, dct)                                       # the repeated side first: the transposed map
    assert t['cost'] == 0.0 and t['ia'].tolist() == list(range(16)) and t['ib'].tolist() == src.tolist()


@pytest.mark.parametrize('shape', [(3, 7), (7, 3), (4, 4), (1, 5), (5, 1)], ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('level', [0.0, 1.5], ids=['zero_cost', 'equal_cost'])
def test_all_equal_costs_give_the_tie_break_path(shape, level):
    Fa, Fb = shape
    dct = _dct()
    ramp = np.linspace(-3, 1, N_MELS).astype(np.float32)[:, None]
    a = np.repeat(ramp, Fa, axis=1)
    b = np.repeat(ramp * np.float32(1.0 + level), Fb, axis=1)
    for dtw in (R.dtw_loops, R.dtw_diagonals):
        r = R.align(a, b, dct, dtw)
        assert len(np.unique(r['d'])) == 1 and (r['d'][0, 0] == 0.0) == (level == 0.0)
        ia, ib = R.tie_break_path(Fa, Fb)
        assert r['ia'].tolist() == ia.tolist() and r['ib'].tolist() == ib.tolist()
        assert r['path_len'] == max(Fa, Fb) and r['diagonal_steps'] == min(Fa, Fb) - 1
    assert [x.tolist() for x in R.tie_break_path(3, 7)] == [[0, 0, 0, 0, 0, 1, 2], [0, 1, 2, 3, 4, 5, 6]]
    assert [x.tolist() for x in R.tie_break_path(7, 3)] == [[0, 1, 2, 3, 4, 5, 6], [0, 0, 0, 0, 0, 1, 2]]


@pytest.mark.parametrize('F', [1, 2, 17, 64])
def test_equal_lengths_cost_no_more_than_the_diagonal(F):
    dct = _dct()
    r = R.align(_log_mel(F, 11), _log_mel(F, 12), dct)
    diagonal = R.path_sum(r['d'], np.arange(F), np.arange(F))
    assert r['cost'] <= diagonal
    same = R.align(_log_mel(F, 11), _log_mel(F, 11), dct)
    assert same['cost'] == 0.0 and same['ia'].tolist() == same['ib'].tolist() == list(range(F))


def test_the_along_path_reduce_order():
    v = np.arange(1, 601, dtype=np.float64)
    assert R.reduce_order(v) == v.sum()
    big = np.array([1e16, 1.0, -1e16, 1.0] * 64 + [1.0])
    s = [big[t::256].tolist() for t in range(256)]
    s = [x[0] + x[1] if len(x) == 2 else x[0] for x in s]
    h = 128
    while h:
        s = [s[k] + s[k + h] for k in range(h)]
        h //= 2
    assert R.reduce_order(big) == s[0]
    la, lb = _log_mel(30, 3), _log_mel(41, 4)
    r = R.align(la, lb, _dct())
    terms = [abs(float(la[m, i]) - float(lb[m, j])) for i, j in zip(r['ia'], r['ib']) for m in range(N_MELS)]
    assert r['log_mel_mae_dtw'] == R.reduce_order(terms) / (r['path_len'] * N_MELS)


# ---- the chunk plan, the refusals ----------------------------------------------------------------------------------------------
def test_the_chunk_plan():
    from vqvae_amd import alignment
    fa, fb = [10, 20, 30], [10, 20, 30]                     # 100, 400, 900 direction bytes
    assert alignment.plan_chunks(fa, fb, 1 << 30) == [(0, 3)]
    assert alignment.plan_chunks(fa, fb, 1) == [(0, 1), (1, 2), (2, 3)]
    assert alignment.plan_chunks(fa, fb, 500) == [(0, 2), (2, 3)]
    assert alignment.plan_chunks(fa, fb, 499) == [(0, 1), (1, 2), (2, 3)]
    assert alignment.plan_chunks([3, 1], [1, 2], 4) == [(0, 1), (1, 2)]      # cells are counted four to a float32 element, rounded up per pair
    with pytest.raises(ValueError, match='chunk_bytes must be positive'):
        alignment.plan_chunks(fa, fb, 0)


def _described(frames, cfg=None):
    from vqvae_amd.metrics import RaggedFeatures
    return RaggedFeatures(cfg or _cfg(), frames, None, None)


def test_every_refusal_names_its_reason():
    import vqvae_amd as V
    from vqvae_amd import alignment
    M = alignment.MAX_SHORT
    assert M == 3072 >= 2048 and 48 * M <= 160 * 1024 < 48 * (M + 1024)
    with pytest.raises(TypeError, match='feats_b must be a metrics.RaggedFeatures'):
        V.align_many(_described([3]), np.zeros((12, 3), np.float32))
    with pytest.raises(ValueError, match='analysed differently'):
        V.align_many(_described([3]), _described([3], _cfg(n_mcep=6)))
    with pytest.raises(ValueError, match='2 utterances on side a and 3 on side b'):
        V.align_many(_described([3, 4]), _described([3, 4, 5]))
    with pytest.raises(ValueError, match='pair 1 has %d and 4000 frames; the shorter side may have at most %d' % (M + 1, M)):
        V.align_many(_described([5, M + 1]), _described([9, 4000]))
    with pytest.raises(ValueError, match='pair 2 has 2 x 1073741825 = 2147483650 cells; .* at most 2\\^31'):
        V.align_many(_described([5, 5, 2]), _described([9, 9, (1 << 30) + 1]))
    with pytest.raises(ValueError, match='chunk_bytes must be positive'):
        V.align_many(_described([5]), _described([9]), chunk_bytes=0)
    # at the bounds nothing is refused by the host rule: the call gets as far as asking for the features themselves
    with pytest.raises(ValueError, match='description only'):
        V.align_many(_described([M, 1 << 10]), _described([M + 7, 1 << 21]))
    cfg = _cfg(hop=1)
    long_ = np.zeros(64 + M, np.float32)                    # M + 1 frames at hop 1
    with pytest.raises(ValueError, match='compare_aligned_many: pair 1 has %d and %d frames' % (M + 1, M + 1)):
        V.compare_aligned_many([np.zeros(80, np.float32), long_], [np.zeros(90, np.float32), long_], cfg)
    with pytest.raises(ValueError, match='2 reference and 1 test utterances'):
        V.compare_aligned_many([long_, long_], [long_], cfg)
    with pytest.raises(ValueError, match='utterance 0 has 10 samples'):
        V.compare_aligned_many([np.zeros(10, np.float32)], [long_], cfg)
    with pytest.raises(TypeError, match='MelConfig'):
        V.compare_aligned_many([long_], [long_], None)
    al = V.Alignment(np.zeros(1), np.zeros(1), np.zeros(1), np.ones(1, np.int64), np.zeros(1, np.int64), np.ones(1, np.int64), np.ones(1, np.int64))
    with pytest.raises(ValueError, match='without paths=True'):
        al.utterance(0)
    with pytest.raises(IndexError):
        al.utterance(1)


# ---- the header, the table -----------------------------------------------------------------------------------------------------
NAMES = {'vqvae_align_abi_version', 'vqvae_align_cepstra_workspace_bytes', 'vqvae_align_dtw_workspace_bytes',
         'vqvae_align_path_workspace_bytes', 'vqvae_align_cepstra', 'vqvae_align_dtw', 'vqvae_align_path'}


def test_the_header_is_in_the_registry_and_alignment_binds_nothing():
    from vqvae_amd import _lib, alignment
    h = _lib.HEADERS[HEADER]                                   # against the header and the library: tests/test_host_abi.py
    assert set(h.prototypes) == NAMES and len(NAMES) == 7 and h.words == 'alignment ABI' and h.version == 1
    assert HEADER in os.listdir(A.INCLUDE) and not any('abi_version' in open(os.path.join(A.CSRC, f)).read() for f in os.listdir(A.CSRC) if f.endswith('.h'))
    assert set(A.structs(HEADER)) == {'vqvae_align_desc', 'vqvae_align_tables'}
    assert (_lib.AlignDesc._c_name_, _lib.AlignTables._c_name_) == ('vqvae_align_desc', 'vqvae_align_tables')
    assert [f for f, _ in _lib.AlignDesc._fields_] == ['n', 'n_mels', 'n_mcep', 'max_short', 'fa_tot', 'fb_tot', 'stride_a', 'stride_b',
                                                       'cells', 'ptot']
    assert [f for f, _ in _lib.AlignTables._fields_] == ['off_a', 'off_b', 'cell_off', 'path_off']
    assert sorted(A.macros(HEADER)) == ['VQVAE_ALIGN_MAX_MELS', 'VQVAE_ALIGN_MAX_SHORT', 'VQVAE_ALIGN_REDUCE_LANES', 'VQVAE_ALIGN_THREADS']
    assert (_lib.ALIGN_MAX_SHORT, _lib.ALIGN_MAX_MELS, _lib.ALIGN_THREADS, _lib.ALIGN_REDUCE_LANES) == (3072, 128, 256, 256)
    assert (alignment.MAX_SHORT, alignment.MAX_MELS, alignment.THREADS, alignment.REDUCE_LANES) == (3072, 128, 256, 256)
    assert R.LANES == alignment.REDUCE_LANES and _lib.ALIGN_MAX_MELS == _lib.METRICS_MAX_MELS
    for name in ('HEADER', 'ABI_WORDS', 'ABI_VERSION', 'PROTOTYPES', 'STRUCTS', '_bound', 'load', 'call', 'AlignDesc', 'AlignTables'):
        assert not hasattr(alignment, name), name


def test_the_source_is_built_and_depends_on_its_header():
    srcs = re.search(r'^SRCS\s*:?=\s*(.*)$', A.make_database(), flags=re.M).group(1).split()
    assert 'audio_align.hip' in srcs
    assert HEADER in [os.path.basename(p) for p in A.object_rule_prerequisites()]


def test_the_workspace_queries_refuse_what_the_entry_points_refuse():
    from vqvae_amd import _lib, alignment
    lib = _lib.load()
    fa, fb = np.array([5, 9], np.int64), np.array([7, 3], np.int64)
    good = alignment._desc(_cfg(), fa, fb, 14, 10)
    assert (good.max_short, good.cells, good.ptot) == (5, 35 + 27, 11 + 11)
    assert lib.vqvae_align_cepstra_workspace_bytes(C.byref(good)) == 0
    assert lib.vqvae_align_dtw_workspace_bytes(C.byref(good)) == 256            # 62 direction bytes, to the pool's granule
    assert lib.vqvae_align_path_workspace_bytes(C.byref(good)) == 256           # 2 * 4 * 22
    refused = C.c_size_t(-1).value
    for field, value in (('n', 0), ('n_mels', 129), ('n_mcep', N_MELS), ('n_mcep', 0), ('max_short', 0),
                         ('max_short', alignment.MAX_SHORT + 1), ('fa_tot', 1), ('stride_b', 9), ('cells', 1), ('ptot', 0)):
        bad = alignment._desc(_cfg(), fa, fb, 14, 10)
        setattr(bad, field, value)
        for q in ('vqvae_align_cepstra_workspace_bytes', 'vqvae_align_dtw_workspace_bytes', 'vqvae_align_path_workspace_bytes'):
            assert getattr(lib, q)(C.byref(bad)) == refused, (field, value, q)


def test_the_package_exports_the_calls():
    import vqvae_amd as V
    from vqvae_amd import alignment
    assert V.align_many is alignment.align_many and V.compare_aligned_many is alignment.compare_aligned_many
    assert V.Alignment is alignment.Alignment
