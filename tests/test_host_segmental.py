"""CPU checks of the segmental module (vqvae_amd.segmental, csrc/segmental.h): the NumPy restatement of the rule
(tests/segmental_ref.py) against the objective it must minimise (a brute force over all k^T paths) and against a second,
independent statement (a textbook Viterbi over the full k x k transition matrix); answers known by construction; exact
ties; every refusal; and the binding of the header that segmental.py carries itself -- the declared functions, parameter
counts, the descriptor's layout as a C99 compiler sees it, the revision error, the source's place in the Makefile.

The only bar here is the brute force's: its objective is summed in path order, the recursion's in time order, so the two
minima are compared at 1e-12 relative (T <= 5 additions of numbers of one sign: a few ulp of 2.2e-16); everything else is
an equality.  The device is not involved."""
import ctypes as C
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

import abi_headers as A
import segmental_ref as R

HEADER = os.path.join(A.CSRC, 'segmental.h')
OBJECTIVE_BAR = 1e-12


def _gauss(d, k, T, seed):
    rs = np.random.default_rng(seed)
    return rs.standard_normal((d, T)).astype(np.float32), rs.standard_normal((k, d)).astype(np.float32)


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def test_the_restatement_minimises_the_objective():
    """200 random cases, T <= 5, k <= 3: the recursion's path is the brute force's, its cost the brute force's minimum."""
    rs = np.random.RandomState(0)
    worst = 0.0
    for case in range(200):
        T, k, d = rs.randint(1, 6), rs.randint(1, 4), rs.randint(1, 4)
        z, W = rs.standard_normal((d, T)).astype(np.float32), rs.standard_normal((k, d)).astype(np.float32)
        lam = [0.0, 0.3, 1.0, 3.0, 30.0][case % 5]
        D = R.distances(z, W)
        codes, n_seg, cost = R.viterbi(D, lam)
        path, best = R.brute_force(D, lam)
        worst = max(worst, abs(cost - best) / max(best, 1e-300))
        assert abs(cost - best) <= OBJECTIVE_BAR * best, (case, cost, best)
        assert abs(R.path_cost(D, codes, lam) - best) <= OBJECTIVE_BAR * best, case
        assert np.array_equal(codes, path), (case, codes, path)         # continuous data: the minimiser is unique
        assert n_seg == 1 + np.count_nonzero(codes[1:] != codes[:-1]) and codes.dtype == np.int32
    print('objective %.3g' % worst)


def test_the_restatement_equals_the_textbook_viterbi():
    for seed, (d, k, T) in enumerate([(3, 2, 40), (8, 16, 300), (5, 33, 120), (2, 1, 9)]):
        z, W = _gauss(d, k, T, seed)
        D = R.distances(z, W)
        for lam in (0.0, d / 8.0, float(d), 1e3 * d):
            codes, n_seg, cost = R.viterbi(D, lam)
            full_codes, full_cost = R.viterbi_full(D, lam)
            assert cost == full_cost and np.array_equal(codes, full_codes), (d, k, T, lam)


def test_the_table_is_the_sum_in_ascending_j():
    z, W = _gauss(5, 4, 7, 11)
    D = R.distances(z, W)
    for t in range(7):
        for c in range(4):
            acc = np.float64(0.0)
            for j in range(5):
                diff = np.float64(z[j, t]) - np.float64(W[c, j])
                acc = acc + diff * diff
            assert D[t, c] == acc
    assert D.dtype == np.float64 and D.shape == (7, 4)


# ---- by construction -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d,k,T', [(8, 16, 300), (64, 128, 2000)])
def test_the_two_ends_and_the_way_between(d, k, T):
    z, W = _gauss(d, k, T, 0)
    D = R.distances(z, W)
    codes, n_seg, cost = R.viterbi(D, 0.0)
    nearest = D.argmin(axis=1)
    assert np.array_equal(codes, nearest) and cost == np.add.accumulate(D[np.arange(T), nearest])[-1]
    huge = float(D.max(axis=1).sum()) * 2.0                              # above the largest possible saving
    codes, n_seg, cost = R.viterbi(D, huge)
    sums = np.zeros(k)
    for t in range(T):                                                   # V of a path that never switches, in time order
        sums = sums + D[t]
    assert n_seg == 1 and (codes == int(np.argmin(sums))).all() and cost == sums.min()
    penalties = [0.0, d / 64.0, d / 8.0, d / 2.0, float(d), 4.0 * d, 64.0 * d, huge]
    counts = [R.viterbi(D, lam)[1] for lam in penalties]
    print('segments along %r: %r' % (penalties, counts))
    assert all(a >= b for a, b in zip(counts, counts[1:])) and counts[0] > counts[3] > counts[-1] == 1


def test_a_planted_segmentation_is_recovered():
    runs = [(2, 1), (0, 63), (3, 64), (1, 65), (0, 200), (2, 1), (3, 5)]
    W, z, want = R.planted(4, 8, runs, spacing=4.0, noise=0.05, seed=3)
    for lam in (0.5, 2.0):                                               # between the noise (8 * 0.05^2) and the spacing (2 * 4^2)
        codes, n_seg, cost = R.viterbi(R.distances(z, W), lam)
        assert np.array_equal(codes, want) and n_seg == len(runs)


# ---- exact ties ----------------------------------------------------------------------------------------------------------------
def _ints(rows):
    return np.array(rows, np.float32)


def test_ties_stay_and_then_take_the_lowest_index():
    """Integer-valued latents and a codebook with duplicated rows: D is exact, so the ties are."""
    W = _ints([[1], [1], [3]])                                           # codes 0 and 1 are the same point
    D = R.distances(_ints([[1, 3, 2]]), W)
    assert D.tolist() == [[0, 0, 4], [4, 4, 0], [1, 1, 1]]
    codes, n_seg, cost = R.viterbi(D, 0.0)                               # the last frame ties three ways: the lowest index
    assert (codes.tolist(), n_seg, cost) == ([0, 2, 0], 3, 1.0)
    W2 = _ints([[0], [2]])
    D2 = R.distances(_ints([[2, 0]]), W2)                                # V[0] = [4, 0]; lam = 4: V[0, 0] == sw
    codes, n_seg, cost = R.viterbi(D2, 4.0)
    assert (codes.tolist(), n_seg, cost) == ([0, 0], 1, 4.0)             # staying in 0 ties with [1, 0]: it stays
    assert R.path_cost(D2, [1, 0], 4.0) == 4.0 == R.path_cost(D2, [0, 0], 4.0)
    codes, n_seg, cost = R.viterbi(D2, 3.0)
    assert (codes.tolist(), n_seg, cost) == ([1, 0], 2, 3.0)
    rs = np.random.RandomState(5)
    for case in range(60):                                               # the objective, exactly: integers sum exactly
        T, lam = rs.randint(1, 6), float(rs.randint(0, 4))
        Wt = _ints(rs.randint(0, 3, (3, 2)))
        Wt[2] = Wt[0]
        Dt = R.distances(_ints(rs.randint(0, 3, (2, T))), Wt)
        codes, n_seg, cost = R.viterbi(Dt, lam)
        assert cost == R.brute_force(Dt, lam)[1] == R.path_cost(Dt, codes, lam), case
        assert 2 not in codes.tolist()                                   # row 2 duplicates row 0: the lower index wins
        full_codes, full_cost = R.viterbi_full(Dt, lam)
        assert full_cost == cost and np.array_equal(full_codes, codes), case


TIE_W, TIE_Z = R.TIE_W, R.TIE_Z


def test_the_shared_tie_case_by_hand():
    """The case tests/test_gpu_segmental.py runs on the device too."""
    got = R.segment(TIE_Z, TIE_W, [0.0, 1.0, 2.0])
    # penalty 0, from the last frame back: (3, 0) is code 2; (1, 2) is code 4; (1, 1) ties codes 0 and 4 and (2, 1) ties all
    # of them, so the walk STAYS in 4; (2, 0) ties 0 and 2 but not 4: the lowest; (3, 0) is 2; (1, 0) is 0
    assert [g[0].tolist() for g in got[0]] == [[0, 2, 0, 4, 4, 4, 2], [0], [0, 0, 0, 0]]
    for p, lam in enumerate([0.0, 1.0, 2.0]):
        for (codes, n_seg, cost), z in zip(got[p], TIE_Z):
            D = R.distances(z, TIE_W)
            if z.shape[1] <= 5:
                assert cost == R.brute_force(D, lam)[1]
            assert cost == R.path_cost(D, codes, lam) and not {1, 3} & set(codes.tolist())      # never the duplicate above


# ---- the refusals ----------------------------------------------------------------------------------------------------------------
def _fake_vq(k, d, dtype=np.float32):
    """A codebook that is on the device as far as the checks can tell; every call below is refused before it is read."""
    from vqvae_amd.backend import DeviceArray
    return types.SimpleNamespace(W=types.SimpleNamespace(data=DeviceArray((k, d), dtype, _block=object(), _ptr=256)))


def test_every_refusal_names_its_reason():
    import vqvae_amd as V
    from vqvae_amd import segmental
    vq = _fake_vq(16, 8)
    z = [np.zeros((8, 5), np.float32)]
    for penalties, words in (([-1.0], 'penalty 0 is -1.0; every penalty must be finite and not negative'),
                             ([0.0, float('nan')], 'penalty 1 is nan'), (float('inf'), 'penalty 0 is inf'),
                             ([], 'the penalty list is empty'), ([1.0] * 17, '17 penalties in one call; at most MAX_PEN = 16'),
                             ([[1.0], [2.0]], 'a flat list of numbers'), ('much', 'must be a number or a list of numbers')):
        with pytest.raises(ValueError, match=re.escape(words)):
            V.segment_latents(vq, z, penalties)
        with pytest.raises(ValueError, match=re.escape(words)):
            V.segment_many(None, vq, [np.zeros(640, np.float32)], penalties)
        with pytest.raises(ValueError, match=re.escape(words)):
            V.ResidentCorpus.describe([300, 300], [0, 1]).segment(None, vq, penalties)
    assert segmental.check_penalties(2).tolist() == [2.0] and segmental.check_penalties([0, 1.5]).dtype == np.float64
    assert segmental.check_penalties(np.float32(0.5)).shape == (1,) and len(segmental.check_penalties(range(16))) == 16
    assert segmental.MAX_K == 8192
    with pytest.raises(ValueError, match='k = 8193 codes; at most MAX_K = 8192'):
        V.segment_latents(_fake_vq(8193, 8), z, 1.0)
    with pytest.raises(ValueError, match='k = 8193'):
        V.segment_many(None, _fake_vq(8193, 8), [np.zeros(640, np.float32)], 1.0)
    with pytest.raises(ValueError, match='codebook must be \\(k, d\\) float32'):
        V.segment_latents(_fake_vq(16, 8, np.float64), z, 1.0)
    with pytest.raises(ValueError, match='utterance 1 have shape \\(7, 5\\); \\(d, frames\\) with d = 8 needed'):
        V.segment_latents(vq, z + [np.zeros((7, 5), np.float32)], 1.0)
    with pytest.raises(ValueError, match='utterance 0 have shape \\(40,\\)'):
        V.segment_latents(vq, [np.zeros(40, np.float32)], 1.0)
    with pytest.raises(ValueError, match='latents of utterance 1 are float64, float32 needed'):
        V.segment_latents(vq, z + [np.zeros((8, 5))], 1.0)
    with pytest.raises(ValueError, match='utterance 2 has no frames'):
        V.segment_latents(vq, z + z + [np.zeros((8, 0), np.float32)], 1.0)
    with pytest.raises(ValueError, match='no utterances'):
        V.segment_latents(vq, [], 1.0)
    with pytest.raises(ValueError, match='vq.W is not on the device'):
        V.segment_latents(types.SimpleNamespace(W=types.SimpleNamespace(data=np.zeros((4, 8), np.float32))), z, 1.0)
    with pytest.raises(ValueError, match='chunk_bytes must be positive'):
        segmental.plan_runs([3, 4], 8, 0)


def test_the_planner_cuts_whole_utterances():
    from vqvae_amd import segmental
    assert segmental.frame_bytes(128, 1) == 8 * 128 + 8 * 2 + 4 and segmental.frame_bytes(65, 4) == 8 * 65 + 4 * (16 + 4)
    assert segmental.frame_bytes(8192, 16) == 8 * 8192 + 16 * (8 * 128 + 4)
    tl = [10, 20, 5, 100, 1, 1]
    assert segmental.plan_runs(tl, 10, 1 << 30) == [(0, 6)]
    assert segmental.plan_runs(tl, 10, 350) == [(0, 3), (3, 4), (4, 6)]                    # 100 frames stand alone
    assert segmental.plan_runs(tl, 10, 1) == [(i, i + 1) for i in range(6)]
    assert segmental.plan_runs([7], 10, 1) == [(0, 1)]


def test_the_derived_figures():
    from vqvae_amd.segmental import SegmentalCodes

    class Flat(object):                                                  # LatentCodes is made on the device only
        def flat_view(self, offset, size):
            return np.zeros(size, np.int32)

    seg = SegmentalCodes([0.0, 2.0], [6, 10], 4, Flat(), [[3, 5], [1, 2]], [[1.5, 2.5], [7.0, 9.0]])
    assert np.array_equal(seg.distortion, [[1.5, 2.5], [7.0, 7.0]]) and len(seg) == 2 and len(seg.codes) == 2
    assert np.array_equal(seg.mean_run, [2.0, 16.0 / 3.0])
    assert np.array_equal(seg.segments_per_second(16000), [8.0 / (16 * 64 / 16000.0), 3.0 / (16 * 64 / 16000.0)])
    assert seg.n_segments.dtype == np.int32 and seg.cost.dtype == np.float64 and seg.codes[1].tl.tolist() == [6, 10]


# ---- the header segmental.py binds itself ------------------------------------------------------------------------------------------
def _code():
    text = open(HEADER).read()
    return re.sub(r'//[^\n]*', '', re.sub(r'/\*.*?\*/', '', text, flags=re.S))


def test_the_header_is_under_csrc_and_outside_the_registry():
    from vqvae_amd import _lib, segmental
    assert os.path.exists(HEADER) and segmental.HEADER == 'segmental.h' and segmental.HEADER not in os.listdir(A.INCLUDE)
    assert 'abi_version' not in open(HEADER).read()
    assert not any(n in h.prototypes for n in segmental.PROTOTYPES for h in _lib.HEADERS.values())
    assert not hasattr(_lib, 'SegDesc') and not any(n.startswith('SEG_') for n in vars(_lib))


def test_declared_functions_equal_the_bound_table():
    from vqvae_amd import segmental
    declared = sorted(set(re.findall(r'\b(vqvae_[a-z0-9_]+)\s*\(', _code())))
    assert declared == sorted(segmental.PROTOTYPES) and len(declared) == 4
    for name, (res, args) in segmental.PROTOTYPES.items():
        found = re.findall(r'\b%s\s*\(([^()]*)\)\s*;' % name, _code())
        assert len(found) == 1, name
        params = found[0].strip()
        assert (0 if params == 'void' else len(params.split(','))) == len(args), (name, params)
    lib = segmental.load()
    for name, (res, args) in segmental.PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert lib.vqvae_seg_revision() == segmental.REVISION == 1


def test_the_descriptor_and_the_macros_are_the_compiler_s(tmp_path):
    from vqvae_amd import segmental
    declared = {}
    for body, name in re.findall(r'typedef\s+struct[^{;]*\{([^}]*)\}\s*(\w+)\s*;', _code()):
        declared[name] = [re.findall(r'\w+', re.sub(r'\[[^\]]*\]', '', declarator))[-1] for declaration in body.split(';')
                          if declaration.strip() for declarator in declaration.split(',')]
    mirrored = {cls._c_name_: cls for cls in segmental.STRUCTS}
    assert set(declared) == set(mirrored) == {'vqvae_seg_desc'}
    assert declared['vqvae_seg_desc'] == ['n', 'd', 'k', 'n_pen', 'ttot', 'stride', 'code_stride', 'utt_stride', 'lam']
    lines = []
    for t, cls in mirrored.items():
        assert [f for f, _ in cls._fields_] == declared[t], t
        lines.append('printf("%s %%d\\n", (int)sizeof(%s));' % (t, t))
        for f, _ in cls._fields_:
            lines.append('printf("%s.%s %%d %%d\\n", (int)offsetof(%s, %s), (int)sizeof(((%s*)0)->%s));' % (t, f, t, f, t, f))
    macros = {'VQVAE_SEG_MAX_K': segmental.MAX_K, 'VQVAE_SEG_MAX_PEN': segmental.MAX_PEN, 'VQVAE_SEG_WAVE_K': segmental.WAVE_K,
              'VQVAE_SEG_LANES': segmental.LANES, 'VQVAE_SEG_TILE': segmental.TILE}
    assert sorted(m for m in re.findall(r'^[ \t]*#[ \t]*define[ \t]+(VQVAE_\w+)', _code(), flags=re.M) if not m.endswith('_H_')) == sorted(macros)
    lines += ['printf("%s %%d\\n", (int)(%s));' % (m, m) for m in macros]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HEADER, 'int main(void) {'] + lines + ['return 0; }', '']
    c, exe = str(tmp_path / 'seg.c'), str(tmp_path / 'seg')
    open(c, 'w').write('\n'.join(src))
    subprocess.check_call([A.host_cc(), '-std=c99', '-o', exe, c])
    out = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in subprocess.check_output([exe], universal_newlines=True).splitlines()}
    for t, cls in mirrored.items():
        assert out[t] == [C.sizeof(cls)] == [176], t
        for f, _ in cls._fields_:
            d = getattr(cls, f)
            assert out['%s.%s' % (t, f)] == [d.offset, d.size], (t, f)
    for m, v in macros.items():
        assert out[m] == [v], m
    assert segmental.MAX_K == 32 * segmental.LANES and segmental.WAVE_K == 8 * 64


def test_a_bumped_revision_is_the_exact_import_error(monkeypatch):
    from vqvae_amd import _lib, segmental
    monkeypatch.setattr(segmental, '_bound', None)
    monkeypatch.setattr(segmental, 'REVISION', 2)
    with pytest.raises(ImportError) as e:
        segmental.load()
    assert str(e.value) == ('libvqvae_hip.so at %s has segmental revision 1, this package binds 2: rebuild it '
                            '(__graft_entry__.build())' % _lib.LIB_PATH)
    assert segmental._bound is None


def test_the_source_is_built_and_depends_on_its_header():
    srcs = re.search(r'^SRCS\s*:?=\s*(.*)$', A.make_database(), flags=re.M).group(1).split()
    assert 'segmental.hip' in srcs
    assert 'segmental.h' in [os.path.basename(p) for p in A.object_rule_prerequisites()]


def _good():
    from vqvae_amd import segmental
    d = segmental.SegDesc()
    d.n, d.d, d.k, d.n_pen, d.ttot, d.stride, d.code_stride, d.utt_stride = 2, 8, 128, 3, 10, 10, 10, 2
    d.lam[0], d.lam[1], d.lam[2] = 0.0, 1.0, 2.5
    d.lam[3] = float('nan')                                              # beyond n_pen: not read
    return d


def test_the_workspace_query_restates_the_plan():
    from vqvae_amd import segmental
    lib = segmental.load()
    up = lambda v: (v + 255) // 256 * 256
    for k, P, ttot in ((128, 3, 10), (1, 1, 1), (65, 16, 1000), (8192, 2, 7), (513, 4, 300)):
        d = _good()
        d.k, d.n_pen, d.ttot, d.stride, d.code_stride = k, P, ttot, ttot, ttot
        d.n = d.utt_stride = 1
        for q in range(P):
            d.lam[q] = 1.0
        want = up(8 * ttot * k) + up(8 * P * ttot * ((k + 63) // 64)) + up(4 * P * ttot)
        assert lib.vqvae_seg_workspace_bytes(C.byref(d)) == want, (k, P, ttot)
        assert want <= ttot * segmental.frame_bytes(k, P) + 3 * 255
    d = _good()
    d.k = 8193
    assert lib.vqvae_seg_workspace_bytes(C.byref(d)) == C.c_size_t(-1).value == lib.vqvae_seg_workspace_bytes(None)


def test_a_bad_descriptor_is_refused_on_the_host_side_of_the_library():
    """The entry points validate before they launch, so the refusals can be had without a device."""
    from vqvae_amd import segmental
    lib = segmental.load()
    one = C.c_void_p(256)                                                # never dereferenced: every call below is refused
    calls = {'seg_distances': lambda d: lib.vqvae_seg_distances(d, one, one, one, None),
             'seg_segment': lambda d: lib.vqvae_seg_segment(d, one, one, one, one, one, one, one, 1 << 40, None)}
    bad = (('n', 0, 'n must be at least 1'), ('d', 0, 'd must be at least 1'), ('k', 0, 'k must be in [1, 8192]'),
           ('k', 8193, 'k must be in [1, 8192]'), ('n_pen', 0, 'n_pen must be in [1, 16]'), ('n_pen', 17, 'n_pen must be in [1, 16]'),
           ('ttot', 1, 'ttot must be at least n'), ('stride', 9, 'stride must be at least ttot'),
           ('code_stride', 9, 'code_stride must be at least ttot'), ('utt_stride', 1, 'utt_stride must be at least n'))
    for who, entry in calls.items():
        for field, value, words in bad:
            d = _good()
            setattr(d, field, value)
            rc = entry(C.byref(d))
            msg = lib.vqvae_last_error_string().decode()
            assert rc != 0 and who in msg and words in msg, (who, field, rc, msg)
            assert lib.vqvae_seg_workspace_bytes(C.byref(d)) == C.c_size_t(-1).value, field
        for value in (-1.0, float('nan'), float('inf')):
            d = _good()
            d.lam[2] = value
            assert entry(C.byref(d)) != 0 and 'every penalty must be finite and not negative' in lib.vqvae_last_error_string().decode()
        assert entry(None) != 0 and 'null descriptor' in lib.vqvae_last_error_string().decode()
    d = _good()
    need = lib.vqvae_seg_workspace_bytes(C.byref(d))
    assert lib.vqvae_seg_segment(C.byref(d), one, one, one, one, one, one, one, need - 1, None) != 0
    assert 'the workspace must hold %d bytes (got %d)' % (need, need - 1) in lib.vqvae_last_error_string().decode()
    assert lib.vqvae_seg_segment(C.byref(d), one, one, one, one, one, one, None, need, None) != 0
    assert 'the workspace must hold' in lib.vqvae_last_error_string().decode()
    assert lib.vqvae_seg_segment(C.byref(d), one, one, one, one, None, one, one, need, None) != 0
    assert 'seg_segment: null' in lib.vqvae_last_error_string().decode()
    assert lib.vqvae_seg_distances(C.byref(d), one, one, None, None) != 0
    assert 'seg_distances: null' in lib.vqvae_last_error_string().decode()


def test_the_package_imports_without_a_library_call():
    code = ('import vqvae_amd as V, vqvae_amd._lib as L, vqvae_amd.segmental as S; '
            'assert L._lib is None and S._bound is None; '
            'assert all(getattr(V, n) is getattr(S, n) for n in ("segment_latents", "segment_many", "SegmentalCodes")); '
            'assert V.CorpusView.segment is V.ResidentCorpus.segment')
    env = dict(os.environ, PYTHONPATH=os.path.join(A.ROOT, 'chainer-vq-vae_amd'))
    subprocess.check_call([sys.executable, '-c', code], env=env)


def test_the_front_end_hook_is_optional():
    """With no hook the front end's driver is what it was: the hook is a trailing keyword with a None default."""
    import inspect
    from vqvae_amd import frontend
    for fn in (frontend._run, frontend._encode_chunk):
        assert inspect.signature(fn).parameters['hook'].default is None
    text = inspect.getsource(frontend._encode_chunk)
    assert text.count('\n        hook(') == 1 and 'if hook is not None:\n        hook(src, T, tb, first)' in text
