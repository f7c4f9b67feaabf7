"""CPU checks of the code statistics (vqvae_amd.codestats, include/vqvae_codes.h): the two NumPy restatements of the edit
distance and of the counts against each other and against answers known by construction, the derived figures against
closed forms and against their restatement, every refusal, and what is this header's own in the registry of
vqvae_amd/_lib.py -- its literal names, structs and limits, the workspace queries and the source's place in the
Makefile; the table against the header text, the library and the compiler's layout is tests/test_host_abi.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import abi_headers as A
import codestats_ref as R

HEADER = 'vqvae_codes.h'
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (5, 9), (9, 5), (63, 65), (64, 64), (40, 33)]
ALPHABETS = [2, 3, 128]


def _string(n, k, seed):
    return np.random.RandomState(seed).randint(0, k, n).astype(np.int32)


def _codes(utts, k):
    from vqvae_amd.frontend import LatentCodes
    return LatentCodes(np.array([len(u) for u in utts], np.int32), np.concatenate([np.asarray(u, np.int32) for u in utts]), k)


# ---- the restatements ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', ALPHABETS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
def test_the_two_edit_restatements_agree(shape, k):
    La, Lb = shape
    a, b = _string(La, k, 10 * La + k), _string(Lb, k, 10 * Lb + k + 1)
    loops, diagonals = R.edit_loops(a, b), R.edit_diagonals(a, b)
    assert loops == diagonals, (loops, diagonals)
    dist, subs = loops
    dels, ins, matches = R.derive(dist, subs, La, Lb)                    # the identities: integral and non-negative
    assert min(dels, ins, matches, subs) >= 0 and dist == subs + ins + dels
    assert matches + subs + dels == La and matches + subs + ins == Lb
    assert abs(La - Lb) <= dist <= max(La, Lb)


@pytest.mark.parametrize('edit', [R.edit_loops, R.edit_diagonals], ids=['loops', 'diagonals'])
def test_edit_answers_known_by_construction(edit):
    a = _string(40, 7, 1)
    assert edit(a, a) == (0, 0)
    for La, Lb in ((5, 9), (9, 5), (6, 6), (1, 4)):                     # disjoint alphabets: nothing matches
        x, y = _string(La, 3, 2), _string(Lb, 3, 3) + 3
        assert edit(x, y) == (max(La, Lb), min(La, Lb)), (La, Lb)
    a = np.arange(30, dtype=np.int32) % 11                              # no two neighbours equal: removing is unambiguous
    b = a[np.arange(30) % 3 != 2]
    removed = 30 - len(b)
    dist, subs = edit(a, b)
    assert (dist, subs) == (removed, 0) and R.derive(dist, subs, 30, len(b)) == (removed, 0, len(b))
    dist, subs = edit(b, a)                                             # the other way: insertions
    assert (dist, subs) == (removed, 0) and R.derive(dist, subs, len(b), 30) == (0, removed, len(b))
    assert edit([1, 2, 3], [1, 5, 3]) == (1, 1) and edit([4], [4, 4, 4]) == (2, 0)


def test_runs_and_their_histogram():
    u, dur = R.runs([5, 5, 5, 2, 5, 5, 7])
    assert u.tolist() == [5, 2, 5, 7] and dur.tolist() == [3, 1, 2, 1] and u.dtype == dur.dtype == np.int32
    assert R.runs([3])[1].tolist() == [1] and R.runs([1, 2, 1, 2])[1].tolist() == [1, 1, 1, 1]
    assert R.run_hist([[3, 1, 2, 1], [9]], 4).tolist() == [2, 1, 1, 1]  # 9 in the clamp bucket
    assert R.run_hist([[3, 1, 2, 1]], 1).tolist() == [4]


def test_the_two_count_restatements_agree():
    rs = np.random.RandomState(4)
    utts = [rs.randint(0, 6, n) for n in (1, 2, 17, 64, 5)]
    utts[2][7], utts[3][0], utts[3][63] = -1, 6, 9                       # invalid codes: the middle, the first, the last position
    groups = [0, 2, 2, 0, 3]                                            # group 1 empty, group 3 outside [0, 3)
    loops, at = R.counts_loops(utts, groups, 6, 3), R.counts_add_at(utts, groups, 6, 3)
    assert np.array_equal(loops[0], at[0]) and np.array_equal(loops[1], at[1]) and loops[2] == at[2] == 3 + 5
    uni, big, _ = loops
    assert uni.sum() == 1 + 2 + 16 + 62 and uni[1].sum() == 0
    assert big.sum() == 0 + 1 + (16 - 2) + (63 - 1 - 1)                  # an invalid code takes the transitions on both its sides
    assert R.counts_loops(utts, groups, 6, 3, bigrams=False)[1] is None
    assert R.agreement([1, 2, 3, 4], [1, 0, 3]) == (2, 3) and R.agreement([7], [7, 7]) == (1, 1)


# ---- the figures ---------------------------------------------------------------------------------------------------------------
def test_figures_in_closed_form():
    from vqvae_amd.codestats import figures
    same = np.array([[3, 0, 5, 1]] * 3, np.int64) * np.array([[1], [2], [7]])       # the same histogram at three sizes
    f = figures(same)
    assert f['mi_bits'] == 0.0 and f['mi_normalised'] == 0.0 and R.mi_bits(same) == 0.0
    assert np.array_equal(f['js_bits'], np.zeros((3, 3)))
    one = figures(same[:1])
    assert one['mi_bits'] == 0.0 and one['mi_normalised'] == 0.0        # G = 1
    code_is_speaker = np.diag([4, 4, 8, 16]).astype(np.int64)
    f = figures(code_is_speaker)
    HS = R.speaker_entropy_bits(code_is_speaker)
    assert HS == 1.75 and abs(f['mi_bits'] - HS) <= 1e-12 and abs(f['mi_normalised'] - 1.0) <= 1e-12
    assert abs(f['entropy_bits'] - 1.75) <= 1e-12 and f['used'] == 4 and f['used_per_speaker'].tolist() == [1, 1, 1, 1]
    assert np.allclose(f['js_bits'], 1.0 - np.eye(4), rtol=0, atol=1e-12)           # disjoint supports: one bit
    uniform = figures(np.full((2, 64), 5, np.int64))
    assert uniform['entropy_bits'] == 6.0 and uniform['perplexity'] == 64.0 and uniform['used'] == 64 and uniform['positions'] == 640
    f = figures(np.array([[2, 1, 0], [0, 0, 0], [1, 1, 4]], np.int64))
    js = f['js_bits']
    assert np.isnan(js[1]).all() and np.isnan(js[:, 1]).all() and js[0, 0] == js[2, 2] == 0.0 and js[0, 2] == js[2, 0] > 0
    big = np.array([[6, 2], [2, 6]], np.int64)
    f = figures(np.array([[8, 8]], np.int64), big)
    assert f['self_share'] == 0.75 and f['transitions'] == 16
    assert abs(f['next_entropy_bits'] - (-(0.75 * np.log2(0.75) + 0.25 * np.log2(0.25)))) <= 1e-12
    assert figures(np.array([[1, 1]], np.int64), np.array([[0, 3], [3, 0]], np.int64))['next_entropy_bits'] == 0.0


@pytest.mark.parametrize('G,k', [(1, 5), (3, 17), (7, 128)])
def test_figures_equal_their_restatement(G, k):
    """Float64 sums of at most G k terms on both sides: 1e-12, the bar of the other restated figures."""
    from vqvae_amd.codestats import figures
    rs = np.random.RandomState(G * k)
    uni = rs.randint(0, 40, (G, k)).astype(np.int64) * (rs.uniform(size=(G, k)) < 0.6)
    big = rs.randint(0, 9, (k, k)).astype(np.int64) * (rs.uniform(size=(k, k)) < 0.3)
    f = figures(uni, big)
    HS = R.speaker_entropy_bits(uni)
    want = dict(entropy_bits=R.entropy_bits(uni), mi_bits=R.mi_bits(uni), self_share=R.self_share(big),
                next_entropy_bits=R.next_entropy_bits(big), perplexity=2.0 ** R.entropy_bits(uni),
                mi_normalised=R.mi_bits(uni) / HS if G > 1 else 0.0)
    for name, v in want.items():
        print('%s: %.17g against %.17g' % (name, f[name], v))
        assert abs(f[name] - v) <= 1e-12 * max(1.0, abs(v)), name
    js = R.js_bits(uni)
    assert np.array_equal(f['js_bits'], f['js_bits'].T) and (np.diag(f['js_bits']) == 0).all()
    assert np.abs(f['js_bits'] - js).max() <= 1e-12
    assert f['positions'] == uni.sum() and f['used'] == (uni.sum(axis=0) > 0).sum() and f['transitions'] == big.sum()


# ---- the refusals ----------------------------------------------------------------------------------------------------------------
def test_every_refusal_names_its_reason():
    """Host codes are uploaded when the device buffer is first asked for: none of these calls gets that far."""
    import vqvae_amd as V
    from vqvae_amd import codestats
    M = codestats.MAX_SHORT
    assert M == 6143 and 24 * M <= 144 * 1024 <= 160 * 1024 and 24 * (M + 2) > 144 * 1024
    two, three = _codes([[1, 2], [3]], 8), _codes([[1], [2], [3]], 8)
    with pytest.raises(TypeError, match='codes_b must be a frontend.LatentCodes'):
        V.compare_codes_many(two, [[1, 2], [3]])
    with pytest.raises(ValueError, match='2 utterances on side a and 3 on side b'):
        V.compare_codes_many(two, three)
    with pytest.raises(ValueError, match='side a has k = 8 and side b k = 9'):
        V.compare_codes_many(two, _codes([[1, 2], [3]], 9))
    long_ = _codes([[1], np.zeros(M + 1, np.int32)], 8)
    with pytest.raises(ValueError, match='pair 1 has %d and %d codes; the shorter side may have at most %d' % (M + 1, M + 1, M)):
        V.compare_codes_many(long_, long_)
    with pytest.raises(ValueError, match='k = 4097: the bigram table would have 134283272 bytes; .* ask for bigrams=False'):
        V.code_stats(_codes([[1, 2]], 4097))
    for speakers, n_speakers, words in (([0], None, 'one integer speaker id per utterance \\(2\\)'),
                                        ([0.0, 1.0], None, 'one integer speaker id per utterance'),
                                        ([0, -1], None, 'utterance 1 has speaker -1'),
                                        ([0, 3, 5], 3, 'one integer speaker id'),
                                        ([3, 1], 3, 'utterance 0 has speaker 3; speaker ids must be in \\[0, 3\\)')):
        with pytest.raises(ValueError, match=words):
            V.code_stats(two, speakers=speakers, n_speakers=n_speakers)
    with pytest.raises(ValueError, match='max_run must be at least 1'):
        V.code_stats(two, max_run=0)
    with pytest.raises(ValueError, match='max_run must be at least 1'):
        V.collapse_many(two, max_run=0)
    with pytest.raises(ValueError, match='permutations = 3 without speakers'):
        V.code_stats(two, permutations=3)
    with pytest.raises(TypeError, match='codes must be a frontend.LatentCodes'):
        V.code_stats([[1, 2]])
    with pytest.raises(TypeError, match='codes must be a frontend.LatentCodes'):
        V.collapse_many(np.zeros(3, np.int32))
    view = V.ResidentCorpus.describe([100, 100, 100], [0, 1, 1]).subset([2, 0])
    with pytest.raises(ValueError, match='permutations must not be negative'):     # the view hands over its own speakers
        view.code_stats(two, permutations=-1)
    with pytest.raises(ValueError, match='one integer speaker id per utterance \\(3\\)'):
        view.code_stats(three)
    assert all(c._dev is None for c in (two, three, long_))                        # nothing was uploaded


def test_the_comparison_derives_the_rest():
    from vqvae_amd.codestats import CodeComparison
    i64 = lambda *v: np.array(v, np.int64)
    c = CodeComparison(i64(10, 0), i64(0, 0), i64(30, 4), i64(20, 4), i64(3, 4), i64(20, 4), True)
    assert (c.dels.tolist(), c.ins.tolist(), c.matches.tolist()) == ([10, 0], [0, 0], [20, 4]) and len(c) == 2
    assert c.error_rate.tolist() == [10 / 30, 0.0] and c.normalised.tolist() == [10 / 30, 0.0] and c.agreement.tolist() == [0.15, 1.0]
    assert all(getattr(c, n).dtype == np.int64 for n in ('distance', 'subs', 'ins', 'dels', 'matches', 'len_a', 'len_b', 'agree', 'overlap'))


# ---- the header, the table -----------------------------------------------------------------------------------------------------
NAMES = {'vqvae_codes_abi_version', 'vqvae_codes_runs_workspace_bytes', 'vqvae_codes_hist_workspace_bytes',
         'vqvae_codes_agree_workspace_bytes', 'vqvae_codes_edit_workspace_bytes', 'vqvae_codes_runs', 'vqvae_codes_hist',
         'vqvae_codes_agree', 'vqvae_codes_edit'}


def test_the_header_is_in_the_registry_and_codestats_binds_nothing():
    from vqvae_amd import _lib, codestats
    h = _lib.HEADERS[HEADER]                                   # against the header and the library: tests/test_host_abi.py
    assert set(h.prototypes) == NAMES and len(NAMES) == 9 and h.words == 'code-statistics ABI' and h.version == 1
    assert HEADER in os.listdir(A.INCLUDE) and not any('abi_version' in open(os.path.join(A.CSRC, f)).read() for f in os.listdir(A.CSRC) if f.endswith('.h'))
    mirrored = {'vqvae_codes_runs_desc': (_lib.CodesRunsDesc, ['n', 'max_run', 'total']),
                'vqvae_codes_hist_desc': (_lib.CodesHistDesc, ['n', 'k', 'groups', 'bigrams', 'accumulate', 'reserved', 'total']),
                'vqvae_codes_pair_desc': (_lib.CodesPairDesc, ['n', 'max_short', 'total_a', 'total_b']),
                'vqvae_codes_pair_tables': (_lib.CodesPairTables, ['start_a', 'len_a', 'start_b', 'len_b'])}
    assert set(A.structs(HEADER)) == set(mirrored)
    for c_name, (cls, fields) in mirrored.items():
        assert cls._c_name_ == c_name and [f for f, _ in cls._fields_] == fields, c_name
    assert sorted(A.macros(HEADER)) == ['VQVAE_CODES_MAX_BIGRAM_K', 'VQVAE_CODES_MAX_SHORT', 'VQVAE_CODES_THREADS']
    assert (_lib.CODES_MAX_SHORT, _lib.CODES_THREADS, _lib.CODES_MAX_BIGRAM_K) == (6143, 256, 4096)
    assert (codestats.MAX_SHORT, codestats.THREADS, codestats.MAX_BIGRAM_K) == (6143, 256, 4096)
    for name in ('HEADER', 'ABI_WORDS', 'ABI_VERSION', 'PROTOTYPES', 'STRUCTS', '_bound', 'load', 'call', '_workspace',
                 'RunsDesc', 'HistDesc', 'PairDesc', 'PairTables'):
        assert not hasattr(codestats, name), name


def test_the_source_is_built_and_depends_on_its_header():
    srcs = re.search(r'^SRCS\s*:?=\s*(.*)$', A.make_database(), flags=re.M).group(1).split()
    assert 'code_stats.hip' in srcs
    assert HEADER in [os.path.basename(p) for p in A.object_rule_prerequisites()]


def test_the_workspace_queries_refuse_what_the_entry_points_refuse():
    from vqvae_amd import _lib, codestats
    lib = _lib.load()
    refused = C.c_size_t(-1).value
    cases = (('vqvae_codes_runs_workspace_bytes', lambda: _lib.CodesRunsDesc(3, 64, 10),
              (('n', 0), ('max_run', 0), ('total', 2))),
             ('vqvae_codes_hist_workspace_bytes', lambda: _lib.CodesHistDesc(3, 4096, 2, 1, 0, 0, 10),
              (('n', 0), ('k', 0), ('k', 4097), ('groups', 0), ('bigrams', 2), ('accumulate', -1), ('reserved', 1), ('total', 2))),
             ('vqvae_codes_agree_workspace_bytes', lambda: _lib.CodesPairDesc(3, codestats.MAX_SHORT, 10, 3),
              (('n', 0), ('max_short', 0), ('max_short', codestats.MAX_SHORT + 1), ('total_a', 2), ('total_b', 0))),
             ('vqvae_codes_edit_workspace_bytes', lambda: _lib.CodesPairDesc(3, 1, 3, 10),
              (('n', 0), ('max_short', 0), ('max_short', codestats.MAX_SHORT + 1), ('total_a', 2), ('total_b', 0))))
    for query, good, bad in cases:
        assert getattr(lib, query)(C.byref(good())) == 0, query            # none of them keeps anything outside its outputs
        assert getattr(lib, query)(None) == refused, query
        for field, value in bad:
            d = good()
            setattr(d, field, value)
            assert getattr(lib, query)(C.byref(d)) == refused, (query, field, value)
    unigrams = _lib.CodesHistDesc(3, 8192, 2, 0, 1, 0, 10)                  # k above the bigram bound without bigrams
    assert lib.vqvae_codes_hist_workspace_bytes(C.byref(unigrams)) == 0


def test_the_package_exports_the_calls():
    import vqvae_amd as V
    from vqvae_amd import codestats
    for name in ('code_stats', 'collapse_many', 'compare_codes_many', 'CodeStats', 'CodeRuns', 'CodeComparison'):
        assert getattr(V, name) is getattr(codestats, name), name
    assert V.CorpusView.code_stats is V.ResidentCorpus.code_stats
