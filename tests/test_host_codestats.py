"""CPU checks of the code statistics (vqvae_amd.codestats, csrc/codes_abi.h): the two NumPy restatements of the edit
distance and of the counts against each other and against answers known by construction, the derived figures against
closed forms and against their restatement, every refusal, and the binding of the header that codestats.py carries itself
-- the declared functions, parameter counts, struct layouts as a C99 compiler sees them, the version error, the source's
place in the Makefile and the workspace queries."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import abi_headers as A
import codestats_ref as R

HEADER = os.path.join(A.CSRC, 'codes_abi.h')
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


# ---- the header codestats.py binds itself ------------------------------------------------------------------------------------------
def _code():
    text = open(HEADER).read()
    return re.sub(r'//[^\n]*', '', re.sub(r'/\*.*?\*/', '', text, flags=re.S))


def test_declared_functions_equal_the_bound_table():
    from vqvae_amd import _lib, codestats
    declared = sorted(set(re.findall(r'\b(vqvae_[a-z0-9_]+)\s*\(', _code())))
    assert declared == sorted(codestats.PROTOTYPES) and len(declared) == 9
    for name, (res, args) in codestats.PROTOTYPES.items():
        found = re.findall(r'\b%s\s*\(([^()]*)\)\s*;' % name, _code())
        assert len(found) == 1, name
        params = found[0].strip()
        assert (0 if params == 'void' else len(params.split(','))) == len(args), (name, params)
    lib = codestats.load()
    for name, (res, args) in codestats.PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert lib.vqvae_codes_abi_version() == codestats.ABI_VERSION == 1
    # nothing was added to _lib's tables or namespace: the header is not under include/
    assert not any(n in h.prototypes for n in codestats.PROTOTYPES for h in _lib.HEADERS.values())
    assert codestats.HEADER not in os.listdir(A.INCLUDE) and not hasattr(_lib, 'PairDesc')
    assert codestats.ABI_WORDS == 'code-statistics ABI'


def test_struct_layouts_and_macros_are_the_compiler_s(tmp_path):
    from vqvae_amd import codestats
    declared = {}
    for body, name in re.findall(r'typedef\s+struct[^{;]*\{([^}]*)\}\s*(\w+)\s*;', _code()):
        declared[name] = [re.findall(r'\w+', declarator)[-1] for declaration in body.split(';') if declaration.strip()
                          for declarator in declaration.split(',')]
    mirrored = {cls._c_name_: cls for cls in codestats.STRUCTS}
    assert set(declared) == set(mirrored) == {'vqvae_codes_runs_desc', 'vqvae_codes_hist_desc', 'vqvae_codes_pair_desc',
                                              'vqvae_codes_pair_tables'}
    lines = []
    for t, cls in mirrored.items():
        assert [f for f, _ in cls._fields_] == declared[t], t
        lines.append('printf("%s %%d\\n", (int)sizeof(%s));' % (t, t))
        for f, _ in cls._fields_:
            lines.append('printf("%s.%s %%d %%d\\n", (int)offsetof(%s, %s), (int)sizeof(((%s*)0)->%s));' % (t, f, t, f, t, f))
    macros = {'VQVAE_CODES_MAX_SHORT': codestats.MAX_SHORT, 'VQVAE_CODES_THREADS': codestats.THREADS,
              'VQVAE_CODES_MAX_BIGRAM_K': codestats.MAX_BIGRAM_K}
    assert sorted(m for m in re.findall(r'^[ \t]*#[ \t]*define[ \t]+(VQVAE_\w+)', _code(), flags=re.M) if not m.endswith('_H_')) == sorted(macros)
    lines += ['printf("%s %%d\\n", (int)(%s));' % (m, m) for m in macros]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HEADER, 'int main(void) {'] + lines + ['return 0; }', '']
    c, exe = str(tmp_path / 'codes.c'), str(tmp_path / 'codes')
    open(c, 'w').write('\n'.join(src))
    subprocess.check_call([A.host_cc(), '-std=c99', '-o', exe, c])                # one C99 program, as abi_headers.run_c99
    out = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in subprocess.check_output([exe], universal_newlines=True).splitlines()}
    for t, cls in mirrored.items():
        assert out[t] == [C.sizeof(cls)], t
        for f, _ in cls._fields_:
            d = getattr(cls, f)
            assert out['%s.%s' % (t, f)] == [d.offset, d.size], (t, f)
    for m, v in macros.items():
        assert out[m] == [v], m


def test_a_bumped_bound_version_is_the_exact_import_error(monkeypatch):
    from vqvae_amd import _lib, codestats
    monkeypatch.setattr(codestats, '_bound', None)
    monkeypatch.setattr(codestats, 'ABI_VERSION', 2)
    with pytest.raises(ImportError) as e:
        codestats.load()
    assert str(e.value) == 'libvqvae_hip.so at %s has code-statistics ABI 1, this package binds 2: rebuild it (__graft_entry__.build())' % _lib.LIB_PATH
    assert codestats._bound is None


def test_the_source_is_built_and_depends_on_its_header():
    srcs = re.search(r'^SRCS\s*:?=\s*(.*)$', A.make_database(), flags=re.M).group(1).split()
    assert 'code_stats.hip' in srcs
    assert 'codes_abi.h' in [os.path.basename(p) for p in A.object_rule_prerequisites()]


def test_the_workspace_queries_refuse_what_the_entry_points_refuse():
    from vqvae_amd import codestats
    lib = codestats.load()
    refused = C.c_size_t(-1).value
    cases = (('vqvae_codes_runs_workspace_bytes', lambda: codestats.RunsDesc(3, 64, 10),
              (('n', 0), ('max_run', 0), ('total', 2))),
             ('vqvae_codes_hist_workspace_bytes', lambda: codestats.HistDesc(3, 4096, 2, 1, 0, 0, 10),
              (('n', 0), ('k', 0), ('k', 4097), ('groups', 0), ('bigrams', 2), ('accumulate', -1), ('reserved', 1), ('total', 2))),
             ('vqvae_codes_agree_workspace_bytes', lambda: codestats.PairDesc(3, codestats.MAX_SHORT, 10, 3),
              (('n', 0), ('max_short', 0), ('max_short', codestats.MAX_SHORT + 1), ('total_a', 2), ('total_b', 0))),
             ('vqvae_codes_edit_workspace_bytes', lambda: codestats.PairDesc(3, 1, 3, 10),
              (('n', 0), ('max_short', 0), ('max_short', codestats.MAX_SHORT + 1), ('total_a', 2), ('total_b', 0))))
    for query, good, bad in cases:
        assert getattr(lib, query)(C.byref(good())) == 0, query            # none of them keeps anything outside its outputs
        assert getattr(lib, query)(None) == refused, query
        for field, value in bad:
            d = good()
            setattr(d, field, value)
            assert getattr(lib, query)(C.byref(d)) == refused, (query, field, value)
    unigrams = codestats.HistDesc(3, 8192, 2, 0, 1, 0, 10)                  # k above the bigram bound without bigrams
    assert lib.vqvae_codes_hist_workspace_bytes(C.byref(unigrams)) == 0


def test_the_package_exports_the_calls():
    import vqvae_amd as V
    from vqvae_amd import codestats
    for name in ('code_stats', 'collapse_many', 'compare_codes_many', 'CodeStats', 'CodeRuns', 'CodeComparison'):
        assert getattr(V, name) is getattr(codestats, name), name
    assert V.CorpusView.code_stats is V.ResidentCorpus.code_stats
