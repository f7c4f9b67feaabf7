"""CPU checks of the ABX module (vqvae_amd.abx, csrc/abx.h): the NumPy restatement of the rule (tests/abx_ref.py) against
the objective it must minimise (a brute force over all monotone paths) and against its own second statement (rows against
anti-diagonals); exact ties; answers known by construction; the plan of both tasks against a brute force over all item
triples; every refusal; and the binding of the header that abx.py carries itself -- the declared functions, parameter
counts, the structures' layout as a C99 compiler sees it, the revision error, the source's place in the Makefile.

Integer-valued features make every local cost of the brute-force cases an exact small integer (euclidean over one channel:
|a - b|), so the recurrence's cost EQUALS the brute force's minimum; everything else is an equality too.  The device is not
involved."""
import ctypes as C
import itertools
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

import abi_headers as A
import abx_ref as R

HEADER = os.path.join(A.CSRC, 'abx.h')


def _ints(rs, d, F, hi=4):
    return rs.randint(0, hi, (d, F)).astype(np.float32)


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def test_the_restated_cost_is_the_cheapest_monotone_path():
    """Every pair of sides up to 5 x 5, integer-valued features of one channel: d = |a - b| exactly."""
    rs = np.random.RandomState(0)
    for Fa, Fb in itertools.product(range(1, 6), repeat=2):
        for rep in range(4):
            d = R.local(_ints(rs, 1, Fa), _ints(rs, 1, Fb), 'euclidean')
            assert np.array_equal(d, np.round(d))
            cost, K = R.dtw_rows(d)
            assert cost == R.brute_force(d), (Fa, Fb, rep)
            assert max(Fa, Fb) <= K <= Fa + Fb - 1
            assert R.dtw_diagonals(d) == (cost, K)


def test_rows_and_diagonals_agree():
    rs = np.random.RandomState(1)
    for Fa, Fb, d in ((1, 1, 3), (1, 40, 2), (40, 1, 2), (17, 33, 5), (64, 65, 1), (30, 7, 16)):
        for metric in ('cosine', 'euclidean'):
            for x in (_ints(rs, d, Fa), rs.randn(d, Fa).astype(np.float32)):
                y = _ints(rs, d, Fb) if x[0, 0] == round(x[0, 0]) else rs.randn(d, Fb).astype(np.float32)
                loc = R.local(x, y, metric)
                assert R.dtw_rows(loc) == R.dtw_diagonals(loc), (Fa, Fb, d, metric)


def test_the_local_cost_is_the_sum_in_ascending_j():
    rs = np.random.RandomState(2)
    xa, xb = rs.randn(5, 4).astype(np.float32), rs.randn(5, 3).astype(np.float32)
    cos, euc = R.local(xa, xb, 'cosine'), R.local(xa, xb, 'euclidean')
    for i in range(4):
        for j in range(3):
            dot = na = nb = s = np.float64(0.0)
            for c in range(5):
                a, b = np.float64(xa[c, i]), np.float64(xb[c, j])
                dot, na, nb = dot + a * b, na + a * a, nb + b * b
                s = s + (a - b) * (a - b)
            assert euc[i, j] == np.sqrt(s)
            assert cos[i, j] == max(np.float64(1.0) - dot / np.sqrt(na * nb), 0.0)
    assert np.array_equal(R.norms(xa), [sum(np.float64(v) * np.float64(v) for v in xa[:, i]) for i in range(4)])


def test_on_exact_ties_the_path_length_follows_the_candidate_order():
    # all costs 0: the diagonal is tried first and nothing is strictly smaller, so K = max(Fa, Fb) ... by way of the diagonal
    assert R.dtw_rows(np.zeros((3, 3))) == (0.0, 3) and R.dtw_rows(np.zeros((2, 5))) == (0.0, 5)
    # (1, 1) reaches cost 1 three ways; the diagonal (K 2) is kept over up and left (K 3)
    assert R.dtw_rows(np.array([[0.0, 0.0], [0.0, 1.0]])) == (1.0, 2)
    # the end cell of a 2 x 3: diagonal D(0, 1) = 0 with K 2, up D(0, 2) = 0 with K 3, left D(1, 1) = 0 with K 2: diagonal
    d = np.zeros((2, 3))
    assert R.dtw_rows(d) == (0.0, 3)
    # up beats left on a tie between them when the diagonal is dearer: D(0,0)=5; D(0,1)=5, D(1,0)=5 -> (1,1) takes the
    # diagonal (5, K 1); make the diagonal dearer instead
    d = np.array([[1.0, 0.0, 9.0], [0.0, 0.0, 0.0]])
    # D(0,1) = 1 K2, D(1,0) = 1 K2, D(1,1): diagonal 1 (K1) first, up 1 and left 1 not smaller -> K 2;
    # D(0,2) = 10 K3; D(1,2): diagonal D(0,1) = 1 K2, up 10, left D(1,1) = 1 not smaller -> K 3
    assert R.dtw_rows(d) == (1.0, 3)
    # swapping the sides can change K: up is tried before left, and the swap exchanges them
    d = np.array([[2.0, 2.0, 0.0, 2.0], [1.0, 1.0, 2.0, 0.0], [0.0, 1.0, 1.0, 2.0]])
    assert R.dtw_rows(d) == (6.0, 5) and R.dtw_rows(d.T) == (6.0, 4) and R.brute_force(d) == 6.0
    rs = np.random.RandomState(3)
    differ = 0
    for case in range(200):                                   # a few of 200 random small integer-valued pairs
        xa, xb = _ints(rs, 1, rs.randint(1, 9)), _ints(rs, 1, rs.randint(1, 9))
        ab, ba = R.pair(xa, xb, 'euclidean'), R.pair(xb, xa, 'euclidean')
        assert ab[1] == ba[1]
        differ += ab[2] != ba[2]
    print('K differs under a swap in %d of 200' % differ)
    assert differ >= 1


# ---- by construction -----------------------------------------------------------------------------------------------------------
def test_an_item_against_itself_and_a_zero_frame():
    rs = np.random.RandomState(4)
    for d, F in ((1, 1), (16, 7), (512, 40)):
        x = rs.randn(d, F).astype(np.float32)
        for metric in ('cosine', 'euclidean'):
            loc = R.local(x, x, metric)
            assert (np.diag(loc) == 0.0).all()
            assert R.dtw(loc) == (0.0, 0.0, F)
    x = rs.randn(8, 3).astype(np.float32)
    x[:, 1] = 0.0
    loc = R.local(x, x, 'cosine')
    assert (loc[1] == 1.0).all() and (loc[:, 1] == 1.0).all() and loc[0, 0] == 0.0


def _set_scores(noise, across=False):
    from vqvae_amd import abx
    feats, label, speaker = R.constructed(noise)
    M = len(feats)
    items = abx.Items(np.arange(M), np.zeros(M, int), [f.shape[1] for f in feats], label, speaker)
    plan = abx.plan_abx(items, across_speakers=across)
    dist = np.array([R.pair(feats[a], feats[b], 'cosine')[0] for a, b in zip(plan.pairs_a, plan.pairs_b)])
    return feats, label, speaker, plan, dist, abx.score_abx(plan, dist)


def test_the_constructed_set_is_told_apart():
    feats, label, speaker, plan, dist, sc = _set_scores(0.05)
    assert plan.tri_a.size == 576 and plan.pairs_a.size == 264
    assert sc.error == 0.0 and sc.triples.sum() == 576 and sc.errors.sum() == 0 and sc.ties.sum() == 0
    assert all(3 <= f.shape[1] <= 8 and f.shape[0] == 16 for f in feats) and len(feats) == 24
    want = R.scores(R.triples(label, speaker), lambda a, x: R.pair(feats[a], feats[x], 'cosine')[0])
    assert sc.error == want[0] and sc.by_label_pair == want[1]
    assert dict((tuple(int(v) for v in g), (int(n), int(e), int(t))) for g, n, e, t in zip(sc.groups, sc.triples, sc.errors, sc.ties)) == want[2]


def test_the_noisy_set_lies_between():
    feats, label, speaker, plan, dist, sc = _set_scores(3.0)
    print('error at noise 3.0: %.4f' % sc.error)
    assert 0.0 < sc.error < 0.5
    want = R.scores(R.triples(label, speaker), lambda a, x: R.pair(feats[a], feats[x], 'cosine')[0])
    assert sc.error == want[0] and sc.by_label_pair == want[1]


def test_identical_items_tie_everywhere():
    from vqvae_amd import abx
    label, speaker = np.repeat([0, 1, 2], 4), np.tile([0, 0, 1, 1], 3)
    items = abx.Items(np.arange(12), np.zeros(12, int), np.full(12, 5), label, speaker)
    plan = abx.plan_abx(items)
    x = np.random.RandomState(5).randn(4, 5).astype(np.float32)
    sc = abx.score_abx(plan, np.full(plan.pairs_a.size, R.pair(x, x, 'cosine')[0]))
    assert sc.error == 0.5 and (sc.ties == sc.triples).all() and sc.errors.sum() == 0
    assert all(v == 0.5 for v in sc.by_label_pair.values()) and len(sc.by_label_pair) == 6


# ---- the plan ----------------------------------------------------------------------------------------------------------------------
def _random_items(seed, M=30, contexts=True):
    from vqvae_amd import abx
    rs = np.random.RandomState(seed)
    return abx.Items(rs.randint(0, 4, M), np.zeros(M, int), np.ones(M, int), rs.randint(0, 3, M), rs.randint(0, 3, M),
                     rs.randint(0, 2, M) if contexts else None)


@pytest.mark.parametrize('across', [False, True])
@pytest.mark.parametrize('contexts', [False, True])
def test_the_plan_is_the_brute_force_s_triples(across, contexts):
    from vqvae_amd import abx
    items = _random_items(7 + contexts, contexts=contexts)
    plan = abx.plan_abx(items, across_speakers=across)
    want = R.triples(items.label, items.speaker, items.context, across)
    got = [(int(a), int(b), int(x), tuple(int(v) for v in plan.groups[g]))
           for a, b, x, g in zip(plan.tri_a, plan.tri_b, plan.tri_x, plan.tri_group)]
    assert len(got) == len(set(got)) == len(want) > 0 and set(got) == set(want)
    assert [tuple(g) for g in plan.groups.tolist()] == sorted(set(w[3] for w in want))
    # pairs: unique, ordered (side b is X), and every triple points at its own
    keys = list(zip(plan.pairs_a.tolist(), plan.pairs_b.tolist()))
    assert len(keys) == len(set(keys)) and set(keys) == set((a, x) for a, b, x, g in want) | set((b, x) for a, b, x, g in want)
    assert np.array_equal(plan.pairs_a[plan.tri_ax], plan.tri_a) and np.array_equal(plan.pairs_b[plan.tri_ax], plan.tri_x)
    assert np.array_equal(plan.pairs_a[plan.tri_bx], plan.tri_b) and np.array_equal(plan.pairs_b[plan.tri_bx], plan.tri_x)
    # the task's conditions, stated once more on the arrays
    L, S = items.label, items.speaker
    assert (plan.tri_a != plan.tri_x).all() and (L[plan.tri_a] == L[plan.tri_x]).all() and (L[plan.tri_b] != L[plan.tri_x]).all()
    assert (S[plan.tri_a] == S[plan.tri_b]).all() and ((S[plan.tri_x] != S[plan.tri_a]) == across).all()
    if contexts:
        assert (items.context[plan.tri_a] == items.context[plan.tri_x]).all() and (items.context[plan.tri_b] == items.context[plan.tri_x]).all()


def test_max_per_group_is_deterministic_in_the_seed():
    from vqvae_amd import abx
    items = _random_items(11, M=40)
    full = abx.plan_abx(items)
    one, again, other = (abx.plan_abx(items, max_per_group=3, seed=s) for s in (5, 5, 6))
    trip = lambda p: list(zip(p.tri_a.tolist(), p.tri_b.tolist(), p.tri_x.tolist()))
    assert trip(one) == trip(again) and trip(one) != trip(other) and np.array_equal(one.groups, full.groups)
    sizes = np.bincount(full.tri_group)
    assert sizes.max() > 3 and np.array_equal(np.bincount(one.tri_group), np.minimum(sizes, 3))
    for g in range(len(full.groups)):
        mine = np.nonzero(full.tri_group == g)[0]
        if mine.size > 3:
            pick = np.sort(np.random.RandomState(5).permutation(mine.size)[:3])
            assert [trip(full)[i] for i in mine[pick]] == [t for t, gg in zip(trip(one), one.tri_group) if gg == g]
    assert set(trip(one)) <= set(trip(full)) and one.pairs_a.size < full.pairs_a.size


def test_the_planner_of_the_device_calls():
    from vqvae_amd import abx
    cells = [10, 20, 5, 100, 1, 1]
    assert abx.plan_chunks(cells, 1 << 30) == [(0, 6)]
    assert abx.plan_chunks(cells, 8 * 35) == [(0, 3), (3, 4), (4, 6)]                        # 100 cells stand alone
    assert abx.plan_chunks(cells, 1) == [(i, i + 1) for i in range(6)] and abx.plan_chunks([7], 1) == [(0, 1)]


# ---- the refusals ----------------------------------------------------------------------------------------------------------------
def _fake(shape, dtype=np.float32):
    from vqvae_amd.backend import DeviceArray
    return DeviceArray(shape, dtype, _block=object(), _ptr=256)


def _fake_frames(d, tl):
    """Frames that are on the device as far as the checks can tell; every call below is refused before they are read."""
    from vqvae_amd import abx
    return abx.Frames(tl, x=_fake((d, sum(tl))), d=d, stride=sum(tl))


def test_every_refusal_names_its_offender():
    import vqvae_amd as V
    from vqvae_amd import abx
    fr = _fake_frames(8, [10, 2000, 1100])
    I = abx.Items
    ok = I([0, 0, 1], [0, 5, 0], [5, 10, 1000], [0, 1, 0], [0, 0, 0])
    refusals = (
        (I([0, 0], [0, 5], [5, 11], [0, 1]), [0], [1], 'item 1, frames [5, 11), is outside utterance 0 of 10 frames'),
        (I([0, 3], [0, 5], [5, 9], [0, 1]), [0], [1], 'item 1 names utterance 3 of 3'),
        (I([0, 0], [-1, 5], [5, 9], [0, 1]), [0], [1], 'item 0, frames [-1, 5), is outside utterance 0'),
        (I([0, 0], [0, 5], [5, 5], [0, 1]), [0], [1], 'item 1 is empty: frames [5, 5)'),
        (I([1, 2], [0, 0], [1025, 1100], [0, 1]), [0], [1], 'pair 0 has 1025 and 1100 frames; the shorter side may have at most MAX_SHORT = 1024: '
                                                               'align whole utterances with align_many'),
        (ok, [0], [3], 'ib[0] = 3 names no item of 3'),
        (ok, [0, 1], [1], '2 items on side a and 1 on side b'),
        (ok, [], [], 'no pairs'),
    )
    for items, ia, ib, words in refusals:
        with pytest.raises(ValueError, match=re.escape(words)):
            abx.pair_distances(fr, items, np.array(ia, int), np.array(ib, int))
    with pytest.raises(ValueError, match=re.escape("unknown metric 'angular'; one of cosine, euclidean")):
        abx.pair_distances(fr, ok, [0], [1], metric='angular')
    with pytest.raises(ValueError, match='chunk_bytes must be positive'):
        abx.pair_distances(fr, ok, [0], [1], chunk_bytes=0)
    with pytest.raises(ValueError, match='side a has D = 8 and side b has D = 9'):
        abx.pair_distances((fr, _fake_frames(9, [10, 2000, 1100])), ok, [0], [1])
    with pytest.raises(TypeError, match='ia must be a flat integer array'):
        abx.pair_distances(fr, ok, [0.5], [1])
    with pytest.raises(TypeError, match='fr must be a Frames'):
        abx.pair_distances(np.zeros((8, 10), np.float32), ok, [0], [1])
    with pytest.raises(TypeError, match='items must be a Items'):
        abx.pair_distances(fr, [0, 1], [0], [1])
    # more than 2^31 cells: 1024 x 2 200 000 frames
    long_fr = _fake_frames(1, [1024, 2200000])
    with pytest.raises(ValueError, match=re.escape('pair 0 has 1024 x 2200000 = 2252800000 cells; one pair may have at most 2^31')):
        abx.pair_distances(long_fr, I([0, 1], [0, 0], [1024, 2200000], [0, 1]), [0], [1])
    # the tasks
    with pytest.raises(ValueError, match='the across-speaker task needs items.speaker'):
        abx.plan_abx(I([0, 0], [0, 5], [5, 9], [0, 1]), across_speakers=True)
    with pytest.raises(ValueError, match='within_context needs items.context'):
        abx.plan_abx(ok, within_context=True)
    with pytest.raises(ValueError, match='no triple exists: the within-speaker task'):
        abx.plan_abx(I([0, 0], [0, 5], [5, 9], [0, 1], [0, 0]))                       # no second item of a label
    with pytest.raises(ValueError, match='no triple exists: the across-speaker task'):
        abx.plan_abx(ok, across_speakers=True)
    with pytest.raises(ValueError, match='max_per_group must be at least 1'):
        abx.plan_abx(ok, max_per_group=0)
    with pytest.raises(TypeError, match='items must be an Items'):
        abx.plan_abx([0, 1])
    with pytest.raises(ValueError, match='item 1, frames'):
        abx.abx(fr, I([0, 0, 0], [0, 5, 0], [5, 11, 3], [0, 1, 0]))
    with pytest.raises(ValueError, match='unknown metric'):
        abx.abx(fr, ok, metric='kl')
    with pytest.raises(TypeError, match='plan must be an ABXPlan'):
        abx.abx(fr, ok, plan=[0, 1])
    with pytest.raises(ValueError, match='the plan names item 23, there are 3'):
        abx.abx(fr, ok, plan=abx.plan_abx(abx.Items(np.arange(24), np.zeros(24, int), np.ones(24, int), np.arange(24) % 3)))
    # Items and Frames themselves
    with pytest.raises(ValueError, match='stop has 1 entries, utterance has 2'):
        I([0, 0], [0, 5], [5], [0, 1])
    with pytest.raises(TypeError, match='label must be a flat integer array'):
        I([0, 0], [0, 5], [5, 9], [0.5, 1.0])
    with pytest.raises(ValueError, match='no items'):
        I(np.zeros(0, int), np.zeros(0, int), np.zeros(0, int), np.zeros(0, int))
    with pytest.raises(ValueError, match=re.escape('D = 4097; it must be in [1, MAX_D = 4096]')):
        abx.Frames.from_latents([np.zeros((4097, 2), np.float32)])
    with pytest.raises(ValueError, match='utterance 1 has D = 7, utterance 0 has D = 8'):
        abx.Frames.from_latents([np.zeros((8, 2), np.float32), np.zeros((7, 2), np.float32)])
    with pytest.raises(ValueError, match='utterance 0 are float64, float32 needed'):
        abx.Frames.from_latents([np.zeros((8, 2))])
    with pytest.raises(ValueError, match='no utterances'):
        abx.Frames.from_latents([])
    with pytest.raises(TypeError, match='a metrics.RaggedFeatures is needed'):
        abx.Frames.from_features(np.zeros((8, 2), np.float32))
    with pytest.raises(TypeError, match='codes must be a LatentCodes'):
        abx.Frames.from_codes([0, 1], None)
    codes = V.LatentCodes([3, 2], np.array([0, 1, 2, 1, 0]), 3)
    bad = np.ones((3, 3))
    bad[2, 1] = -0.5
    with pytest.raises(ValueError, match=re.escape('table[2, 1] is -0.5; every entry must be finite and not negative')):
        abx.Frames.from_codes(codes, table=bad)
    bad[2, 1] = np.nan
    with pytest.raises(ValueError, match=re.escape('table[2, 1] is nan')):
        abx.Frames.from_codes(codes, table=bad)
    with pytest.raises(ValueError, match=re.escape('the table must be (k, k) = (3, 3) float64')):
        abx.Frames.from_codes(codes, table=np.ones((3, 4)))
    with pytest.raises(ValueError, match='the codebook or a table is needed'):
        abx.Frames.from_codes(codes)
    vq4 = types.SimpleNamespace(W=types.SimpleNamespace(data=_fake((4, 8))))
    with pytest.raises(ValueError, match='codes were taken from a codebook of k = 3, this one has k = 4'):
        abx.Frames.from_codes(codes, vq4)
    # from waves: refused before the encoder is looked at for anything but its shapes
    with pytest.raises(ValueError, match="what must be 'latents' or 'codes'"):
        abx.abx_many(None, vq4, [np.zeros(640, np.float32)], ok, what='mel')
    with pytest.raises(ValueError, match='unknown metric'):
        V.ResidentCorpus.describe([300, 300], [0, 1]).abx(None, vq4, ok, metric='angular')


def test_the_feature_buffer_is_bounded(monkeypatch):
    """abx_many names the size of the buffer it will not allocate; the encoder is only asked for its shapes."""
    from vqvae_amd import abx, frontend
    vq = types.SimpleNamespace(W=types.SimpleNamespace(data=_fake((4, 8))))
    monkeypatch.setattr(frontend, '_encoder_params', lambda enc, who: [(_fake((8, 1, 4, 1)), None)] * 6)
    items = abx.Items([0, 0, 1], [0, 5, 0], [5, 10, 9], [0, 1, 0], [0, 0, 0])
    waves = [np.zeros(64 * 10, np.float32), np.zeros(64 * 9, np.float32)]
    with pytest.raises(ValueError, match=re.escape('the latents of 19 frames take 608 bytes, feature_bytes allows 607')):
        abx.abx_many(None, vq, waves, items, feature_bytes=607)
    with pytest.raises(ValueError, match=re.escape('the codes of 19 frames take 76 bytes, feature_bytes allows 75')):
        abx.abx_many(None, vq, waves, items, what='codes', feature_bytes=75)
    with pytest.raises(ValueError, match='item 2, frames \\[0, 9\\), is outside utterance 1 of 8 frames'):
        abx.abx_many(None, vq, [waves[0], np.zeros(64 * 8, np.float32)], items)


# ---- the header abx.py binds itself ------------------------------------------------------------------------------------------------
def _code():
    text = open(HEADER).read()
    return re.sub(r'//[^\n]*', '', re.sub(r'/\*.*?\*/', '', text, flags=re.S))


def test_the_header_is_under_csrc_and_outside_the_registry():
    from vqvae_amd import _lib, abx
    assert os.path.exists(HEADER) and abx.HEADER == 'abx.h' and abx.HEADER not in os.listdir(A.INCLUDE)
    assert 'abi_version' not in open(HEADER).read()
    assert not any(n in h.prototypes for n in abx.PROTOTYPES for h in _lib.HEADERS.values())
    assert not hasattr(_lib, 'AbxDesc') and not any(n.startswith('ABX_') for n in vars(_lib))


def test_declared_functions_equal_the_bound_table():
    from vqvae_amd import abx
    declared = sorted(set(re.findall(r'\b(vqvae_[a-z0-9_]+)\s*\(', _code())))
    assert declared == sorted(abx.PROTOTYPES) and len(declared) == 7
    for name, (res, args) in abx.PROTOTYPES.items():
        found = re.findall(r'\b%s\s*\(([^()]*)\)\s*;' % name, _code())
        assert len(found) == 1, name
        params = found[0].strip()
        assert (0 if params == 'void' else len(params.split(','))) == len(args), (name, params)
    lib = abx.load()
    for name, (res, args) in abx.PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert lib.vqvae_abx_revision() == abx.REVISION == 1


def test_the_structures_and_the_macros_are_the_compiler_s(tmp_path):
    from vqvae_amd import abx
    declared = {}
    for body, name in re.findall(r'typedef\s+struct[^{;]*\{([^}]*)\}\s*(\w+)\s*;', _code()):
        declared[name] = [re.findall(r'\w+', re.sub(r'\[[^\]]*\]', '', declarator))[-1] for declaration in body.split(';')
                          if declaration.strip() for declarator in declaration.split(',')]
    mirrored = {cls._c_name_: cls for cls in abx.STRUCTS}
    assert set(declared) == set(mirrored) == {'vqvae_abx_desc', 'vqvae_abx_tables'}
    assert declared['vqvae_abx_desc'] == ['n', 'd', 'metric', 'form', 'k', 'max_short', 'ftot_a', 'ftot_b', 'stride_a', 'stride_b', 'cells']
    assert declared['vqvae_abx_tables'] == ['a_start', 'b_start', 'a_len', 'b_len', 'cell_off']
    lines = []
    for t, cls in mirrored.items():
        assert [f for f, _ in cls._fields_] == declared[t], t
        lines.append('printf("%s %%d\\n", (int)sizeof(%s));' % (t, t))
        for f, _ in cls._fields_:
            lines.append('printf("%s.%s %%d %%d\\n", (int)offsetof(%s, %s), (int)sizeof(((%s*)0)->%s));' % (t, f, t, f, t, f))
    macros = {'VQVAE_ABX_MAX_D': abx.MAX_D, 'VQVAE_ABX_MAX_K': abx.MAX_K, 'VQVAE_ABX_WAVE_SHORT': abx.WAVE_SHORT,
              'VQVAE_ABX_MAX_SHORT': abx.MAX_SHORT, 'VQVAE_ABX_LANES': abx.LANES, 'VQVAE_ABX_TILE': abx.TILE,
              'VQVAE_ABX_COSINE': abx.METRICS['cosine'], 'VQVAE_ABX_EUCLIDEAN': abx.METRICS['euclidean'],
              'VQVAE_ABX_DENSE': abx.DENSE, 'VQVAE_ABX_CODES': abx.CODES}
    assert sorted(m for m in re.findall(r'^[ \t]*#[ \t]*define[ \t]+(VQVAE_\w+)', _code(), flags=re.M) if not m.endswith('_H_')) == sorted(macros)
    lines += ['printf("%s %%d\\n", (int)(%s));' % (m, m) for m in macros]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HEADER, 'int main(void) {'] + lines + ['return 0; }', '']
    c, exe = str(tmp_path / 'abx.c'), str(tmp_path / 'abx')
    open(c, 'w').write('\n'.join(src))
    subprocess.check_call([A.host_cc(), '-std=c99', '-o', exe, c])
    out = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in subprocess.check_output([exe], universal_newlines=True).splitlines()}
    assert out['vqvae_abx_desc'] == [C.sizeof(abx.AbxDesc)] == [64] and out['vqvae_abx_tables'] == [C.sizeof(abx.AbxTables)] == [40]
    for t, cls in mirrored.items():
        for f, _ in cls._fields_:
            d = getattr(cls, f)
            assert out['%s.%s' % (t, f)] == [d.offset, d.size], (t, f)
    for m, v in macros.items():
        assert out[m] == [v], m
    assert 12 * 3 * abx.MAX_SHORT == 36864                               # the 256-lane DP's LDS at the bound: 36 KB


def test_a_bumped_revision_is_the_exact_import_error(monkeypatch):
    from vqvae_amd import _lib, abx
    monkeypatch.setattr(abx, '_bound', None)
    monkeypatch.setattr(abx, 'REVISION', 2)
    with pytest.raises(ImportError) as e:
        abx.load()
    assert str(e.value) == ('libvqvae_hip.so at %s has abx revision 1, this package binds 2: rebuild it '
                            '(__graft_entry__.build())' % _lib.LIB_PATH)
    assert abx._bound is None


def test_the_source_is_built_and_depends_on_its_header():
    srcs = re.search(r'^SRCS\s*:?=\s*(.*)$', A.make_database(), flags=re.M).group(1).split()
    assert 'abx.hip' in srcs
    assert 'abx.h' in [os.path.basename(p) for p in A.object_rule_prerequisites()]


def _good(form=0):
    from vqvae_amd import abx
    d = abx.AbxDesc()
    d.n, d.d, d.metric, d.form, d.k, d.max_short = 2, 8, 0, form, 16, 10
    d.ftot_a, d.ftot_b, d.stride_a, d.stride_b, d.cells = 30, 40, 30, 40, 200
    return d


def test_a_bad_descriptor_is_refused_on_the_host_side_of_the_library():
    """The entry points validate before they launch, so the refusals can be had without a device."""
    from vqvae_amd import abx
    lib = abx.load()
    one = C.c_void_p(256)                                                # never dereferenced: every call below is refused
    t = abx.AbxTables()
    t.a_start = t.b_start = t.a_len = t.b_len = t.cell_off = 256
    calls = {'abx_norms': lambda d: lib.vqvae_abx_norms(d, 0, one, one, None),
             'abx_local': lambda d: lib.vqvae_abx_local(d, C.byref(t), one, one, one, one, one, one, 1 << 40, None),
             'abx_dtw': lambda d: lib.vqvae_abx_dtw(d, C.byref(t), one, 1 << 40, one, one, one, None)}
    bad = (('n', 0, 'n must be at least 1'), ('d', 0, 'd must be in [1, 4096]'), ('d', 4097, 'd must be in [1, 4096]'),
           ('metric', 2, 'metric must be 0 (cosine) or 1 (euclidean)'), ('form', 2, 'form must be 0 (dense) or 1 (codes)'),
           ('ftot_a', 0, 'ftot_a and ftot_b must be at least 1'), ('stride_a', 29, 'stride_a must be at least ftot_a'),
           ('stride_b', 39, 'stride_b must be at least ftot_b'), ('max_short', 0, 'max_short must be at least 1'),
           ('max_short', 1025, 'max_short must be at most 1024 (got 1025): align whole utterances with align_many'),
           ('cells', 1, 'cells must be in [n, 2^44]'))
    for who, entry in calls.items():
        for field, value, words in bad:
            d = _good()
            setattr(d, field, value)
            rc = entry(C.byref(d))
            msg = lib.vqvae_last_error_string().decode()
            assert rc != 0 and who in msg and words in msg, (who, field, rc, msg)
            assert lib.vqvae_abx_workspace_bytes(C.byref(d)) == C.c_size_t(-1).value, field
        assert entry(None) != 0 and 'null descriptor' in lib.vqvae_last_error_string().decode()
    for value in (0, 8193):
        d = _good(form=1)
        d.k = value
        assert calls['abx_local'](C.byref(d)) != 0 and 'k must be in [1, 8192]' in lib.vqvae_last_error_string().decode()
        assert lib.vqvae_abx_workspace_bytes(C.byref(d)) == C.c_size_t(-1).value
    d = _good()
    assert lib.vqvae_abx_workspace_bytes(C.byref(d)) == 1792 == (8 * 200 + 255) // 256 * 256
    assert lib.vqvae_abx_workspace_bytes(None) == C.c_size_t(-1).value
    assert lib.vqvae_abx_local(C.byref(d), C.byref(t), one, one, one, one, None, one, 1599, None) != 0
    assert 'the workspace must hold 1600 bytes (got 1599)' in lib.vqvae_last_error_string().decode()
    assert lib.vqvae_abx_local(C.byref(d), C.byref(t), one, one, None, one, None, one, 1600, None) != 0
    assert 'the cosine metric needs the norms' in lib.vqvae_last_error_string().decode()
    assert lib.vqvae_abx_local(C.byref(d), None, one, one, one, one, None, one, 1600, None) != 0
    assert 'null tables' in lib.vqvae_last_error_string().decode()
    assert lib.vqvae_abx_local(C.byref(_good(form=1)), C.byref(t), one, one, None, None, None, one, 1600, None) != 0
    assert 'the codes form needs a table' in lib.vqvae_last_error_string().decode()
    assert lib.vqvae_abx_dtw(C.byref(d), C.byref(t), one, 1600, one, None, one, None) != 0
    assert 'abx_dtw: null cost, path_len or distance' in lib.vqvae_last_error_string().decode()
    assert lib.vqvae_abx_norms(C.byref(d), 2, one, one, None) != 0 and 'side must be 0 (a) or 1 (b)' in lib.vqvae_last_error_string().decode()
    assert lib.vqvae_abx_table_workspace_bytes(8193) == C.c_size_t(-1).value and lib.vqvae_abx_table_workspace_bytes(33) == 512
    for args, words in (((0, 8, 0), 'k must be in [1, 8192]'), ((4, 0, 0), 'd must be in [1, 4096]'), ((4, 8, 3), 'metric must be')):
        assert lib.vqvae_abx_table(*(args + (one, one, one, 1 << 20, None))) != 0
        assert 'abx_table' in lib.vqvae_last_error_string().decode() and words in lib.vqvae_last_error_string().decode()
    assert lib.vqvae_abx_table(4, 8, 0, one, one, one, 31, None) != 0 and 'must hold 32 bytes (got 31)' in lib.vqvae_last_error_string().decode()


def test_the_package_imports_without_a_library_call():
    code = ('import vqvae_amd as V, vqvae_amd._lib as L, vqvae_amd.abx as X; '
            'assert L._lib is None and X._bound is None and V.abx is X; '
            'assert all(getattr(V, n) is getattr(X, n) for n in ("Frames", "Items", "PairDistances", "ABXPlan", "ABXScores", '
            '"pair_distances", "plan_abx", "abx_many", "code_table")); '
            'assert V.CorpusView.abx is V.ResidentCorpus.abx and callable(X.abx)')
    env = dict(os.environ, PYTHONPATH=os.path.join(A.ROOT, 'chainer-vq-vae_amd'))
    subprocess.check_call([sys.executable, '-c', code], env=env)


def test_the_front_end_is_untouched():
    """abx_many uses the hook frontend._run already has; its driver launches nothing new without one."""
    import inspect
    from vqvae_amd import abx, frontend
    assert inspect.signature(frontend._run).parameters['hook'].default is None
    text = inspect.getsource(abx._from_waves)
    assert 'frontend._run(' in text and 'hook=keep' in text
