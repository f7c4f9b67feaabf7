"""Duration-penalised quantisation on the device (vqvae_amd.segmental, csrc/segmental.h, csrc/segmental.hip) against the
NumPy restatement of the rule (tests/segmental_ref.py).  The rule is float64 ``- * + min`` in one written order, so EVERY
comparison with the restatement is a bit equality: the table D, the codes, n_seg and cost, in every arrangement of the
list; answers known without the restatement; red zones round every output and an exactly sized, poisoned workspace.

The distance kernel tiles 64 frames x 64 codes and stages 32 channels at a time: the shapes straddle all three.  The DP
has one kernel per register block: one wavefront with 1, 2, 4 or 8 codes a lane up to SEG_WAVE_K = 512 codes, 256 lanes
with 4, 8, 16 or 32 above; the codebook sizes below take every one of them.  The backtrack looks at 64 frames at a time:
the utterance lengths and the planted constant runs put their ends before, on and behind that window's edge."""
import ctypes as C

import numpy as np
import pytest

import segmental_ref as R
import zoned as Z
from vqvae_amd import _lib, segmental
from vqvae_amd.utils import VQ

pytestmark = pytest.mark.gpu
WAVE_K = segmental.WAVE_K
D_DP = 8                                                   # channels of the DP cases
PEN = [D_DP / 8.0 * s for s in (0.0, 1.0, 8.0, 1e6)]      # [0, small, middle, huge], scaled to the data
LENGTHS = [1, 2, 63, 64, 65, 129]
RUNS = [1, 63, 64, 65, 200, 1, 7]                          # planted constant runs: the jumps cross the window's edges


def _vq(W):
    W = np.ascontiguousarray(W, np.float32)
    vq = VQ(W.shape[0], W.shape[1])
    vq.W.data = W.copy()
    vq.to_gpu()
    return vq


def _gauss(d, k, lengths, seed):
    rs = np.random.default_rng(seed)
    return [rs.standard_normal((d, T)).astype(np.float32) for T in lengths], rs.standard_normal((k, d)).astype(np.float32)


def _constant_runs(d, runs, seed):
    """Frames that repeat one random vector per run, so that D's rows repeat and the path stays for the whole run."""
    rs = np.random.default_rng(seed)
    return np.concatenate([np.repeat(rs.standard_normal((d, 1)), n, axis=1) for n in runs], axis=1).astype(np.float32)


def _same(seg, want, utts=None, at=None, what=''):
    """Device result against restated (codes, n_seg, cost) per penalty and utterance; ``utts``: positions in ``want`` of
    the utterances of ``seg``."""
    host = [c.to_host() for c in seg.codes]
    for p in range(len(seg.penalties)):
        for i in range(len(seg)):
            codes, n_seg, cost = want[p][i if utts is None else utts[i]]
            assert host[p][i].dtype == np.int32 and np.array_equal(host[p][i], codes), (what, p, i)
            assert seg.n_segments[p, i] == n_seg and seg.cost[p, i] == cost, (what, p, i, seg.cost[p, i], cost)


# ---- the distance table ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [1, 2, 63, 64, 65, 128, 513])
@pytest.mark.parametrize('d', [1, 3, 64, 512])
def test_the_table_equals_the_restatement(gpu, d, k):
    for seed, frames in enumerate(([1, 2, 3, 70], [300, 1, 255, 257, 2])):
        latents, W = _gauss(d, k, frames, 100 * d + k + seed)
        got = segmental.distance_table(_vq(W), latents)
        for i, z in enumerate(latents):
            want = R.distances(z, W)
            assert got[i].dtype == np.float64 and got[i].shape == (frames[i], k)
            assert np.array_equal(got[i], want), (d, k, frames, i, np.abs(got[i] - want).max())


def test_the_table_at_the_largest_codebook(gpu):
    latents, W = _gauss(8, 8192, [1, 5], 7)
    got = segmental.distance_table(_vq(W), [latents[0], gpu.to_device(latents[1])])       # a device array beside a host one
    for i, z in enumerate(latents):
        assert np.array_equal(got[i], R.distances(z, W)), i


# ---- the DP -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [1, 31, 32, 33, 64, 65, 128, WAVE_K, WAVE_K + 1, 8192])
def test_the_codes_equal_the_restatement(gpu, k):
    lengths = [1, 2, 5] if k == 8192 else LENGTHS
    latents, W = _gauss(D_DP, k, lengths, 300 + k)
    if k != 8192:
        latents.append(_constant_runs(D_DP, RUNS, 400 + k))
    seg = segmental.segment_latents(_vq(W), latents, PEN)
    want = R.segment(latents, W, PEN)
    _same(seg, want, what='k %d' % k)
    assert seg.n_segments.shape == seg.cost.shape == (4, len(latents)) and seg.indices.shape == (4, sum(z.shape[1] for z in latents))
    assert (seg.n_segments[3] == 1).all() and (seg.n_segments[0] >= seg.n_segments[1]).all()
    if k not in (1, 8192):
        runs = seg.codes[2].to_host()[-1]                                # the middle penalty on the planted runs
        print('k %d: segments per penalty %r; planted-run utterance %r' % (k, seg.n_segments.sum(axis=1).tolist(), seg.n_segments[:, -1].tolist()))
        assert seg.n_segments[2, -1] <= len(RUNS) and len(runs) == sum(RUNS)


def test_a_long_utterance(gpu):
    """5 000 frames at d = 8, k = 128, beside a short one: 78 windows of the backtrack, four penalties."""
    latents, W = _gauss(D_DP, 128, [5000, 3], 21)
    seg = segmental.segment_latents(_vq(W), latents, PEN)
    _same(seg, R.segment(latents, W, PEN), what='long')
    print('segments of the 5000 frames per penalty: %r' % seg.n_segments[:, 0].tolist())
    assert seg.n_segments[0, 0] > seg.n_segments[1, 0] > seg.n_segments[2, 0] > seg.n_segments[3, 0] == 1


# ---- composition independence ---------------------------------------------------------------------------------------------------
class Case(object):
    pass


@pytest.fixture(scope='module')
def case(gpu):
    """Computed once and left unchanged: a list at k = 65 (two codes a lane, the second word nearly empty) and its
    restatement."""
    c = Case()
    c.latents, c.W = _gauss(D_DP, 65, [40, 1, 129, 64, 7, 200], 55)
    c.latents.append(_constant_runs(D_DP, RUNS, 56))
    c.vq = _vq(c.W)
    c.want = R.segment(c.latents, c.W, PEN)
    c.whole = segmental.segment_latents(c.vq, c.latents, PEN)
    return c


def test_an_utterance_is_the_same_in_every_arrangement(case, gpu):
    c = case
    n = len(c.latents)
    _same(c.whole, c.want, what='whole')
    for i in (0, 2, n - 1):                                                                     # alone
        _same(segmental.segment_latents(c.vq, [c.latents[i]], PEN), c.want, [i], what='alone %d' % i)
    order = list(range(n))[::-1]                                                                # reversed: first is last
    _same(segmental.segment_latents(c.vq, [c.latents[i] for i in order], PEN), c.want, order, what='reversed')
    mixed, where = [], []                                                                       # beside neighbours scaled by 1 000
    for i in range(n):
        mixed += [(1000.0 * c.latents[(i + 1) % n]).astype(np.float32), gpu.to_device(c.latents[i])]
        where += [None, i]
    seg = segmental.segment_latents(c.vq, mixed, PEN)
    host = [x.to_host() for x in seg.codes]
    for j, i in enumerate(where):
        if i is not None:
            for p in range(4):
                codes, n_seg, cost = c.want[p][i]
                assert np.array_equal(host[p][j], codes) and seg.n_segments[p, j] == n_seg and seg.cost[p, j] == cost, (i, p)


def test_the_result_does_not_depend_on_chunk_bytes(case, gpu):
    c = case
    per = segmental.frame_bytes(65, 4) + 4 * D_DP
    for chunk_bytes in (1, 130 * per, 300 * per):                                               # one utterance a run; a few
        runs = segmental.plan_runs([z.shape[1] for z in c.latents], per, chunk_bytes)
        assert len(runs) > 1
        _same(segmental.segment_latents(c.vq, c.latents, PEN, chunk_bytes=chunk_bytes), c.want, what='chunk_bytes %d' % chunk_bytes)
    # the sub-runs the module plans inside one chunk of the front end: the whole list as one z, cut by the table's bytes
    tl = [z.shape[1] for z in c.latents]
    job = segmental._Job('test', c.vq.W.data, np.array(PEN), tl, 130 * segmental.frame_bytes(65, 4))
    assert len(segmental.plan_runs(tl, segmental.frame_bytes(65, 4), job.chunk_bytes)) > 2
    z = gpu.to_device(np.concatenate(c.latents, axis=1))
    job.chunk(z.ptr, sum(tl), 0, len(tl))
    _same(job.result(), c.want, what='sub-runs')


def test_penalties_in_one_call_equal_one_call_each(case):
    c = case
    for p, lam in enumerate(PEN):
        one = segmental.segment_latents(c.vq, c.latents, lam)                                   # a scalar: P = 1
        assert one.penalties.tolist() == [lam] and one.indices.shape[0] == 1
        _same(one, [c.want[p]], what='penalty %r alone' % lam)
    _same(segmental.segment_latents(c.vq, c.latents, PEN[::-1] + [0.25] * 12), [c.want[p] for p in (3, 2, 1, 0)] + R.segment(c.latents, c.W, [0.25] * 12),
          what='sixteen penalties')


# ---- answers known without the restatement --------------------------------------------------------------------------------------
def test_a_planted_segmentation_is_returned(gpu):
    runs = [(2, 1), (0, 63), (3, 64), (1, 65), (0, 200), (2, 1), (3, 5)]
    W, z, planted = R.planted(4, 8, runs, spacing=4.0, noise=0.05, seed=3)
    lam = 2.0                                                            # between the noise (8 * 0.05^2) and the spacing (2 * 4^2)
    codes, n_seg, cost = R.viterbi(R.distances(z, W), lam)
    assert np.array_equal(codes, planted) and n_seg == len(runs)         # the restatement recovers it on the CPU: first
    seg = segmental.segment_latents(_vq(W), [z, z[:, :64].copy()], lam)
    got = seg.codes[0].to_host()
    assert np.array_equal(got[0], planted) and np.array_equal(got[1], planted[:64]) and seg.n_segments.tolist() == [[len(runs), 2]]


def test_a_huge_penalty_gives_the_one_best_code(case):
    c = case
    host = c.whole.codes[3].to_host()
    for i, z in enumerate(c.latents):
        D = R.distances(z, c.W)
        sums = np.zeros(D.shape[1])
        for t in range(D.shape[0]):
            sums = sums + D[t]
        assert (host[i] == int(np.argmin(sums))).all() and c.whole.n_segments[3, i] == 1 and c.whole.cost[3, i] == sums.min(), i


def test_penalty_zero_is_the_quantiser(gpu):
    """Standard normals of default_rng(0) at (d, k, T) = (8, 16, 300), z drawn before W: the smallest relative float64
    margin between a frame's best and second-best code is 1.07e-3 (measured on the host), so the float32 search of
    encode_many's quantiser must agree on every frame; none is left out."""
    from vqvae_amd.utils import StraightThrough
    rs = np.random.default_rng(0)
    z, W = rs.standard_normal((8, 300)).astype(np.float32), rs.standard_normal((16, 8)).astype(np.float32)
    D = np.sort(R.distances(z, W), axis=1)
    margin = ((D[:, 1] - D[:, 0]) / D[:, 1]).min()
    print('smallest margin %.3g' % margin)
    assert margin > 1e-4
    vq = _vq(W)
    seg = segmental.segment_latents(vq, [z], 0.0)
    zd, idx = gpu.to_device(z), gpu.DeviceArray((300,), np.int32)
    lib = _lib.load()
    ws = gpu.workspace(lib.vqvae_vq_workspace_bytes(1, 8, 300, 16))
    _lib.call('vqvae_vq_nearest_fwd', zd.ptr, vq.W.data.ptr, 1, 8, 300, 16, StraightThrough.mode, idx.ptr, None, None, ws.ptr,
              ws.nbytes, gpu.stream())
    assert np.array_equal(seg.codes[0].to_host()[0], idx.get())
    assert seg.cost[0, 0] == np.add.accumulate(D[:, 0])[-1] and seg.distortion[0, 0] == seg.cost[0, 0]


def test_exact_ties_on_the_device(gpu):
    pen = [0.0, 1.0, 2.0]
    seg = segmental.segment_latents(_vq(R.TIE_W), R.TIE_Z, pen)
    _same(seg, R.segment(R.TIE_Z, R.TIE_W, pen), what='ties')
    assert [h.tolist() for h in seg.codes[0].to_host()] == [[0, 2, 0, 4, 4, 4, 2], [0], [0, 0, 0, 0]]
    W2 = np.array([[0], [2]], np.float32)
    two = segmental.segment_latents(_vq(W2), [np.array([[2, 0]], np.float32)], [4.0, 3.0])
    assert [c.to_host()[0].tolist() for c in two.codes] == [[0, 0], [1, 0]] and two.cost.tolist() == [[4.0], [3.0]]
    assert two.n_segments.tolist() == [[1], [2]] and two.distortion.tolist() == [[4.0], [0.0]]


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def test_waves_end_to_end(gpu):
    import vqvae_amd as V
    import codestats_ref as CR
    from vqvae_amd.net import ConditionEmbed, Encoder
    rs = np.random.RandomState(77)
    d, k = 16, 24
    enc, vq = Encoder(d), VQ(k, d)
    vq.W.data = (0.02 * rs.standard_normal((k, d))).astype(np.float32)
    enc.to_gpu()
    vq.to_gpu()
    waves = [(0.5 * rs.standard_normal(64 * tl + 13) * np.sin(np.arange(64 * tl + 13) / 50.0)).astype(np.float32) for tl in (30, 41, 7, 64, 22, 35)]
    latents = V.encode_many(enc, vq, waves, return_latents=True)[1]
    scale = float(np.median([R.distances(z, vq.W.data.get()).min(axis=1).mean() for z in latents]))
    pen = [0.0, 0.02 * scale, 0.5 * scale]
    want = segmental.segment_latents(vq, latents, pen)
    _same(want, R.segment(latents, vq.W.data.get(), pen), what='latents')
    seg = V.segment_many(enc, vq, waves, pen)
    small = V.segment_many(enc, vq, waves, pen, chunk_bytes=60 * segmental.frame_bytes(k, 3))   # several chunks, several sub-runs
    for got in (seg, small):
        assert got.tl.tolist() == [30, 41, 7, 64, 22, 35] and got.k == k
        assert np.array_equal(got.indices.get(), want.indices.get())
        assert np.array_equal(got.n_segments, want.n_segments) and np.array_equal(got.cost, want.cost)
    print('segments per penalty %r, mean run %r' % (seg.n_segments.sum(axis=1).tolist(), seg.mean_run.tolist()))
    assert (seg.n_segments[0] >= seg.n_segments[1]).all() and (seg.n_segments[1] >= seg.n_segments[2]).all()
    # a corpus read in place, and a reordered view of it, against segment_many on the corpus's own samples
    speakers = np.array([0, 1, 2, 0, 1, 2], np.int32)
    corpus = V.ResidentCorpus(waves, speakers)
    flat = corpus.samples.get()
    own = [flat[int(o):int(o) + int(L)].copy() for o, L in zip(corpus.offsets, corpus.lengths)]
    host = V.segment_many(enc, vq, own, pen)
    in_place = corpus.segment(enc, vq, pen)
    assert np.array_equal(in_place.indices.get(), host.indices.get()) and np.array_equal(in_place.cost, host.cost)
    view = corpus.subset([4, 0, 5])
    part = view.segment(enc, vq, pen[1])
    for j, i in enumerate([4, 0, 5]):
        assert np.array_equal(part.codes[0].to_host()[j], host.codes[1].to_host()[i]) and part.cost[0, j] == host.cost[1, i]
    # codes[p] is a LatentCodes like any other
    for p in range(3):
        codes = seg.codes[p]
        hostp = codes.to_host()
        runs = V.collapse_many(codes, max_run=8)
        assert runs.lengths.tolist() == seg.n_segments[p].tolist()
        for i, (u, dur) in enumerate(runs.to_host()):
            wu, wd = CR.runs(hostp[i])
            assert np.array_equal(u, wu) and np.array_equal(dur, wd)
        st = V.code_stats(codes, speakers, 3, collapsed=True)
        assert st.uni.sum() == seg.n_segments[p].sum() and st.invalid == 0
        assert np.array_equal(st.uni, CR.counts_loops([CR.runs(h)[0] for h in hostp], speakers, k, 3)[0])
    embed, cin = ConditionEmbed(3, 4, 8), d
    for i in range(1, 6):
        conv = getattr(embed, 'local_embed%d' % i)
        conv.W.data = (0.2 * rs.standard_normal((8, cin, 3, 1))).astype(np.float32)
        conv.b.data = (0.1 * rs.standard_normal(8)).astype(np.float32)
        cin = 8
    embed.to_gpu()
    cond = V.condition_many(vq, embed, seg.codes[2], speakers)
    again = V.condition_many(vq, embed, V.LatentCodes(seg.tl, np.concatenate(seg.codes[2].to_host()), k), speakers)
    assert np.array_equal(cond.local.get(), again.local.get()) and cond.tl.tolist() == seg.tl.tolist()


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def _desc(n, d, k, P, ttot, pen, code_stride=None, utt_stride=None):
    s = segmental.SegDesc()
    s.n, s.d, s.k, s.n_pen, s.ttot, s.stride = n, d, k, P, ttot, ttot
    s.code_stride, s.utt_stride = ttot if code_stride is None else code_stride, n if utt_stride is None else utt_stride
    for q, v in enumerate(pen):
        s.lam[q] = v
    return s


@pytest.mark.parametrize('k', [65, WAVE_K + 1])
def test_every_entry_point_writes_inside_its_outputs(gpu, k):
    """Red zones round every output and round a workspace of exactly the queried size, poisoned; both DP forms."""
    lib = segmental.load()
    frames = [1, 64, 70, 5]
    latents, W = _gauss(D_DP, k, frames, 900 + k)
    z = np.concatenate(latents, axis=1)
    off = np.concatenate([[0], np.cumsum(frames)]).astype(np.int64)
    n, ttot, pen = len(frames), int(off[-1]), [0.0, 1.0, 8.0]
    d = _desc(n, D_DP, k, 3, ttot, pen)
    need = lib.vqvae_seg_workspace_bytes(C.byref(d))
    assert 0 < need <= ttot * segmental.frame_bytes(k, 3) + 3 * 255
    st = gpu.stream
    want = R.segment(latents, W, pen)

    out = Z.run_contract(gpu, lambda b: segmental.call('vqvae_seg_distances', C.byref(d), b.z.ptr, b.W.ptr, b.table.ptr, st()),
                         dict(z=Z.In(z), W=Z.In(W), table=Z.Out((ttot, k), np.float64)))
    assert np.array_equal(out['table'], np.concatenate([R.distances(x, W) for x in latents]))

    def run(b):
        segmental.call('vqvae_seg_segment', C.byref(d), b.z.ptr, b.W.ptr, b.off.ptr, b.codes.ptr, b.n_seg.ptr, b.cost.ptr,
                       b.ws.ptr, need, st())

    out = Z.run_contract(gpu, run, dict(z=Z.In(z), W=Z.In(W), off=Z.In(off), codes=Z.Out((3, ttot), np.int32),
                                        n_seg=Z.Out((3, n), np.int32), cost=Z.Out((3, n), np.float64), ws=Z.Ws(need)))
    for p in range(3):
        assert np.array_equal(out['codes'][p], np.concatenate([w[0] for w in want[p]]))
        assert out['n_seg'][p].tolist() == [w[1] for w in want[p]] and out['cost'][p].tolist() == [w[2] for w in want[p]]

    # rows of the outputs further apart than they are long: the elements between the rows keep their bits
    wide = _desc(n, D_DP, k, 3, ttot, pen, code_stride=ttot + 9, utt_stride=n + 3)
    cv, uv = np.zeros((3, ttot + 9), bool), np.zeros((3, n + 3), bool)
    cv[:, :ttot], uv[:, :n] = True, True

    def run_wide(b):
        segmental.call('vqvae_seg_segment', C.byref(wide), b.z.ptr, b.W.ptr, b.off.ptr, b.codes.ptr, b.n_seg.ptr, b.cost.ptr,
                       b.ws.ptr, need, st())

    out = Z.run_contract(gpu, run_wide, dict(z=Z.In(z), W=Z.In(W), off=Z.In(off), codes=Z.Out((3, ttot + 9), np.int32, valid=cv),
                                             n_seg=Z.Out((3, n + 3), np.int32, valid=uv),
                                             cost=Z.Out((3, n + 3), np.float64, valid=uv), ws=Z.Ws(need)))
    assert np.array_equal(out['codes'][1, :ttot], np.concatenate([w[0] for w in want[1]]))
    assert out['cost'][2, :n].tolist() == [w[2] for w in want[2]]


def test_a_contradicting_frame_off_is_skipped_and_marked(gpu):
    lib = segmental.load()
    k, frames = 33, [20, 30, 40]
    latents, W = _gauss(D_DP, k, frames, 970)
    zd, Wd = gpu.to_device(np.concatenate(latents, axis=1)), gpu.to_device(W)
    n, ttot, pen = 3, 90, [0.0, 2.0]
    want = R.segment(latents, W, pen)
    d = _desc(n, D_DP, k, 2, ttot, pen)
    need = lib.vqvae_seg_workspace_bytes(C.byref(d))
    ws = gpu.DeviceArray((need,), np.uint8)

    def run(off):
        codes, n_seg, cost = gpu.DeviceArray((2, ttot), np.int32), gpu.DeviceArray((2, n), np.int32), gpu.DeviceArray((2, n), np.float64)
        codes.set(np.full((2, ttot), 7777, np.int32))
        segmental.call('vqvae_seg_segment', C.byref(d), zd.ptr, Wd.ptr, gpu.to_device(np.array(off, np.int64)).ptr, codes.ptr,
                       n_seg.ptr, cost.ptr, ws.ptr, need, gpu.stream())
        return codes.get(), n_seg.get(), cost.get()

    codes, n_seg, cost = run([0, 20, 50, 90])                                       # the table that agrees
    assert n_seg.tolist() == [[w[1] for w in want[p]] for p in range(2)]
    codes, n_seg, cost = run([0, 20, 20, 90])                                       # utterance 1 owns no frame: skipped
    third = R.viterbi(R.distances(np.concatenate(latents[1:], axis=1), W), 2.0)     # ... and 2 owns [20, 90)
    assert n_seg[1].tolist() == [want[1][0][1], 0, third[1]] and np.isnan(cost[:, 1]).all() and cost[1, 2] == third[2]
    assert np.array_equal(codes[1, :20], want[1][0][0]) and np.array_equal(codes[1, 20:], third[0])
    codes, n_seg, cost = run([0, 20, 50, 91])                                       # the end contradicts ttot: every utterance
    assert (n_seg == 0).all() and np.isnan(cost).all() and (codes == -1).all()
    codes, n_seg, cost = run([1, 20, 50, 90])                                       # the start is not 0
    assert (n_seg == 0).all() and np.isnan(cost).all() and (codes[:, 1:] == -1).all() and (codes[:, 0] == 7777).all()
    codes, n_seg, cost = run([0, 50, 20, 90])                                       # a descending entry: skipped, nothing marked
    assert n_seg[0, 1] == 0 and np.isnan(cost[0, 1]) and n_seg[0, 0] >= 1 and n_seg[0, 2] >= 1
    assert ((codes >= 0) & (codes < k)).all()


def test_a_bad_descriptor_is_refused_without_a_launch(gpu):
    lib = segmental.load()
    n, dd, k, ttot = 2, 4, 8, 10
    bufs = dict((name, Z.ZonedArray(gpu, shape=s, dtype=t, name=name)) for name, s, t in (
        ('codes', (2, ttot), np.int32), ('n_seg', (2, n), np.int32), ('cost', (2, n), np.float64), ('table', (ttot, k), np.float64),
        ('ws', (4096,), np.uint8)))
    z, W, off = gpu.to_device(np.zeros((dd, ttot), np.float32)), gpu.to_device(np.zeros((k, dd), np.float32)), gpu.to_device(np.array([0, 4, 10], np.int64))
    good = lambda: _desc(n, dd, k, 2, ttot, [0.0, 1.0])
    assert lib.vqvae_seg_workspace_bytes(C.byref(good())) <= 4096

    def segment(d, ws_bytes=4096, codes=bufs['codes'].ptr):
        return 'seg_segment', lib.vqvae_seg_segment(d, z.ptr, W.ptr, off.ptr, codes, bufs['n_seg'].ptr, bufs['cost'].ptr,
                                                    bufs['ws'].ptr, ws_bytes, gpu.stream())

    def distances(d):
        return 'seg_distances', lib.vqvae_seg_distances(d, z.ptr, W.ptr, bufs['table'].ptr, gpu.stream())

    def refused(result, words):
        who, rc = result
        msg = lib.vqvae_last_error_string().decode()
        assert rc != 0 and who in msg and words in msg, (who, rc, msg, words)

    for field, value, words in (('n', 0, 'n must be at least 1'), ('d', 0, 'd must be at least 1'), ('k', 0, 'k must be in [1, 8192]'),
                                ('k', 8193, 'k must be in [1, 8192]'), ('n_pen', 0, 'n_pen must be in [1, 16]'), ('n_pen', 17, 'n_pen must be in [1, 16]'),
                                ('ttot', 1, 'ttot must be at least n'), ('stride', 9, 'stride must be at least ttot'),
                                ('code_stride', 9, 'code_stride must be at least ttot'), ('utt_stride', 1, 'utt_stride must be at least n')):
        for entry in (segment, distances):
            d = good()
            setattr(d, field, value)
            refused(entry(C.byref(d)), words)
    for value in (-1.0, float('nan'), float('inf')):
        d = good()
        d.lam[1] = value
        refused(segment(C.byref(d)), 'every penalty must be finite and not negative')
    refused(segment(None), 'null descriptor')
    refused(segment(C.byref(good()), ws_bytes=64), 'the workspace must hold')
    refused(segment(C.byref(good()), codes=None), 'seg_segment: null')
    gpu.synchronize()
    for name, zb in bufs.items():                           # nothing ran: every payload still holds its poison, every zone its pattern
        zb.check()
        assert np.array_equal(zb.arr.get().view(np.uint8).reshape(-1), zb.initial), name
