"""Held-out likelihood of mixture-of-logistics decoders on the device (vqvae_amd.scoring_mol, csrc/ragged_mol.h,
csrc/ragged_mol.hip).

1. vqvae_rdmol_nll alone against _mol_terms in float64 over the values it was handed, at chain_accuracy_ref.bar(e32), e32
   NumPy's float32 evaluation of the same function; ragged layouts with segment borders inside and at the edge of a
   256-column block, M = 1, 10 and 16.
2. Its branches on the reference's crafted input (tests/golden/ref_mol_loss.npz): both tails, both sides of +-0.999, clamped
   log-scales, a saturated term.
3. vqvae_rdmol_embed alone: BIT equality with scoring_mol_ref.embed_bits.
4. Both entry points under zoned.run_contract, and every C-side refusal with nothing written.
5. Composition independence as BIT equality of per-sample NLL, nll and count: alone / reversed / beside replaced
   neighbours / three chunks against one / the smallest chunks / a ResidentCorpus read in place / a reversed CorpusView /
   evaluate_many_mol against its two halves.
6. Values: per-sample NLL, params and nll against the float64 restatement (tests/scoring_mol_ref.py) at the project's 1e-4.
7. The reference's own model and batch (tests/golden/ref_model_mol.npz): nll / count against its loss1.
8. The tie to the device's training path: VAE.__call__'s loss1 on B = 1.

Models (O.make_params): m40s reads raw samples (embed (40, 1, 2)), m40q mu-law classes (embed (40, 37, 2)); every row edge is
off a tile.  A randomly initialised head would put every component at the 1e-12 floor of cdf_plus - cdf_min and the values
test would compare constants, so proj2 is spread (spread_head) and the test ASSERTS that no position is at the floor."""
import ctypes as C

import numpy as np
import pytest

import call_accuracy_ref as CA
import chain_accuracy_ref as A
import helpers as H
from helpers import _bits
import ref_model as RM
import scoring_mol_ref as R
import vqvae_oracle as O
from zoned import In, Out, run_contract

pytestmark = pytest.mark.gpu

TOL = 1e-4
UP = 64
N_SPEAKER = 3
# name -> (R, D, S, Cl, G, Qin, M, n_loop, n_layer, tl, seed)
MODELS = {'m40s': (40, 48, 24, 24, 8, 1, 10, 2, 3, [1, 3, 2, 1, 5, 2], 12),
          'm40q': (40, 48, 24, 24, 8, 37, 3, 2, 3, [1, 3, 2], 14)}
ENC_D, ENC_K = 16, 8


def lengths_for(tl):
    return [64 * t if i % 2 == 0 else 64 * t + 1 + i for i, t in enumerate(tl)]


def spread_head(P, M):
    """proj2 of a head whose mixture covers the sample range: the mean rows' weights times 20, their biases
    linspace(-100, 100, M), the log-scale rows' biases 3.0."""
    W, b = P['decoder']['proj2']
    W[M:2 * M] *= 20.0
    b[M:2 * M] = np.linspace(-100.0, 100.0, M)
    b[2 * M:] = 3.0


_CASES = {}


def case(name):
    """Everything of a model that the CPU makes, once: parameters, waves, latent blocks, speaker vectors and the float64
    restatement of every utterance."""
    if name not in _CASES:
        Rr, D, S, Cl, G, Qin, M, n_loop, n_layer, tl, seed = MODELS[name]
        rs = np.random.RandomState(seed)
        P = O.make_params(rs, d=ENC_D, k=ENC_K, n_loop=n_loop, n_layer=n_layer, input_dim=Qin, residual=Rr, dilated=D, skip=S,
                          out_dim=3 * M, local_dim=Cl, global_dim=G, n_speaker=N_SPEAKER)
        H.named_tweak('biases:%d' % seed)(P)
        spread_head(P, M)
        Ls = lengths_for(tl)
        waves = [O.synth_batch(1, length=L - 1, n_speaker=N_SPEAKER, seed=500 + 7 * i + seed)[0].reshape(-1).copy() for i, L in enumerate(Ls)]
        local = [np.maximum(rs.standard_normal((Cl, t)), 0).astype(np.float32) for t in tl]
        gvec = rs.standard_normal((len(tl), G)).astype(np.float32)
        ref = [R.score_utterance_mol(P['decoder'], w, lo, g, n_loop, n_layer, UP) for w, lo, g in zip(waves, local, gvec)]
        for a in waves + local + [gvec]:
            a.setflags(write=False)
        _CASES[name] = dict(P=P, waves=waves, local=local, gvec=gvec, ref=ref, tl=tl, L=Ls,
                            speakers=np.array([(2 * i + 1) % N_SPEAKER for i in range(len(tl))], np.int32))
    return _CASES[name]


def wavenet_link(name):
    from vqvae_amd.wavenet import WaveNet
    Rr, D, S, Cl, G, Qin, M, n_loop, n_layer = MODELS[name][:9]
    wn = WaveNet(n_loop, n_layer, 2, Qin, Rr, D, S, 256, True, 3 * M, -40, Cl + G, 0)
    named = dict(wn.namedparams())
    for n, arr in O.flatten_params(case(name)['P']['decoder']):
        p = named[n.replace('/blocks/', '/resnet/')]
        p.data = np.ascontiguousarray(arr.reshape(arr.shape + (1,) if arr.ndim == 3 else arr.shape), np.float32).copy()
    wn.to_gpu()
    return wn


def front_links(name):
    from vqvae_amd.net import ConditionEmbed, Encoder
    from vqvae_amd.utils import VQ
    P = case(name)['P']
    Cl, G = MODELS[name][3:5]
    enc, vq, ce = Encoder(ENC_D), VQ(ENC_K, ENC_D), ConditionEmbed(N_SPEAKER, G, Cl)
    for grp, link in (('encoder', enc), ('condition_embed', ce)):
        for n, v in P[grp].items():
            if isinstance(v, tuple):
                conv = getattr(link, n)
                conv.W.data = np.ascontiguousarray(v[0][..., None], np.float32).copy()
                conv.b.data = np.ascontiguousarray(v[1], np.float32).copy()
    ce.global_embed.W.data = P['condition_embed']['global_embed'].copy()
    vq.W.data = P['vq'].copy()
    for link in (enc, vq, ce):
        link.to_gpu()
    return enc, vq, ce


def condition(gpu, local, gvec):
    import vqvae_amd as V
    return V.LatentCondition.from_latents([gpu.to_device(a) for a in local], gpu.to_device(np.ascontiguousarray(gvec)), UP)


def same_utterance(got, i, want, k, what):
    a, b = got.sample_nll(i), want.sample_nll(k)
    assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), \
        '%s: the per-sample NLL differs in %d of %d positions' % (what, int((_bits(a) != _bits(b)).sum()) if a.shape == b.shape else -1, b.size)
    assert _bits(got.nll[i:i + 1])[0] == _bits(want.nll[k:k + 1])[0], '%s: nll %r against %r' % (what, got.nll[i], want.nll[k])
    assert got.count[i] == want.count[k], '%s: count differs' % what


# ---- direct calls -----------------------------------------------------------------------------------------------------------------
class Ragged(object):
    """n_i columns per utterance and, per utterance, n_i + 1 samples placed in one buffer `w` at `woff` (with gaps of poison
    between them when asked, in any order)."""

    def __init__(self, counts, Rr=8, Q=30):
        from vqvae_amd import _lib
        self.n = np.asarray(counts, np.int64)
        self.off = np.concatenate([[0], np.cumsum(self.n)]).astype(np.int64)
        self.T = int(self.off[-1])
        self.desc = _lib.RdecDesc(len(counts), Rr, 8, 8, Q, 4, 0, 1, UP, 0, self.T, len(counts))

    def place(self, waves, order=None, gap=0):
        """(w, woff): wave i (n_i + 1 samples) at woff[i]; `order` is the order they lie in, `gap` NaNs between them."""
        order = list(range(len(waves))) if order is None else list(order)
        woff, parts, at = np.zeros(len(waves), np.int64), [], 0
        for i in order:
            parts.append(np.full(gap, np.nan, np.float32))
            woff[i] = at + gap
            parts.append(np.asarray(waves[i], np.float32))
            at += gap + len(waves[i])
        return np.concatenate(parts + [np.full(gap, np.nan, np.float32)]), woff

    def tables(self, b):
        from vqvae_amd import _lib
        return C.byref(_lib.RdecTables(b.off.ptr, None, None, None))

    def seg(self, i):
        return slice(int(self.off[i]), int(self.off[i + 1]))


def _nll_on_device(gpu, g, y, w, woff, M, zoned=True):
    from vqvae_amd import scoring_mol
    d = C.byref(g.desc)
    fn = lambda b: scoring_mol.call('vqvae_rdmol_nll', d, g.tables(b), b.y.ptr, b.w.ptr, b.woff.ptr, M, 256, -40.0, b.nll.ptr, gpu.stream())
    return run_contract(gpu, fn, dict(off=In(g.off), y=In(y), w=In(w), woff=In(woff), nll=Out((g.T,))))['nll']


def _judge(what, got, y, t):
    """err <= bar(e32) in both metrics; prints err / e32."""
    w64 = R.mol_nll(y.astype(np.float64), t.astype(np.float64))[0]
    w32 = R.mol_nll(y, t)[0]
    assert w32.dtype == np.float32
    err, e32 = A.metrics(got, w64), A.metrics(w32, w64)
    print('RDMOL_ACC %s l2 %.3e (e32 %.3e, ratio %.2f) max %.3e (e32 %.3e, ratio %.2f)' % (
        what, err[0], e32[0], err[0] / max(e32[0], 1e-300), err[1], e32[1], err[1] / max(e32[1], 1e-300)))
    assert all(e <= A.bar(r) for e, r in zip(err, e32)), '%s: outside err <= 3 e32 + 1e-7: %r against e32 %r' % (what, err, e32)
    return w64


NLL_ROWS = [(10, [63, 1, 192]), (16, [257]), (1, [255, 2]), (10, [1])]


# ---- 1. the NLL alone ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,counts', NLL_ROWS)
def test_the_nll_alone_meets_the_float32_bar(gpu, M, counts):
    g = Ragged(counts, Q=3 * M)
    inp = CA.mol_inputs((M, 1, g.T))
    y, t = inp['y'], inp['t']                                                    # (1, 3 M, T), (1, 1, T)
    waves = [np.concatenate([[0.25], t[0, 0, g.seg(i)]]).astype(np.float32) for i in range(len(counts))]   # the target of jl is w[jl + 1]
    w, woff = g.place(waves, order=range(len(counts))[::-1], gap=3)
    got = _nll_on_device(gpu, g, np.ascontiguousarray(y[0]), w, woff, M)
    _judge('M %d columns %r' % (M, counts), got, y, t)


# ---- 2. the branches ---------------------------------------------------------------------------------------------------------------
def test_the_nll_s_branches_on_the_reference_s_crafted_input(gpu):
    fx = RM.load('ref_mol_loss.npz')
    y, t = RM.crafted_mol_inputs(fx['meta']['seed'])                               # (2, 30, 64), (2, 1, 64)
    g = Ragged([64, 64])
    waves = [np.concatenate([[0.0], t[b, 0]]).astype(np.float32) for b in range(2)]
    w, woff = g.place(waves)
    flat_y = np.ascontiguousarray(np.concatenate([y[0], y[1]], axis=1))
    flat_t = np.concatenate([t[0], t[1]], axis=1)[None]
    got = _nll_on_device(gpu, g, flat_y, w, woff, 10)
    print('RDMOL crafted: mean %.9g, reference %.9g' % (got.astype(np.float64).mean(), float(fx['loss'])))
    H.assert_close(got.astype(np.float64).mean(), float(fx['loss']), 1e-4, 'mean of the 128 NLLs against the reference loss')
    w64 = R.mol_nll(flat_y[None].astype(np.float64), flat_t.astype(np.float64))[0]
    w32 = R.mol_nll(flat_y[None], flat_t)[0]
    err, e32 = A.metrics(got, w64)[1], A.metrics(w32, w64)[1]
    print('RDMOL crafted: max %.3e (e32 %.3e, ratio %.2f)' % (err, e32, err / max(e32, 1e-300)))
    each = np.abs(got.astype(np.float64) - w64) / np.abs(w64).max()
    assert (each <= A.bar(e32)).all(), 'position %d: %.3e of the scale against bar %.3e' % (int(each.argmax()), each.max(), A.bar(e32))


# ---- 3. the embed alone -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Rr', [40, 65])
@pytest.mark.parametrize('bias', [True, False])
def test_the_embed_alone_is_the_restatement_s_bits(gpu, Rr, bias):
    from vqvae_amd import scoring_mol
    rs = np.random.RandomState(7 + Rr)
    for counts, order, gap in (([63, 1, 192], None, 0), ([255, 2, 1, 300], [2, 0, 3, 1], 5), ([63, 1, 192], [2, 1, 0], 0)):
        g = Ragged(counts, Rr=Rr)
        waves = [rs.uniform(-1, 1, n + 1).astype(np.float32) for n in counts]
        w, woff = g.place(waves, order, gap)
        W, b = rs.standard_normal((Rr, 1, 2)).astype(np.float32), rs.standard_normal(Rr).astype(np.float32)
        d = C.byref(g.desc)
        specs = dict(off=In(g.off), w=In(w), woff=In(woff), W=In(W), x=Out((Rr, g.T)))
        if bias:
            specs['b'] = In(b)
        out = run_contract(gpu, lambda bf: scoring_mol.call('vqvae_rdmol_embed', d, g.tables(bf), bf.w.ptr, bf.woff.ptr, bf.W.ptr,
                                                            bf.b.ptr if bias else None, bf.x.ptr, gpu.stream()), specs)
        want = R.embed_bits(W, b if bias else None, waves, counts)
        diff = _bits(out['x']) != _bits(want)
        assert out['x'].shape == want.shape and not diff.any(), 'R %d bias %r columns %r: %d elements differ, first at %r' % (
            Rr, bias, counts, int(diff.sum()), tuple(np.argwhere(diff)[0]))


# ---- 4. the refusals write nothing ----------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing(gpu):
    from vqvae_amd import _lib, scoring_mol
    lib = scoring_mol.load()
    g = Ragged([5, 3])
    msg = lambda: lib.vqvae_last_error_string().decode()
    poison = np.full((30, g.T), 7.5, np.float32)
    off, woff, w, y = gpu.to_device(g.off), gpu.to_device(np.array([0, 6], np.int64)), gpu.to_device(np.zeros(10, np.float32)), gpu.to_device(poison)
    x, nll = gpu.to_device(poison[:8].copy()), gpu.to_device(poison[0].copy())
    W = gpu.to_device(np.ones((8, 1, 2), np.float32))
    tb = _lib.RdecTables(off.ptr, None, None, None)
    S_ = gpu.stream
    bad_desc = _lib.RdecDesc(2, 8, 7, 8, 30, 4, 0, 1, UP, 0, g.T, 2)               # an odd D
    d = g.desc
    calls = [
        (lambda: lib.vqvae_rdmol_embed(None, C.byref(tb), w.ptr, woff.ptr, W.ptr, None, x.ptr, S_()), 'rdmol_embed: null descriptor'),
        (lambda: lib.vqvae_rdmol_embed(C.byref(bad_desc), C.byref(tb), w.ptr, woff.ptr, W.ptr, None, x.ptr, S_()), 'rdmol_embed: a descriptor the ragged decoder refuses'),
        (lambda: lib.vqvae_rdmol_embed(C.byref(d), None, w.ptr, woff.ptr, W.ptr, None, x.ptr, S_()), 'rdmol_embed: null tables or off'),
        (lambda: lib.vqvae_rdmol_embed(C.byref(d), C.byref(tb), None, woff.ptr, W.ptr, None, x.ptr, S_()), 'rdmol_embed: null w, woff, W or x'),
        (lambda: lib.vqvae_rdmol_embed(C.byref(d), C.byref(tb), w.ptr, None, W.ptr, None, x.ptr, S_()), 'rdmol_embed: null w, woff, W or x'),
        (lambda: lib.vqvae_rdmol_embed(C.byref(d), C.byref(tb), w.ptr, woff.ptr, None, None, x.ptr, S_()), 'rdmol_embed: null w, woff, W or x'),
        (lambda: lib.vqvae_rdmol_nll(None, C.byref(tb), y.ptr, w.ptr, woff.ptr, 10, 256, -40.0, nll.ptr, S_()), 'rdmol_nll: null descriptor'),
        (lambda: lib.vqvae_rdmol_nll(C.byref(bad_desc), C.byref(tb), y.ptr, w.ptr, woff.ptr, 10, 256, -40.0, nll.ptr, S_()), 'rdmol_nll: a descriptor the ragged decoder refuses'),
        (lambda: lib.vqvae_rdmol_nll(C.byref(d), None, y.ptr, w.ptr, woff.ptr, 10, 256, -40.0, nll.ptr, S_()), 'rdmol_nll: null tables or off'),
        (lambda: lib.vqvae_rdmol_nll(C.byref(d), C.byref(tb), None, w.ptr, woff.ptr, 10, 256, -40.0, nll.ptr, S_()), 'rdmol_nll: null y, w, woff or nll'),
        (lambda: lib.vqvae_rdmol_nll(C.byref(d), C.byref(tb), y.ptr, None, woff.ptr, 10, 256, -40.0, nll.ptr, S_()), 'rdmol_nll: null y, w, woff or nll'),
        (lambda: lib.vqvae_rdmol_nll(C.byref(d), C.byref(tb), y.ptr, w.ptr, None, 10, 256, -40.0, nll.ptr, S_()), 'rdmol_nll: null y, w, woff or nll'),
        (lambda: lib.vqvae_rdmol_nll(C.byref(d), C.byref(tb), y.ptr, w.ptr, woff.ptr, 0, 256, -40.0, nll.ptr, S_()), 'n_mix must be in 1 .. 16 (got 0)'),
        (lambda: lib.vqvae_rdmol_nll(C.byref(d), C.byref(tb), y.ptr, w.ptr, woff.ptr, 17, 256, -40.0, nll.ptr, S_()), 'n_mix must be in 1 .. 16 (got 17)'),
        (lambda: lib.vqvae_rdmol_nll(C.byref(d), C.byref(tb), y.ptr, w.ptr, woff.ptr, 9, 256, -40.0, nll.ptr, S_()), "Q must be 3 n_mix = 27 (got 30)"),
        (lambda: lib.vqvae_rdmol_nll(C.byref(d), C.byref(tb), y.ptr, w.ptr, woff.ptr, 10, 1, -40.0, nll.ptr, S_()), 'quantize must be at least 2 (got 1)'),
    ]
    for fn, words in calls:
        assert fn() == -1 and words in msg(), (words, msg())                       # VQVAE_E_INVALID
    gpu.synchronize()
    assert np.array_equal(x.get(), poison[:8]) and np.array_equal(nll.get(), poison[0])


# ---- 5. composition independence, as bit equality ---------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['m40s', 'm40q'])
def test_an_utterance_gets_the_same_bits_in_any_composition(gpu, matmul_mode, name):
    import vqvae_amd as V
    from vqvae_amd import scoring_mol
    c = case(name)
    wn = wavenet_link(name)
    n = len(c['tl'])
    cond = condition(gpu, c['local'], c['gvec'])
    base = V.score_many_mol(wn, cond, c['waves'], per_sample=True)
    assert base.count.tolist() == [r['n'] for r in c['ref']] and base.nll.dtype == np.float64 and base.count.dtype == np.int64
    np.testing.assert_array_equal(base.bits_per_sample, base.nll / base.count / np.log(2.0))
    assert base.total() == float(base.nll.sum() / base.count.sum() / np.log(2.0))
    for i in range(n):                                                           # alone
        one = V.score_many_mol(wn, condition(gpu, c['local'][i:i + 1], c['gvec'][i:i + 1]), [c['waves'][i]], per_sample=True)
        same_utterance(one, 0, base, i, 'utterance %d alone' % i)
        want = R.reduce_order(base.sample_nll(i))                                # the reduce's written order over the device's own NLL
        assert _bits(base.nll[i:i + 1])[0] == _bits(np.array([want]))[0], 'utterance %d: %r against the restated order %r' % (i, base.nll[i], want)
    rev = V.score_many_mol(wn, condition(gpu, c['local'][::-1], c['gvec'][::-1]), c['waves'][::-1], per_sample=True)
    for i in range(n):
        same_utterance(rev, n - 1 - i, base, i, 'utterance %d in the reversed list' % i)
    rs = np.random.RandomState(5)
    for parity in (0, 1):                # every neighbour replaced: samples permuted, condition block scaled by 1e3
        wv = [w if i % 2 == parity else rs.permutation(w).astype(np.float32) for i, w in enumerate(c['waves'])]
        loc = [a if i % 2 == parity else (1e3 * a).astype(np.float32) for i, a in enumerate(c['local'])]
        gv = np.stack([g if i % 2 == parity else 1e3 * g for i, g in enumerate(c['gvec'])]).astype(np.float32)
        other = V.score_many_mol(wn, condition(gpu, loc, gv), wv, per_sample=True)
        for i in range(parity, n, 2):
            same_utterance(other, i, base, i, 'utterance %d beside replaced neighbours' % i)
    _, dims = scoring_mol._check_decoder(wn, 'test')
    per = scoring_mol.chunk_elements(base.count, c['tl'], c['L'], dims)
    sizes = sorted(set(4 * int(per[:, a:b].sum(axis=1).max()) for a in range(n) for b in range(a + 1, n + 1)))
    three = [cb for cb in sizes if cb >= 4 * per.max() and len(scoring_mol.plan_chunks(base.count, c['tl'], c['L'], dims, cb)) == 3]
    assert three, 'no chunk_bytes cuts these lengths into three chunks'
    cut = V.score_many_mol(wn, cond, c['waves'], chunk_bytes=three[0], per_sample=True)
    for i in range(n):
        same_utterance(cut, i, base, i, 'utterance %d in three chunks of %d bytes' % (i, three[0]))
    smallest = 4 * int(per.max())                                                # every utterance fits alone; most chunks
    cut = V.score_many_mol(wn, cond, c['waves'], chunk_bytes=smallest, per_sample=True)
    for i in range(n):
        same_utterance(cut, i, base, i, 'utterance %d in chunks of %d bytes' % (i, smallest))
    corpus = V.ResidentCorpus(c['waves'], c['speakers'])                         # read in place, and a reordered view
    inplace = corpus.score_mol(wn, cond, per_sample=True)
    for i in range(n):
        same_utterance(inplace, i, base, i, 'utterance %d read in place from a ResidentCorpus' % i)
    order = np.arange(n)[::-1].copy()
    view = corpus.subset(order).score_mol(wn, condition(gpu, c['local'][::-1], c['gvec'][::-1]), per_sample=True)
    for i in range(n):
        same_utterance(view, n - 1 - i, base, i, 'utterance %d through a reversed CorpusView' % i)


@pytest.mark.parametrize('name', ['m40s', 'm40q'])
def test_evaluate_many_mol_is_frontend_many_then_score_many_mol(gpu, matmul_mode, name):
    import vqvae_amd as V
    c = case(name)
    wn, links = wavenet_link(name), front_links(name)
    cond = V.frontend_many(*links, c['waves'], c['speakers'])
    assert cond.tl.tolist() == c['tl']
    two = V.score_many_mol(wn, cond, c['waves'], per_sample=True)
    one = V.evaluate_many_mol(*links, wn, c['waves'], c['speakers'], per_sample=True)
    for i in range(len(c['tl'])):
        same_utterance(one, i, two, i, 'utterance %d' % i)


# ---- 6. values ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['m40s', 'm40q'])
def test_values_against_the_float64_restatement(gpu, matmul_mode, name):
    import vqvae_amd as V
    c = case(name)
    at_floor = sum(int(r['floor'].sum()) for r in c['ref'])
    assert at_floor == 0, '%d positions have every component at the 1e-12 floor: the comparison would compare constants' % at_floor
    for i, (w, r) in enumerate(zip(c['waves'], c['ref'])):
        assert (np.abs(w[1:r['n'] + 1]) > 0.999).any(), 'utterance %d has no target in a tail' % i
    wn = wavenet_link(name)
    s = V.score_many_mol(wn, condition(gpu, c['local'], c['gvec']), c['waves'], per_sample=True, return_params=True)
    for i, r in enumerate(c['ref']):
        nll, y = s.sample_nll(i), s.params[i]
        print('SCORING_MOL %s %s utterance %d: nll in [%.3f, %.3f], max |nll - ref| %.3e, max |params - ref| %.3e' % (
            name, matmul_mode, i, r['nll'].min(), r['nll'].max(), np.abs(nll - r['nll']).max(), np.abs(y - r['params']).max()))
        H.assert_close(nll, r['nll'], TOL, 'per-sample NLL of utterance %d' % i)
        H.assert_close(y, r['params'], TOL, 'mixture parameters of utterance %d' % i)
        H.assert_close(s.nll[i], r['nll'].sum(), TOL, 'nll of utterance %d' % i)


# ---- 7. the reference's model ---------------------------------------------------------------------------------------------------
def test_the_reference_s_model_and_batch(gpu):
    import vqvae_amd as V
    fx = RM.load('ref_model_mol.npz')
    meta = fx['meta']
    _, model = H.build_model(dict(meta['cfg']), seed=meta['param_seed'], use_logistic=True, tweak=H.named_tweak(meta['tweak']))
    model.to_gpu()
    x_enc, _, spk, _ = O.synth_batch_raw(meta['B'], length=meta['length'], n_speaker=meta['cfg']['n_speaker'], seed=meta['batch_seed'])
    gpu.set_matmul_dtype('float32')
    try:
        s = V.evaluate_many_mol(model.encoder, model.vq, model.condition_embed, model.decoder, [x_enc[b, 0] for b in range(meta['B'])], spk)
    finally:
        gpu.set_matmul_dtype(gpu.default_matmul_dtype())
    assert s.count.tolist() == [512, 512]
    got = s.nll.sum() / s.count.sum()
    print('SCORING_MOL reference model: nll / count %.9g, reference loss1 %.9g' % (got, float(fx['losses'][0])))
    H.assert_close(got, float(fx['losses'][0]), TOL, 'nll / count against the reference loss1')


# ---- 8. the tie to the existing device path ---------------------------------------------------------------------------------------
def test_loss1_of_the_training_forward_is_nll_over_count(gpu, matmul_mode):
    import vqvae_amd as V
    cfg = dict(H.MOL_SHALLOW)
    P, model = H.build_model(cfg, seed=3, use_logistic=True, tweak=H.named_tweak('mol_output+biases:3'))
    model.to_gpu()
    tl = 3
    x_enc, x_dec, spk, t = O.synth_batch_raw(1, length=64 * tl, n_speaker=cfg['n_speaker'], seed=77)
    with V.using_config('train', False), V.core.no_backprop_mode():
        losses = model(gpu.to_device(x_enc[..., None]), gpu.to_device(x_dec[..., None]), gpu.to_device(spk), gpu.to_device(t[..., None]))
    loss1 = float(losses[0].data.get())
    s = V.evaluate_many_mol(model.encoder, model.vq, model.condition_embed, model.decoder, [x_enc.reshape(-1)], spk)
    assert s.count.tolist() == [64 * tl]
    print('SCORING_MOL tie %s: loss1 %.9g, nll / count %.9g' % (matmul_mode, loss1, s.nll[0] / s.count[0]))
    H.assert_close(s.nll[0] / s.count[0], loss1, TOL, 'nll / count against loss1')
