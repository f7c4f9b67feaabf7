"""Held-out likelihood on the device (vqvae_amd.scoring, include/vqvae_ragged_decoder.h, csrc/ragged_decoder.hip).

1. Composition independence as BIT equality of per-sample NLL, nll, count and hits: alone / reversed / beside replaced
   neighbours / three chunks against one / a ResidentCorpus read in place / evaluate_many against its two halves.
2. Values: per-sample NLL and logits against the float64 restatement (tests/scoring_ref.py) at the project's conv tolerance
   (1e-4, helpers.assert_close); every entry point alone against its own function in float64 over the values it was handed,
   at chain_accuracy_ref.bar(e32).
3. The reduce against the exact restatement of its order: bits.
4. The tie to the existing device path: VAE.__call__'s loss1 on B = 1.
5. Every entry point under zoned.run_contract.

Models (O.make_params): s64 has dilation 128, longer than the shortest utterance; s40 puts every row edge off a tile; s512
runs the 128-row tiles at the default widths.  Lengths: L_i = 64 tl_i for even i (n_i = 64 tl_i - 1: segment borders inside
column tiles, 63 columns first), 64 tl_i + 1 + i for odd i.  Conditions are random latent blocks handed over through
LatentCondition.from_latents, so the references are computed on the CPU once per model and never modified; the seeds were
chosen there so that fewer than 1 % of the positions have a top-two logit gap within the tolerance (asserted)."""
import ctypes as C

import numpy as np
import pytest

import chain_accuracy_ref as A
import helpers as H
from helpers import _bits
import scoring_ref as R
import vqvae_oracle as O
from zoned import In, Out, Ws, run_contract

pytestmark = pytest.mark.gpu

TOL = 1e-4
UP = 64
N_SPEAKER = 3
TL = [1, 3, 2, 1, 5, 2]
# name -> (R, D, S, Cl, G, Q, n_loop, n_layer, tl, seed)
MODELS = {'s64': (64, 128, 64, 64, 8, 256, 1, 8, TL, 11),
          's40': (40, 48, 24, 24, 8, 37, 2, 3, TL, 12),
          's512': (512, 512, 256, 512, 128, 256, 1, 2, [2, 1], 13)}
ENC_D, ENC_K = 16, 8


def lengths_for(tl):
    return [64 * t if i % 2 == 0 else 64 * t + 1 + i for i, t in enumerate(tl)]


_CASES = {}


def case(name):
    """Everything of a model that the CPU makes, once: parameters, waves, classes, latent blocks, speaker vectors and the
    float64 restatement of every utterance."""
    if name not in _CASES:
        Rr, D, S, Cl, G, Q, n_loop, n_layer, tl, seed = MODELS[name]
        rs = np.random.RandomState(seed)
        P = O.make_params(rs, d=ENC_D, k=ENC_K, n_loop=n_loop, n_layer=n_layer, input_dim=Q, residual=Rr, dilated=D, skip=S,
                          out_dim=Q, local_dim=Cl, global_dim=G, n_speaker=N_SPEAKER)
        H.named_tweak('biases:%d' % seed)(P)
        P['decoder']['proj2'] = (3.0 * P['decoder']['proj2'][0], P['decoder']['proj2'][1])      # logits a few units apart
        Ls = lengths_for(tl)
        waves = [O.synth_batch(1, length=L - 1, n_speaker=N_SPEAKER, seed=500 + 7 * i + seed)[0].reshape(-1).copy() for i, L in enumerate(Ls)]
        classes = [O.MuLaw(Q).transform(w).astype(np.int32) for w in waves]
        local = [np.maximum(rs.standard_normal((Cl, t)), 0).astype(np.float32) for t in tl]
        gvec = rs.standard_normal((len(tl), G)).astype(np.float32)
        ref = [R.score_utterance(P['decoder'], q, lo, g, n_loop, n_layer, UP) for q, lo, g in zip(classes, local, gvec)]
        for a in waves + classes + local + [gvec]:
            a.setflags(write=False)
        _CASES[name] = dict(P=P, waves=waves, classes=classes, local=local, gvec=gvec, ref=ref, tl=tl, L=Ls,
                            speakers=np.array([(2 * i + 1) % N_SPEAKER for i in range(len(tl))], np.int32))
    return _CASES[name]


def wavenet_link(name):
    from vqvae_amd.wavenet import WaveNet
    Rr, D, S, Cl, G, Q, n_loop, n_layer = MODELS[name][:8]
    wn = WaveNet(n_loop, n_layer, 2, Q, Rr, D, S, Q, False, 10, -40, Cl + G, 0)
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
    assert got.count[i] == want.count[k] and got.hits[i] == want.hits[k], '%s: count / hits differ' % what


# ---- 1. composition independence, as bit equality ---------------------------------------------------------------------
@pytest.mark.parametrize('name', ['s64', 's40', 's512'])
def test_an_utterance_gets_the_same_bits_in_any_composition(gpu, matmul_mode, name):
    import vqvae_amd as V
    from vqvae_amd import scoring
    c = case(name)
    wn = wavenet_link(name)
    n = len(c['tl'])
    cond = condition(gpu, c['local'], c['gvec'])
    base = V.score_many(wn, cond, c['waves'], per_sample=True)
    assert base.count.tolist() == [r['n'] for r in c['ref']] and base.nll.dtype == np.float64 and base.hits.dtype == np.int64
    np.testing.assert_array_equal(base.bits_per_sample, base.nll / base.count / np.log(2.0))
    assert base.total() == float(base.nll.sum() / base.count.sum() / np.log(2.0))
    for i in range(n):                                                           # alone
        one = V.score_many(wn, condition(gpu, c['local'][i:i + 1], c['gvec'][i:i + 1]), [c['waves'][i]], per_sample=True)
        same_utterance(one, 0, base, i, 'utterance %d alone' % i)
    rev = V.score_many(wn, condition(gpu, c['local'][::-1], c['gvec'][::-1]), c['waves'][::-1], per_sample=True)
    for i in range(n):
        same_utterance(rev, n - 1 - i, base, i, 'utterance %d in the reversed list' % i)
    rs = np.random.RandomState(5)
    for parity in (0, 1):                # every neighbour replaced: classes shuffled, condition block scaled by 1e3; int32 classes are taken as binned
        cls = [q if i % 2 == parity else rs.permutation(q).astype(np.int32) for i, q in enumerate(c['classes'])]
        loc = [a if i % 2 == parity else (1e3 * a).astype(np.float32) for i, a in enumerate(c['local'])]
        gv = np.stack([g if i % 2 == parity else 1e3 * g for i, g in enumerate(c['gvec'])]).astype(np.float32)
        other = V.score_many(wn, condition(gpu, loc, gv), cls, per_sample=True)
        for i in range(parity, n, 2):
            same_utterance(other, i, base, i, 'utterance %d beside replaced neighbours' % i)
    dims = scoring._dims(wn, list(wn.resnet.children()), 'test')
    per = scoring.chunk_elements(base.count, c['tl'], c['L'], dims)
    sizes = sorted(set(4 * int(per[:, a:b].sum(axis=1).max()) for a in range(n) for b in range(a + 1, n + 1)))
    three = [cb for cb in sizes if cb >= 4 * per.max() and len(scoring.plan_chunks(base.count, c['tl'], c['L'], dims, cb)) == 3]
    if n >= 3:
        assert three, 'no chunk_bytes cuts these lengths into three chunks'
        cut = V.score_many(wn, cond, c['waves'], chunk_bytes=three[0], per_sample=True)
        for i in range(n):
            same_utterance(cut, i, base, i, 'utterance %d in three chunks of %d bytes' % (i, three[0]))
    smallest = 4 * int(per.max())                                                # every utterance fits alone; most chunks
    cut = V.score_many(wn, cond, c['waves'], chunk_bytes=smallest, per_sample=True)
    for i in range(n):
        same_utterance(cut, i, base, i, 'utterance %d in chunks of %d bytes' % (i, smallest))
    corpus = V.ResidentCorpus(c['waves'], c['speakers'])                         # read in place, and a reordered view
    inplace = corpus.score(wn, cond, per_sample=True)
    for i in range(n):
        same_utterance(inplace, i, base, i, 'utterance %d read in place from a ResidentCorpus' % i)
    order = np.arange(n)[::-1].copy()
    view = corpus.subset(order).score(wn, condition(gpu, c['local'][::-1], c['gvec'][::-1]), per_sample=True)
    for i in range(n):
        same_utterance(view, n - 1 - i, base, i, 'utterance %d through a reversed CorpusView' % i)


@pytest.mark.parametrize('name', ['s40'])
def test_evaluate_many_is_frontend_many_then_score_many(gpu, matmul_mode, name):
    import vqvae_amd as V
    c = case(name)
    wn, links = wavenet_link(name), front_links(name)
    cond = V.frontend_many(*links, c['waves'], c['speakers'])
    assert cond.tl.tolist() == c['tl']
    two = V.score_many(wn, cond, c['waves'], per_sample=True)
    one = V.evaluate_many(*links, wn, c['waves'], c['speakers'], per_sample=True)
    for i in range(len(c['tl'])):
        same_utterance(one, i, two, i, 'utterance %d' % i)


# ---- 2. values ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['s64', 's40', 's512'])
def test_values_against_the_float64_restatement(gpu, matmul_mode, name):
    import vqvae_amd as V
    c = case(name)
    wn = wavenet_link(name)
    s = V.score_many(wn, condition(gpu, c['local'], c['gvec']), c['waves'], per_sample=True, return_logits=True)
    left_out = total = 0
    for i, r in enumerate(c['ref']):
        nll, y = s.sample_nll(i), s.logits[i]
        print('SCORING %s %s utterance %d: max |nll - ref| %.3e, max |logit - ref| %.3e' % (
            name, matmul_mode, i, np.abs(nll - r['nll']).max(), np.abs(y - r['logits']).max()))
        H.assert_close(nll, r['nll'], TOL, 'per-sample NLL of utterance %d' % i)
        H.assert_close(y, r['logits'], TOL, 'logits of utterance %d' % i)
        # either of the two largest logits may move by TOL max(1, |y|): the arg-max is decided where their gap is above twice that
        sure = r['gap'] > 2 * TOL * np.maximum(1.0, np.abs(r['logits']).max(axis=0))
        left_out += int((~sure).sum())
        total += r['n']
        hit_dev = np.argmax(y, axis=0) == c['classes'][i][1:r['n'] + 1]
        assert np.array_equal(hit_dev[sure], r['hit'][sure]), 'utterance %d: the arg-max differs where the gap is decisive' % i
        assert s.hits[i] == int(hit_dev.sum()), 'utterance %d: hits %d against the logits\' own count %d' % (i, s.hits[i], hit_dev.sum())
        assert abs(int(s.hits[i]) - int(r['hit'].sum())) <= int((~sure).sum())
        H.assert_close(s.nll[i], r['nll'].sum(), TOL, 'nll of utterance %d' % i)
    assert left_out <= 0.01 * total, '%d of %d positions have an undecided arg-max: choose another seed' % (left_out, total)


# ---- 2b / 3 / 5. every entry point alone: contract, accuracy, the reduce's bits -----------------------------------------------
class Geo(object):
    """One chunk's geometry and its tables for direct calls."""

    def __init__(self, Rr, D, S, Cl, G, Q, nb, tl):
        from vqvae_amd import _lib
        self.R, self.D, self.S, self.Cl, self.G, self.Q, self.nb, self.tl = Rr, D, S, Cl, G, Q, nb, np.asarray(tl, np.int32)
        self.L = np.asarray(lengths_for(tl), np.int64)
        self.n = np.minimum(UP * self.tl.astype(np.int64), self.L - 1)
        self.off = np.concatenate([[0], np.cumsum(self.n)]).astype(np.int64)
        self.qoff = np.concatenate([[0], np.cumsum(self.L)[:-1]]).astype(np.int64)
        self.latoff = np.concatenate([[0], np.cumsum(self.tl)]).astype(np.int64)
        self.T, self.TL = int(self.off[-1]), int(self.latoff[-1])
        self.desc = _lib.RdecDesc(len(tl), Rr, D, S, Q, Cl, G, nb, UP, 0, self.T, self.TL)
        self.specs = dict(off=In(self.off), qoff=In(self.qoff), latoff=In(self.latoff), tl=In(self.tl))

    def tables(self, b):
        from vqvae_amd import _lib
        return C.byref(_lib.RdecTables(b.off.ptr, b.qoff.ptr, b.latoff.ptr, b.tl.ptr))

    def seg(self, i):
        return slice(int(self.off[i]), int(self.off[i + 1]))


GEOS = {'g40': (40, 48, 24, 24, 8, 37, 2, [1, 3, 2]), 'g512': (512, 512, 256, 512, 128, 256, 2, [2, 1])}


class Judge(object):
    def __init__(self, geo, mode):
        self.geo, self.mode, self.misses = geo, mode, []

    def __call__(self, what, got, f, margin=(0.0, 0.0)):
        w64, w32 = f(np.float64), f(np.float32)
        assert w32.dtype == np.float32
        err, e32 = A.metrics(got, w64), A.metrics(w32, w64)
        line = 'RDEC_ACC %s %s %s l2 %.3e (e32 %.3e) max %.3e (e32 %.3e)' % (self.geo, self.mode, what, err[0], e32[0], err[1], e32[1])
        print(line)
        if not all(e <= A.bar(r) + m for e, r, m in zip(err, e32, margin)):
            self.misses.append(line + ' margin %.3e %.3e' % tuple(margin))

    def finish(self):
        assert not self.misses, 'outside err <= 3 e32 + 1e-7:\n' + '\n'.join(self.misses)


def _c(a, dt):
    return np.ascontiguousarray(np.asarray(a).astype(dt))


@pytest.mark.parametrize('geo', ['g40', 'g512'])
def test_every_entry_point_alone(gpu, matmul_mode, geo):
    from vqvae_amd import _lib
    g = Geo(*GEOS[geo])
    rs = np.random.RandomState(3)
    Ch, M, Cc = g.D // 2, g.nb * g.D, g.Cl + g.G
    d, S_ = C.byref(g.desc), gpu.stream
    judge = Judge(geo, matmul_mode)
    f32 = lambda *sh: rs.standard_normal(sh).astype(np.float32)
    q = rs.randint(0, g.Q, int(g.L.sum())).astype(np.int32)
    qs = [q[int(o):int(o) + int(L)] for o, L in zip(g.qoff, g.L)]

    # embed
    We, be = f32(g.R, g.Q, 2), f32(g.R)
    out = run_contract(gpu, lambda b: _lib.call('vqvae_rdec_embed', d, g.tables(b), b.q.ptr, b.W.ptr, b.b.ptr, b.x.ptr, S_()),
                       dict(g.specs, q=In(q, index_range=(0, g.Q)), W=In(We), b=In(be), x=Out((g.R, g.T))))

    def embed_ref(dt):
        W, cols = _c(We, dt), []
        for qi, n in zip(qs, g.n):
            first = np.concatenate([np.zeros((g.R, 1), dt), W[:, qi[:n - 1], 0]], axis=1)
            cols.append(first + W[:, qi[:n], 1] + _c(be, dt)[:, None])
        return np.concatenate(cols, axis=1)
    judge('embed', out['x'], embed_ref)

    # the condition at the latent rate
    Wc_all, bias_all, gv = f32(M, Cc) / np.float32(np.sqrt(Cc)), f32(M), f32(len(g.tl), g.G)
    local = [np.maximum(f32(g.Cl, int(t)), 0) for t in g.tl]
    local_flat = np.concatenate([a.reshape(-1) for a in local])
    out = run_contract(gpu, lambda b: _lib.call('vqvae_rdec_cond_project', d, g.tables(b), b.local.ptr, b.W.ptr, b.P.ptr, S_()),
                       dict(g.specs, local=In(local_flat), W=In(Wc_all), P=Out((M, g.TL))))
    Pdev = out['P']
    judge('cond_project', Pdev, lambda dt: np.concatenate([np.matmul(_c(Wc_all[:, :g.Cl], dt), _c(a, dt)) for a in local], axis=1))
    out = run_contract(gpu, lambda b: _lib.call('vqvae_rdec_cond_global', d, b.gv.ptr, b.W.ptr, b.bias.ptr, b.g.ptr, S_()),
                       dict(gv=In(gv), W=In(Wc_all), bias=In(bias_all), g=Out((len(g.tl), M))))
    gdev = out['g']
    judge('cond_global', gdev, lambda dt: np.matmul(_c(gv, dt), _c(Wc_all[:, g.Cl:], dt).T) + _c(bias_all, dt)[None],
          (0.0, A.seq_error(g.G)))

    # gate: block 1 of 2, a dilation longer than the shortest utterance, over the P and g the device wrote
    x, Wd = f32(g.R, g.T), f32(g.D, g.R, 2) / np.float32(np.sqrt(2 * g.R))
    for dil in (1, 128):
        out = run_contract(gpu, lambda b: _lib.call('vqvae_rdec_gate', d, g.tables(b), 1, dil, b.x.ptr, b.Wd.ptr, b.P.ptr, b.g.ptr,
                                                    b.z.ptr, S_()),
                           dict(g.specs, x=In(x), Wd=In(Wd), P=In(Pdev), g=In(gdev), z=Out((Ch, g.T))))

        def gate_h(dt, dil=dil):
            hs = []
            for i, (n, t) in enumerate(zip(g.n, g.tl)):
                xi = _c(x[:, g.seg(i)], dt)[None]
                v0, v1, w0, w1 = O.resize_tables(int(t), UP * int(t), np.float32)
                Pi = _c(Pdev[g.D:2 * g.D, int(g.latoff[i]):int(g.latoff[i + 1])], dt)
                lerp = (_c(w0, dt)[None] * Pi[:, v0] + _c(w1, dt)[None] * Pi[:, v1])[:, :n]
                h = np.matmul(_c(Wd[:, :, 0], dt), A._shift(xi, dil)[0]) + np.matmul(_c(Wd[:, :, 1], dt), xi[0])
                hs.append(h + lerp + _c(gdev[i, g.D:2 * g.D], dt)[:, None])
            return np.concatenate(hs, axis=1)

        def gate_ref(dt):
            h = gate_h(dt)
            return np.tanh(h[:Ch]) * A._sigmoid(h[Ch:])
        h64 = gate_h(np.float64)
        seq = A.seq_error(2 * g.R + 2) if matmul_mode == 'float32' else 0.0        # one fp32 accumulator over K (test_gpu_chain_accuracy: GATE MARGIN)
        judge('gate dil %d' % dil, out['z'], gate_ref, (0.0, seq * (np.abs(h64[:Ch]).max() + np.abs(h64[Ch:]).max() / 4)))

    # res / skip: the first block writes skip, a later one adds to it, the last has no residual output
    z, Wr, br, Ws_, bs = np.tanh(f32(Ch, g.T)), f32(g.R, Ch) / np.float32(np.sqrt(Ch)), f32(g.R), f32(g.S, Ch) / np.float32(np.sqrt(Ch)), f32(g.S)
    skip0 = f32(g.S, g.T)
    for acc, last in ((0, False), (1, False), (1, True)):
        specs = dict(z=In(z), Wr=In(Wr), br=In(br), Ws=In(Ws_), bs=In(bs), x=In(x), xo=Out((g.R, g.T), valid=np.full((g.R, g.T), not last)),
                     skip=Out(init=skip0) if acc else Out((g.S, g.T)))
        out = run_contract(gpu, lambda b: _lib.call('vqvae_rdec_res_skip', d, b.z.ptr, None if last else b.Wr.ptr, None if last else b.br.ptr,
                                                    b.Ws.ptr, b.bs.ptr, None if last else b.x.ptr, None if last else b.xo.ptr, b.skip.ptr, acc, S_()), specs)
        if not last:
            judge('res (accumulate %d)' % acc, out['xo'], lambda dt: np.matmul(_c(Wr, dt), _c(z, dt)) + _c(br, dt)[:, None] + _c(x, dt))
        judge('skip (accumulate %d, last %d)' % (acc, last), out['skip'],
              lambda dt: (_c(skip0, dt) if acc else 0) + (np.matmul(_c(Ws_, dt), _c(z, dt)) + _c(bs, dt)[:, None]))

    # head, with and without the logits, and the reduce over what it wrote
    W1, b1, W2, b2 = f32(g.S, g.S) / np.float32(np.sqrt(g.S)), f32(g.S), 3 * f32(g.Q, g.S) / np.float32(np.sqrt(g.S)), f32(g.Q)
    need = _lib.load().vqvae_rdec_workspace_bytes(d)
    assert need == -(-4 * g.S * g.T // 256) * 256
    tgt = np.concatenate([qi[1:n + 1] for qi, n in zip(qs, g.n)])

    def head_ref(dt):
        s1 = np.maximum(np.matmul(_c(W1, dt), np.maximum(_c(skip0, dt), 0)) + _c(b1, dt)[:, None], 0)
        return np.matmul(_c(W2, dt), s1) + _c(b2, dt)[:, None]

    def nll_ref(dt):
        y = head_ref(dt)
        m = y.max(axis=0)
        return np.log(np.exp(y - m).sum(axis=0, dtype=dt)) + m - y[tgt, np.arange(g.T)]
    outs = {}
    for with_logits in (True, False):
        specs = dict(g.specs, q=In(q, index_range=(0, g.Q)), skip=In(skip0), W1=In(W1), b1=In(b1), W2=In(W2), b2=In(b2),
                     nll=Out((g.T,)), hit=Out((g.T,), np.int32), ws=Ws(need))
        if with_logits:
            specs['logits'] = Out((g.Q, g.T))
        outs[with_logits] = run_contract(gpu, lambda b: _lib.call(
            'vqvae_rdec_head', d, g.tables(b), b.q.ptr, b.skip.ptr, b.W1.ptr, b.b1.ptr, b.W2.ptr, b.b2.ptr, b.nll.ptr, b.hit.ptr,
            b.logits.ptr if with_logits else None, b.ws.ptr, need, S_()), specs)
    out = outs[True]
    assert np.array_equal(_bits(out['nll']), _bits(outs[False]['nll'])) and np.array_equal(out['hit'], outs[False]['hit'])
    judge('head logits', out['logits'], head_ref)
    judge('head nll', out['nll'], nll_ref)
    y = out['logits']                                         # the column functions, exactly, over the logits the device wrote
    assert np.array_equal(out['hit'], (np.argmax(y, axis=0) == tgt).astype(np.int32)), 'hit is not the arg-max (lowest index) of the logits'
    H.assert_close(out['nll'], nll_ref(np.float64), TOL, 'head nll')

    red = run_contract(gpu, lambda b: _lib.call('vqvae_rdec_reduce', d, g.tables(b), b.nll.ptr, b.hit.ptr, b.s.ptr, b.h.ptr, S_()),
                       dict(g.specs, nll=In(out['nll']), hit=In(out['hit']), s=Out((len(g.tl),), np.float64), h=Out((len(g.tl),), np.int64)))
    for i in range(len(g.tl)):
        want = R.reduce_order(out['nll'][g.seg(i)])
        assert _bits(red['s'][i:i + 1])[0] == _bits(np.array([want]))[0], 'utterance %d: %r against the restated order %r' % (i, red['s'][i], want)
        assert red['h'][i] == int(out['hit'][g.seg(i)].sum())
    judge.finish()


def test_the_reduce_follows_its_written_order_on_long_utterances(gpu):
    """Bits, on lengths around the lane count and values whose float64 sum depends on the order."""
    from vqvae_amd import _lib
    n = np.array([1, 255, 256, 257, 1000, 513], np.int64)
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    rs = np.random.RandomState(9)
    nll = (rs.standard_normal(int(off[-1])) * 10.0 ** rs.randint(-6, 6, int(off[-1]))).astype(np.float32)
    hit = rs.randint(0, 2, int(off[-1])).astype(np.int32)
    desc = _lib.RdecDesc(len(n), 8, 8, 8, 8, 8, 0, 1, 64, 0, int(off[-1]), len(n))
    keep = gpu.to_device(off)
    tb = _lib.RdecTables(keep.ptr, None, None, None)
    s, h = gpu.DeviceArray((len(n),), np.float64), gpu.DeviceArray((len(n),), np.int64)
    nll_dev, hit_dev = gpu.to_device(nll), gpu.to_device(hit)
    _lib.call('vqvae_rdec_reduce', C.byref(desc), C.byref(tb), nll_dev.ptr, hit_dev.ptr, s.ptr, h.ptr, gpu.stream())
    s, h = s.get(), h.get()
    for i in range(len(n)):
        seg = slice(int(off[i]), int(off[i + 1]))
        assert _bits(s[i:i + 1])[0] == _bits(np.array([R.reduce_order(nll[seg])]))[0], i
        assert h[i] == R.reduce_order(hit[seg]) == hit[seg].sum()


# ---- 4. the tie to the existing device path -----------------------------------------------------------------------------------
def test_loss1_of_the_training_forward_is_nll_over_count(gpu, matmul_mode):
    import vqvae_amd as V
    cfg = dict(H.SMALL)
    P, model = H.build_model(cfg, seed=3, tweak=H.named_tweak('biases:3'))
    model.to_gpu()
    tl = 3
    x_enc, x_dec, spk, t = O.synth_batch(1, length=64 * tl, n_speaker=cfg['n_speaker'], seed=77)
    with V.using_config('train', False), V.core.no_backprop_mode():
        losses = model(gpu.to_device(x_enc[..., None]), gpu.to_device(x_dec[..., None]), gpu.to_device(spk), gpu.to_device(t[..., None]))
    loss1 = float(losses[0].data.get())
    wave = x_enc.reshape(-1)
    s = V.evaluate_many(model.encoder, model.vq, model.condition_embed, model.decoder, [wave], spk)
    assert s.count.tolist() == [64 * tl]
    print('SCORING tie %s: loss1 %.9g, nll / count %.9g' % (matmul_mode, loss1, s.nll[0] / s.count[0]))
    H.assert_close(s.nll[0] / s.count[0], loss1, TOL, 'nll / count against loss1')
