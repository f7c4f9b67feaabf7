"""The ragged front end on the device (vqvae_amd.frontend, include/vqvae_ragged.h, csrc/ragged_front.hip).

The property under test is composition independence: an utterance's codes and condition block are a pure function of
its own samples and the weights, so they are compared as BITS alone / in a list / reversed / beside loud neighbours /
in any chunking / read in place from a corpus.  Values are compared per utterance with the float64 restatement
(tests/ragged_frontend_ref.py) at the project's conv tolerance (1e-4, helpers.assert_close), in the three fp32-accurate
matmul modes.  Latent lengths 1, 2, 17, 40, 127, 128 put one segment boundary inside a 64-column tile and one exactly
on column 128; the sample counts are odd at different stages."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
from helpers import _bits
import ragged_frontend_ref as R
import vqvae_oracle as O
from zoned import In, Out, run_contract

pytestmark = pytest.mark.gpu

TOL = 1e-4
G, N_SPEAKER = 8, 3
TL_RUN = [1, 127, 128, 2, 40, 17, 1]
# name -> (d, Cl, k, seed, codebook scale, latent lengths): seeds chosen on the float64 restatement so that the codebook
# separates the latents (the precondition test_values_against_float64_and_indices_bit_for_bit asserts) and several codes are in use
MODELS = {'m64': (64, 64, 16, 40, 0.1, TL_RUN), 'm40': (40, 24, 7, 108, 0.1, TL_RUN), 'm512': (512, 512, 16, 4, 0.1, [2, 1])}


def _samples_for(tl, odd):
    """A sample count whose latent length is tl; bit s of ``odd`` makes the length of stage 5 - s odd."""
    t = tl
    for s in range(R.DEPTH):
        t = 2 * t + ((odd >> s) & 1)
    assert R.latent_length(t) == tl
    return t


_CASES = {}


def _case(name):
    """(P, waves, speakers, per-utterance float64 reference), computed once per model and never modified."""
    if name not in _CASES:
        d, Cl, k, seed, scale, tls = MODELS[name]
        rs = np.random.RandomState(seed)
        P = O.make_params(rs, d=d, k=k, n_loop=1, n_layer=1, residual=8, dilated=8, skip=8, local_dim=Cl, global_dim=G,
                          n_speaker=N_SPEAKER)
        for grp in ('encoder', 'condition_embed'):
            for n, v in P[grp].items():
                if isinstance(v, tuple):
                    P[grp][n] = (v[0], (0.1 * rs.standard_normal(v[1].shape)).astype(np.float32))
        P['vq'] = (scale * rs.standard_normal((k, d))).astype(np.float32)
        waves = []
        for i, tl in enumerate(tls):
            n = _samples_for(tl, (37 * i + 5) & 63)
            waves.append(O.synth_batch(1, length=n - 1, n_speaker=N_SPEAKER, seed=300 + i)[0].reshape(-1).copy())
        speakers = np.array([(2 * i + 1) % N_SPEAKER for i in range(len(tls))], np.int32)
        ref = [R.frontend(P, w) for w in waves]
        for w in waves:
            w.setflags(write=False)
        _CASES[name] = (P, waves, speakers, ref)
    return _CASES[name]


def _links(P):
    from vqvae_amd.net import ConditionEmbed, Encoder
    from vqvae_amd.utils import VQ
    k, d = P['vq'].shape
    Cl = P['condition_embed']['local_embed5'][0].shape[0]
    enc, vq, ce = Encoder(d), VQ(k, d), ConditionEmbed(N_SPEAKER, G, Cl)
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


def _blocks(cond):
    """The local blocks of a LatentCondition as host arrays (Cl, tl_i)."""
    flat = cond.local.get().reshape(-1)
    return [flat[int(o):int(o) + cond.Cl * int(t)].reshape(cond.Cl, int(t)).copy() for o, t in zip(cond.local_off, cond.tl)]


def _same_utterance(got_codes, got_block, want_codes, want_block, what):
    assert got_codes.dtype == want_codes.dtype == np.int32 and np.array_equal(got_codes, want_codes), '%s: codes differ' % what
    assert got_block.shape == want_block.shape and np.array_equal(_bits(got_block), _bits(want_block)), \
        '%s: the condition block differs in %d of %d elements' % (what, int((_bits(got_block) != _bits(want_block)).sum()),
                                                                 got_block.size)


def _front(links, waves, speakers, **kw):
    import vqvae_amd as V
    cond, codes = V.frontend_many(*links, waves, speakers, return_codes=True, **kw)
    return codes.to_host(), _blocks(cond), cond, codes


# ---- 1. composition independence, as bit equality ---------------------------------------------------------------------
@pytest.mark.parametrize('name', ['m64', 'm40', 'm512'])
def test_an_utterance_gets_the_same_bits_in_any_composition(gpu, matmul_mode, name):
    import vqvae_amd as V
    P, waves, speakers, ref = _case(name)
    links = _links(P)
    n = len(waves)
    codes, blocks, cond, _ = _front(links, waves, speakers)
    assert cond.tl.tolist() == MODELS[name][5] and [len(c) for c in codes] == MODELS[name][5]
    for i in range(n):                                                           # alone
        c1, b1, _, _ = _front(links, [waves[i]], speakers[i:i + 1])
        _same_utterance(c1[0], b1[0], codes[i], blocks[i], 'utterance %d alone' % i)
    cr, br, _, _ = _front(links, waves[::-1], speakers[::-1].copy())            # reversed
    for i in range(n):
        _same_utterance(cr[n - 1 - i], br[n - 1 - i], codes[i], blocks[i], 'utterance %d in the reversed list' % i)
    for parity in (0, 1):                                                        # between neighbours of amplitude 1e3
        loud = [w if i % 2 == parity else (1e3 * w).astype(np.float32) for i, w in enumerate(waves)]
        cl, bl, _, _ = _front(links, loud, speakers)
        for i in range(parity, n, 2):
            _same_utterance(cl[i], bl[i], codes[i], blocks[i], 'utterance %d between loud neighbours' % i)
    c1, b1, _, _ = _front(links, waves, speakers, chunk_bytes=1)                 # one utterance per chunk
    c2, b2, _, _ = _front(links, waves, speakers, chunk_bytes=1 << 40)           # all in one chunk
    mid = 4 * MODELS[name][0] * int(sum(R.stage_lengths(len(w))[1] for w in waves[:3]))      # the first three fit, then cuts
    assert V.plan_chunks([len(w) for w in waves], [1] + [MODELS[name][0]] * 6, mid)[0] == (0, min(3, n))
    c3, b3, _, _ = _front(links, waves, speakers, chunk_bytes=mid)
    for i in range(n):
        for c, b, what in ((c1, b1, 'a chunk of its own'), (c2, b2, 'one chunk'), (c3, b3, 'chunks of %d bytes' % mid)):
            _same_utterance(c[i], b[i], codes[i], blocks[i], 'utterance %d, %s' % (i, what))
    # device waves and a mixed list are the same list
    mixed = [gpu.to_device(w) if i % 2 else w.reshape(1, -1, 1) for i, w in enumerate(waves)]
    cm, bm, _, _ = _front(links, mixed, speakers)
    for i in range(n):
        _same_utterance(cm[i], bm[i], codes[i], blocks[i], 'utterance %d of the mixed host / device list' % i)
    # the corpus read in place, and a reordered view of it, against encode_many on the corpus's own samples
    corpus = V.ResidentCorpus(waves, speakers)
    flat = corpus.samples.get()
    own = [flat[int(o):int(o) + int(L)].copy() for o, L in zip(corpus.offsets, corpus.lengths)]
    want = V.encode_many(links[0], links[1], own).to_host()
    got = corpus.encode(links[0], links[1]).to_host()
    order = [4, 0, 6, 1] if n > 6 else [0]
    view = corpus.subset(order).encode(links[0], links[1], chunk_bytes=1).to_host()
    for i in range(n):
        assert np.array_equal(got[i], want[i]), 'corpus utterance %d' % i
    for j, u in enumerate(order):
        assert np.array_equal(view[j], want[u]), 'view position %d (utterance %d)' % (j, u)


def test_a_single_utterance_list(gpu):
    P, waves, speakers, ref = _case('m40')
    assert R.stage_lengths(len(waves[4])) == [2598, 1299, 649, 324, 162, 81, 40]
    codes, blocks, cond, _ = _front(_links(P), waves[4:5], speakers[4:5])
    assert len(codes) == 1 and codes[0].shape == (40,) and blocks[0].shape == (24, 40) and cond.shape == (1, 24 + G, 2560)
    assert np.array_equal(codes[0], ref[4][1])
    H.assert_close(blocks[0], ref[4][2], TOL, 'single utterance local')


# ---- 2. against the float64 restatement, 3. the indices ----------------------------------------------------------------
@pytest.mark.parametrize('name', ['m64', 'm40', 'm512'])
def test_values_against_float64_and_indices_bit_for_bit(gpu, matmul_mode, name):
    import vqvae_amd as V
    from vqvae_amd.core import Variable, no_backprop_mode, using_config
    from vqvae_amd.utils import _straight_through_node
    P, waves, speakers, ref = _case(name)
    enc, vq, ce = links = _links(P)
    # the precondition, on the float64 restatement: no row of any utterance is a near-tie between two codes
    for i, (z64, idx64, _) in enumerate(ref):
        best, second, _ = R.distance_gaps(z64, P['vq'])
        assert ((second - best) > 1e-3 * best).all(), 'utterance %d: the codebook does not separate its latents (gap %.2e)' % (
            i, ((second - best) / best).min())
    assert len(set(np.concatenate([r[1] for r in ref]).tolist())) >= 2
    codes, z = V.encode_many(enc, vq, waves, return_latents=True)
    codes = codes.to_host()
    _, blocks, cond, _ = _front(links, waves, speakers)
    for i, (z64, idx64, local64) in enumerate(ref):
        assert z[i].shape == z64.shape and z[i].dtype == np.float32
        H.assert_close(z[i], z64, TOL, '%s z of utterance %d' % (name, i))
        H.assert_close(blocks[i], local64, TOL, '%s condition stack of utterance %d' % (name, i))
        assert np.array_equal(codes[i], R.argmin_f32(z[i], P['vq'])), 'utterance %d: not the float32 argmin of its own z' % i
        assert np.array_equal(codes[i], idx64), 'utterance %d: not the codes of the float64 restatement' % i
        with using_config('train', False), no_backprop_mode():                    # the per-utterance n = 1 path
            z1 = enc(Variable(gpu.to_device(waves[i].reshape(1, 1, -1, 1))))
            _, node = _straight_through_node(z1, vq.W)
        assert np.array_equal(codes[i], node.indexes.get().reshape(-1)), 'utterance %d: not the n = 1 path\'s codes' % i


# ---- 4. the way back from stored codes ---------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['m64', 'm40'])
def test_condition_from_stored_codes(gpu, name, tmp_path):
    import vqvae_amd as V
    from vqvae_amd.core import Variable, no_backprop_mode, using_config
    from vqvae_amd.generation import LatentCondition
    from vqvae_amd.synthesis import _latent_condition
    P, waves, speakers, ref = _case(name)
    enc, vq, ce = links = _links(P)
    _, blocks, cond, codes = _front(links, waves, speakers)
    codes.save(str(tmp_path / 'codes'))
    for stored, kw in ((codes, {}), (V.LatentCodes.load(str(tmp_path / 'codes')), dict(chunk_bytes=1))):
        back = V.condition_many(vq, ce, stored, speakers, **kw)
        assert back.tl.tolist() == cond.tl.tolist() and (back.Cl, back.G, back.upscale) == (cond.Cl, G, 64)
        assert np.array_equal(_bits(back.local.get()), _bits(cond.local.get()))
        assert np.array_equal(_bits(back.global_vec.get()), _bits(cond.global_vec.get()))
    assert np.array_equal(cond.global_vec.get(), P['condition_embed']['global_embed'][speakers])
    other = V.condition_many(vq, ce, codes, (speakers + 1) % N_SPEAKER)           # other speakers, no second encoding
    assert np.array_equal(_bits(other.local.get()), _bits(cond.local.get()))
    assert np.array_equal(other.global_vec.get(), P['condition_embed']['global_embed'][(speakers + 1) % N_SPEAKER])
    singles = []
    with using_config('train', False), no_backprop_mode():
        for w, s in zip(waves, speakers):
            c = ce(vq(enc(Variable(gpu.to_device(w.reshape(1, 1, -1, 1))))), Variable(gpu.to_device(np.array([s], np.int32)))).data
            singles.append(_latent_condition(c, ce))
    want = LatentCondition.concatenate(singles).dense().get()
    got = cond.dense().get()
    assert got.shape == want.shape == (len(waves), cond.Cl + G, 64 * max(MODELS[name][5]))
    H.assert_close(got, want, TOL, 'dense condition against the per-utterance ConditionEmbed')


# ---- 5. synthesize_many with the batched front end ---------------------------------------------------------------------
def test_synthesize_many_with_the_batched_front_end(gpu):
    import vqvae_amd as V
    from vqvae_amd.core import Variable, no_backprop_mode, using_config
    from vqvae_amd.generation import LatentCondition
    from vqvae_amd.synthesis import _latent_condition
    from test_gpu_generate import _random_biases
    cfg = dict(H.SMALL)
    P, model = H.build_model(cfg, seed=145, tweak=_random_biases(146))
    model.to_gpu()
    enc, vq, dec, ce = links = (model.encoder, model.vq, model.decoder, model.condition_embed)
    sizes = (128, 64, 193, 320, 255)
    speaker = np.array([2, 5, 2, 0, 6], np.int32)
    ids = [11, 2 ** 40 + 7, 3, 2 ** 64 - 1, 0]
    waves = [O.synth_batch(1, length=L - 1, n_speaker=cfg['n_speaker'], seed=16 + i)[0].reshape(-1) for i, L in enumerate(sizes)]
    kw = dict(group=5, return_output=True, latent_condition=True, top_k=1)
    got = V.synthesize_many(*links, waves, speaker, rng=V.DeviceUniforms(7, ids), batched_frontend=True, **kw)
    cond = V.frontend_many(enc, vq, ce, waves, speaker)
    out = dec.generate_lockstep(cond, V.DeviceUniforms(7, ids), n_steps=None, lengths=cond.lengths, group=5, refill=True, top_k=1)
    wave = V.MuLaw(256).itransform(out)
    assert len(got) == 5 and cond.lengths.tolist() == [64 * R.latent_length(L) for L in sizes]
    for i, L in enumerate(cond.lengths):
        assert got[i][1].dtype == np.int32 and np.array_equal(got[i][1], out[i, :L]), 'utterance %d output' % i
        assert np.array_equal(_bits(np.asarray(got[i][0], np.float32)), _bits(np.asarray(wave[i, :L], np.float32)))
    # without the keyword the call is the parent's: the per-utterance loop, restated here
    plain = V.synthesize_many(*links, waves, speaker, rng=V.DeviceUniforms(7, ids), **kw)
    singles = []
    with using_config('train', False), no_backprop_mode():
        for w, s in zip(waves, speaker):
            xd = gpu.to_device(np.asarray(w, np.float32)).reshape(1, 1, w.size, 1)
            c = ce(vq(enc(Variable(xd))), Variable(gpu.to_device(np.array([s], np.int32)))).data
            singles.append(_latent_condition(c, ce))
    loop = LatentCondition.concatenate(singles)
    out1 = dec.generate_lockstep(loop, V.DeviceUniforms(7, ids), n_steps=None, lengths=loop.lengths, group=5, refill=True, top_k=1)
    for i, L in enumerate(loop.lengths):
        assert np.array_equal(plain[i][1], out1[i, :L]), 'utterance %d: the call without the keyword changed' % i


# ---- 6. red zones ------------------------------------------------------------------------------------------------------
def _tables(lens_in, window):
    K, stride, pad, dil = window
    lens_in = np.asarray(lens_in, np.int64)
    lens_out = np.array([O.conv_out_len(int(t), K, stride, pad, dil) for t in lens_in], np.int64)
    off_out = np.concatenate([[0], np.cumsum(lens_out)]).astype(np.int64)
    return lens_in.astype(np.int32), lens_out, off_out


def _conv_ref(x, off_in, lens_in, W, b, window, relu):
    K, stride, pad, dil = window
    outs = []
    for o, t in zip(off_in, lens_in):
        y = O.conv1d_fwd(x[None, :, int(o):int(o) + int(t)].astype(np.float64), W.astype(np.float64), b.astype(np.float64),
                         stride=stride, pad=pad, dil=dil)[0]
        outs.append(np.maximum(y, 0) if relu else y)
    return outs


@pytest.mark.parametrize('window, cin, cout, blocked', [((4, 2, 1, 1), 1, 70, False), ((4, 2, 1, 1), 40, 70, False),
                                                        ((3, 1, 16, 16), 40, 24, True), ((3, 1, 2, 2), 24, 40, False),
                                                        # 128 output channels and more: the 128 x 128-tile kernels
                                                        ((3, 1, 2, 2), 24, 130, False), ((4, 2, 1, 1), 40, 130, True),
                                                        ((3, 1, 1, 1), 17, 128, True)])
def test_conv_entry_point_under_red_zones(gpu, matmul_mode, window, cin, cout, blocked):
    from vqvae_amd import _lib
    rs = np.random.RandomState(cin + cout)
    lens_in, lens_out, off_out = _tables([5, 131, 2, 64, 33], window)
    gap = 3 if cin == 1 else 0                                   # stage 1 reads a corpus buffer in place: gaps allowed
    off_in = np.concatenate([[0], np.cumsum(lens_in[:-1] + gap)]).astype(np.int64)
    ttot_in = int(off_in[-1] + lens_in[-1])
    x = rs.standard_normal((cin, ttot_in)).astype(np.float32)
    W = (rs.standard_normal((cout, cin, window[0])) / np.sqrt(cin * window[0])).astype(np.float32)
    b = rs.standard_normal(cout).astype(np.float32)
    ttot = int(off_out[-1])
    d = _lib.RaggedConvDesc()
    d.n, d.cin, d.cout = len(lens_in), cin, cout
    d.K, d.stride, d.pad, d.dil = window
    d.relu, d.blocked_out, d.ttot_out, d.x_cstride = 1, int(blocked), ttot, ttot_in
    assert _lib.load().vqvae_ragged_conv_workspace_bytes(C.byref(d)) == 0        # exactly sized: there is none

    def fn(bufs):
        _lib.call('vqvae_ragged_conv_fwd', C.byref(d), bufs.x.ptr, bufs.off_in.ptr, bufs.len_in.ptr, bufs.off_out.ptr,
                  bufs.W.ptr, bufs.b.ptr, bufs.y.ptr, None, 0, gpu.stream())

    res = run_contract(gpu, fn, dict(x=In(x), off_in=In(off_in), len_in=In(lens_in), off_out=In(off_out), W=In(W), b=In(b),
                                     y=Out((cout * ttot,))))
    want = _conv_ref(x, off_in, lens_in, W, b, window, True)
    y = res['y']
    for i, w in enumerate(want):
        if blocked:
            got = y[cout * int(off_out[i]):cout * int(off_out[i + 1])].reshape(cout, -1)
        else:
            got = y.reshape(cout, ttot)[:, int(off_out[i]):int(off_out[i + 1])]
        H.assert_close(got, w, TOL, 'segment %d' % i)


def test_gathers_under_red_zones(gpu):
    from vqvae_amd import _lib
    rs = np.random.RandomState(9)
    k, d, ttot = 7, 40, 300
    Wc = rs.standard_normal((k, d)).astype(np.float32)
    idx = rs.randint(0, k, ttot).astype(np.int32)
    res = run_contract(gpu, lambda b: _lib.call('vqvae_ragged_code_gather', b.idx.ptr, b.W.ptr, ttot, d, k, b.e.ptr, gpu.stream()),
                       dict(idx=In(idx), W=In(Wc), e=Out((d, ttot))))
    assert np.array_equal(res['e'], Wc[idx].T)
    E = rs.standard_normal((N_SPEAKER, G)).astype(np.float32)
    spk = rs.randint(0, N_SPEAKER, 37).astype(np.int32)
    res = run_contract(gpu, lambda b: _lib.call('vqvae_ragged_speaker_gather', b.spk.ptr, b.E.ptr, 37, G, N_SPEAKER, b.g.ptr,
                                                gpu.stream()), dict(spk=In(spk), E=In(E), g=Out((37, G))))
    assert np.array_equal(res['g'], E[spk])


# ---- 7. mode 1 ---------------------------------------------------------------------------------------------------------
def test_matmul_mode_1_is_refused_by_name(gpu):
    import vqvae_amd as V
    from vqvae_amd._lib import HipError
    P, waves, speakers, _ = _case('m40')
    waves, speakers = waves[4:5], speakers[4:5]
    links = _links(P)
    gpu.set_matmul_dtype('bfloat16')
    try:
        with pytest.raises(HipError, match='matmul mode 1 \\(bf16 operands\\) is not supported by the ragged front end'):
            V.frontend_many(*links, waves, speakers)
    finally:
        gpu.set_matmul_dtype(gpu.default_matmul_dtype())
    codes, blocks, _, _ = _front(links, waves, speakers)                         # and the mode after it works as before
    assert codes[0].shape == (40,)
