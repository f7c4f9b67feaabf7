"""CPU checks of held-out scoring (vqvae_amd.scoring, include/vqvae_ragged_decoder.h): the float64 restatement against
the oracle, the host side of the rule (positions, chunk plan, refusals), and what is this header's own in the registry of
vqvae_amd/_lib.py -- its literal names, structs and limits and the source's place in the Makefile; the table against the
header text, the library and the compiler's layout is tests/test_host_abi.py."""
import os
import re

import numpy as np
import pytest

import abi_headers as A
import helpers as H
import scoring_ref as R
import vqvae_oracle as O

HEADER = 'vqvae_ragged_decoder.h'
TL = [1, 3, 2, 1, 5, 2]
L = [64 * t if i % 2 == 0 else 64 * t + 1 + i for i, t in enumerate(TL)]


# ---- the restatement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tl', [1, 3])
def test_the_restatement_reproduces_the_oracle_s_loss1(tl):
    cfg = dict(H.SMALL)
    rs = np.random.RandomState(4)
    P = O.make_params(rs, **cfg)
    H.named_tweak('biases:4')(P)
    P64 = R.cast_tree(P, np.float64)
    x_enc, x_dec, spk, t = O.synth_batch(1, length=64 * tl, n_speaker=cfg['n_speaker'], seed=21, dtype=np.float64)
    (loss1, _, _), cache = O.vae_forward(P64, x_enc, x_dec, spk, t, cfg['n_loop'], cfg['n_layer'])
    q = np.concatenate([np.argmax(x_dec[0], axis=0), t[0, -1:]])                   # L = 64 tl + 1 classes
    assert len(q) == 64 * tl + 1 and np.array_equal(q[1:], t[0])
    local = cache['ce_hs'][-1][0]
    gvec = P64['condition_embed']['global_embed'][spk[0]]
    r = R.score_utterance(P['decoder'], q, local, gvec, cfg['n_loop'], cfg['n_layer'])
    assert r['n'] == 64 * tl and r['nll'].dtype == np.float64
    assert abs(r['nll'].sum() / r['n'] - loss1) <= 1e-12 * max(1.0, abs(loss1)), (r['nll'].sum() / r['n'], loss1)
    np.testing.assert_allclose(R.dense_condition(local, gvec), cache['cond'], rtol=0, atol=1e-12)
    assert np.array_equal(r['hit'], np.argmax(cache['y'][0], axis=0) == t[0])


def test_the_restated_reduce_order():
    from vqvae_amd import scoring
    v = np.arange(1, 601, dtype=np.float32)
    assert R.reduce_order(v) == v.astype(np.float64).sum() == scoring.reduce_order(v)
    big = np.array([1e16, 1.0, -1e16, 1.0] * 64 + [1.0], np.float32)
    lanes = [big[t::256].astype(np.float64) for t in range(256)]
    s = [float(np.add.reduce(x)) if x.size < 3 else None for x in lanes]
    assert None not in s
    h = 128
    while h:
        s = [s[k] + s[k + h] for k in range(h)]
        h //= 2
    assert R.reduce_order(big) == s[0] == scoring.reduce_order(big)
    assert R.reduce_order(np.array([1, 0, 1, 1], np.int32)) == 3


# ---- positions, the chunk plan, the refusals -------------------------------------------------------------------------------------
DIMS = dict(R=64, D=128, S=64, Q=256, Cc=72, n_blocks=8)


def test_positions_and_the_chunk_plan():
    from vqvae_amd import scoring
    n = scoring.positions(L, TL, 64)
    assert n.tolist() == [63, 192, 127, 64, 319, 128] == [R.positions(l, t) for l, t in zip(L, TL)]
    assert scoring.latent_lengths(L, 64).tolist() == TL
    with pytest.raises(ValueError, match='utterance 1 '):
        scoring.positions([64, 1, 64], [1, 1, 1], 64)
    per = scoring.chunk_elements(n, TL, L, DIMS)
    assert per.shape == (7, 6) and per[0].tolist() == (64 * n).tolist() and per[5].tolist() == [8 * 128 * t for t in TL]
    assert scoring.plan_chunks(n, TL, L, DIMS, 1 << 30) == [(0, 6)]
    alone = 4 * int(per.max())
    assert scoring.plan_chunks(n, TL, L, DIMS, alone) == [(0, 2), (2, 4), (4, 5), (5, 6)]
    three = 4 * 64 * int(n[3:5].sum())
    assert scoring.plan_chunks(n, TL, L, DIMS, three) == [(0, 3), (3, 5), (5, 6)]
    with pytest.raises(ValueError, match='utterance 4 .* does not fit a chunk'):
        scoring.plan_chunks(n, TL, L, DIMS, alone - 1)
    assert scoring.chunk_elements(n, TL, L, DIMS, logits=True).shape == (8, 6)


def _host_wavenet(**kw):
    from vqvae_amd.wavenet import WaveNet
    a = dict(n_loop=1, n_layer=2, filter_size=2, Q=16, R=8, D=8, S=8, use_logistic=False, Cc=6)
    a.update(kw)
    wn = WaveNet(a['n_loop'], a['n_layer'], a['filter_size'], a['Q'], a['R'], a['D'], a['S'], a['Q'], a['use_logistic'], 10, -40, a['Cc'], 0)
    rs = np.random.RandomState(0)
    for _, p in wn.namedparams():
        if p.data is None:
            continue
        p.data = rs.standard_normal(p.data.shape).astype(np.float32)
    return wn


def _waves(lengths):
    return [np.linspace(-1, 1, n).astype(np.float32) for n in lengths]


def test_every_refusal_names_its_reason():
    import vqvae_amd as V
    from vqvae_amd import _lib, scoring
    cond = V.LatentCondition([1, 2], 4, 2, 64)
    waves = _waves([64, 129])
    with pytest.raises(NotImplementedError, match='mixture-of-logistics'):
        V.score_many(_host_wavenet(use_logistic=True), cond, waves)
    with pytest.raises(ValueError, match='filter_size 3'):
        V.score_many(_host_wavenet(filter_size=3), cond, waves)
    wn = _host_wavenet()
    with pytest.raises(TypeError, match='LatentCondition'):
        V.score_many(wn, np.zeros((2, 6, 128), np.float32), waves)
    with pytest.raises(ValueError, match='utterance 1 has 200 samples, that is 3 latent frames, but the condition holds 2'):
        V.score_many(wn, cond, _waves([64, 200]))
    with pytest.raises(ValueError, match='2 utterances against a condition of 3'):
        V.score_many(wn, V.LatentCondition([1, 2, 1], 4, 2, 64), waves)
    with pytest.raises(ValueError, match='utterance 1 .* does not fit a chunk'):
        V.score_many(wn, cond, waves, chunk_bytes=4 * 8 * 128 - 1)
    with pytest.raises(ValueError, match='utterance 0 holds class 16'):
        V.score_many(wn, cond, [np.full(64, 16, np.int32), np.zeros(129, np.int32)])
    with pytest.raises(ValueError, match='return_logits'):
        V.score_many(wn, V.LatentCondition([2000], 4, 2, 64), _waves([128000]), return_logits=True)
    with pytest.raises(ValueError, match='4 \\+ 3 channels, the decoder projects 6'):
        V.score_many(wn, V.LatentCondition([1, 2], 4, 3, 64), waves)
    lib = _lib.load()
    before = lib.vqvae_get_matmul_dtype()
    try:
        assert lib.vqvae_set_matmul_dtype(1) == 0
        with pytest.raises(ValueError, match='matmul mode 1'):
            V.score_many(wn, cond, waves)
    finally:
        assert lib.vqvae_set_matmul_dtype(before) == 0
    with pytest.raises(ValueError, match='not on the device'):                  # every host-side check passed: the parameters are asked for last
        V.score_many(wn, cond, waves)
    assert scoring.MAX_LOGIT_COLUMNS == 1 << 16


# ---- the header, the table -----------------------------------------------------------------------------------------------------
NAMES = {'vqvae_ragged_decoder_abi_version', 'vqvae_rdec_workspace_bytes', 'vqvae_rdec_embed', 'vqvae_rdec_cond_project',
         'vqvae_rdec_cond_global', 'vqvae_rdec_gate', 'vqvae_rdec_res_skip', 'vqvae_rdec_head', 'vqvae_rdec_reduce'}


def test_the_header_is_in_the_registry_and_scoring_binds_nothing():
    from vqvae_amd import _lib, scoring
    h = _lib.HEADERS[HEADER]                                   # against the header and the library: tests/test_host_abi.py
    assert set(h.prototypes) == NAMES and len(NAMES) == 9 and h.words == 'ragged-decoder ABI' and h.version == 1
    assert HEADER in os.listdir(A.INCLUDE) and not any('abi_version' in open(os.path.join(A.CSRC, f)).read() for f in os.listdir(A.CSRC) if f.endswith('.h'))
    assert set(A.structs(HEADER)) == {'vqvae_rdec_desc', 'vqvae_rdec_tables'}
    assert (_lib.RdecDesc._c_name_, _lib.RdecTables._c_name_) == ('vqvae_rdec_desc', 'vqvae_rdec_tables')
    assert [f for f, _ in _lib.RdecDesc._fields_] == ['n', 'R', 'D', 'S', 'Q', 'Cl', 'G', 'n_blocks', 'upscale', 'reserved', 'ttot', 'tltot']
    assert [f for f, _ in _lib.RdecTables._fields_] == ['off', 'qoff', 'latoff', 'tl']
    assert sorted(A.macros(HEADER)) == ['VQVAE_RAGGED_DECODER_MAX_CLASSES', 'VQVAE_RAGGED_DECODER_MAX_DILATION',
                                        'VQVAE_RAGGED_DECODER_REDUCE_LANES']
    assert (_lib.RAGGED_DECODER_MAX_CLASSES, _lib.RAGGED_DECODER_MAX_DILATION, _lib.RAGGED_DECODER_REDUCE_LANES) == (512, 512, 256)
    assert (scoring.MAX_CLASSES, scoring.MAX_DILATION, scoring.REDUCE_LANES) == (512, 512, 256) and R.LANES == scoring.REDUCE_LANES
    for name in ('HEADER', 'ABI_WORDS', 'ABI_VERSION', 'PROTOTYPES', 'STRUCTS', '_bound', 'load', 'call', 'RdecDesc', 'RdecTables'):
        assert not hasattr(scoring, name), name


def test_the_source_is_built_and_depends_on_its_header():
    srcs = re.search(r'^SRCS\s*:?=\s*(.*)$', A.make_database(), flags=re.M).group(1).split()
    assert 'ragged_decoder.hip' in srcs
    assert HEADER in [os.path.basename(p) for p in A.object_rule_prerequisites()]


def test_the_package_exports_the_calls():
    import vqvae_amd as V
    from vqvae_amd import scoring
    assert V.score_many is scoring.score_many and V.evaluate_many is scoring.evaluate_many and V.Scores is scoring.Scores
    assert callable(V.ResidentCorpus.score) and callable(V.CorpusView.score)
    s = V.Scores(np.array([np.log(2.0) * 6, np.log(2.0) * 2]), np.array([3, 2], np.int64), np.array([1, 2], np.int64))
    np.testing.assert_allclose(s.bits_per_sample, [2.0, 1.0], rtol=1e-15)
    assert abs(s.total() - 8.0 / 5.0) < 1e-15 and s.accuracy.tolist() == [1.0 / 3.0, 1.0]
