"""CPU checks of mixture-of-logistics scoring (vqvae_amd.scoring_mol, csrc/ragged_mol.h): the float64 restatement against
the oracle and against the reference's own fixture, the host side (chunk plan, MolScores, every refusal), and the binding
of the header that scoring_mol.py carries itself -- the declared functions, parameter counts, the revision error, the
source's place in the Makefile, the refusals the library makes before it launches."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import abi_headers as A
import helpers as H
import ref_model as RM
import scoring_mol_ref as R
import vqvae_oracle as O

HEADER = os.path.join(A.CSRC, 'ragged_mol.h')
E_INVALID = -1                                                         # VQVAE_E_INVALID


# ---- the restatement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tl', [1, 3])
def test_the_restatement_reproduces_the_oracle_s_mol_loss1(tl):
    cfg = dict(H.MOL_SHALLOW)
    P = O.make_params(np.random.RandomState(4), **cfg)
    H.named_tweak('mol_output+biases:4')(P)
    P64 = R.cast_tree(P, np.float64)
    x_enc, x_dec, spk, t = O.synth_batch_raw(1, length=64 * tl, n_speaker=cfg['n_speaker'], seed=21, dtype=np.float64)
    (loss1, _, _), cache = O.vae_forward(P64, x_enc, x_dec, spk, t, cfg['n_loop'], cfg['n_layer'], loss_kind='mol')
    wave = x_enc[0, 0].astype(np.float32)                                          # L = 64 tl + 1 samples
    assert len(wave) == 64 * tl + 1 and np.array_equal(wave.astype(np.float64), x_enc[0, 0])
    local = cache['ce_hs'][-1][0]
    gvec = P64['condition_embed']['global_embed'][spk[0]]
    r = R.score_utterance_mol(P['decoder'], wave, local, gvec, cfg['n_loop'], cfg['n_layer'])
    assert r['n'] == 64 * tl and r['nll'].dtype == np.float64 and r['params'].shape == (30, 64 * tl)
    assert abs(r['nll'].sum() / r['n'] - loss1) <= 1e-12 * max(1.0, abs(loss1)), (r['nll'].sum() / r['n'], loss1)


def test_the_restated_terms_average_to_the_reference_s_loss():
    """On the crafted input (both tails, both sides of +-0.999, clamped scales, a saturated term), in float64, at the bar
    test_oracle_mol_loss_matches_reference holds the oracle to."""
    fx = RM.load('ref_mol_loss.npz')
    y, t = RM.crafted_mol_inputs(fx['meta']['seed'])
    assert fx['meta']['seed'] == 8
    nll = R.mol_nll(y.astype(np.float64), t.astype(np.float64))
    assert nll.shape == (2, 64)
    H.assert_close(nll.mean(), float(fx['loss']), 1e-9, 'mean of the per-position terms')
    assert not R.at_floor(y.astype(np.float64), t).any()


def test_embed_bits_by_hand():
    W = np.array([[[2.0, 3.0]], [[-1.0, 0.5]]], np.float32)
    w = [np.array([1.0, -2.0, 4.0], np.float32), np.array([0.25, 8.0], np.float32)]
    got = R.embed_bits(W, np.array([10.0, 20.0], np.float32), w, [2, 1])
    assert got.dtype == np.float32 and np.array_equal(got, [[13.0, 6.0, 10.75], [20.5, 18.0, 20.125]])
    assert np.array_equal(R.embed_bits(W, None, w, [2, 1]), [[3.0, -4.0, 0.75], [0.5, -2.0, 0.125]])
    neg = R.embed_bits(np.array([[[1.0, -1.0]]], np.float32), None, [np.zeros(2, np.float32)], [1])
    assert np.signbit(neg[0, 0])                                                   # the second product alone: -0.0 stays


# ---- the chunk plan, MolScores, the refusals -------------------------------------------------------------------------------------
TL = [1, 3, 2, 1, 5, 2]
L = [64 * t if i % 2 == 0 else 64 * t + 1 + i for i, t in enumerate(TL)]


def test_the_chunk_plan_counts_the_output_and_the_classes_only_when_read():
    from vqvae_amd import scoring, scoring_mol
    n = scoring.positions(L, TL, 64)
    base = dict(R=8, D=8, S=8, Q=30, M=10, Cc=6, n_blocks=2)
    sample, classes = dict(base, Qin=1), dict(base, Qin=16)
    ps, pc = scoring_mol.chunk_elements(n, TL, L, sample), scoring_mol.chunk_elements(n, TL, L, classes)
    assert ps.shape == (7, 6) and pc.shape == (8, 6)
    assert ps[-1].tolist() == (30 * n).tolist() == pc[-1].tolist() and pc[6].tolist() == L and ps[5].tolist() == [2 * 8 * t for t in TL]
    assert scoring_mol.plan_chunks(n, TL, L, sample, 1 << 30) == [(0, 6)]
    alone = 4 * int(ps.max())
    assert alone == 4 * 30 * 319 and len(scoring_mol.plan_chunks(n, TL, L, sample, alone)) == 4
    with pytest.raises(ValueError, match='utterance 4 .* does not fit a chunk'):
        scoring_mol.plan_chunks(n, TL, L, sample, alone - 1)
    with pytest.raises(ValueError, match='chunk_bytes must be positive'):
        scoring_mol.plan_chunks(n, TL, L, sample, 0)


def test_mol_scores_arithmetic():
    import vqvae_amd as V
    from vqvae_amd import scoring_mol
    assert V.score_many_mol is scoring_mol.score_many_mol and V.evaluate_many_mol is scoring_mol.evaluate_many_mol
    assert V.MolScores is scoring_mol.MolScores and callable(V.ResidentCorpus.score_mol) and V.CorpusView.score_mol is V.ResidentCorpus.score_mol
    s = V.MolScores(np.array([np.log(2.0) * 6, np.log(2.0) * 2]), np.array([3, 2], np.int64))
    np.testing.assert_allclose(s.bits_per_sample, [2.0, 1.0], rtol=1e-15)
    assert abs(s.total() - 8.0 / 5.0) < 1e-15 and len(s) == 2 and s.params is None
    assert not hasattr(s, 'hits') and not hasattr(s, 'accuracy')
    with pytest.raises(ValueError, match='without per_sample=True'):
        s.sample_nll(0)
    assert 'LINEAR amplitude grid' in V.MolScores.__doc__ and 'NOT comparable' in V.MolScores.__doc__


def _host_wavenet(**kw):
    from vqvae_amd.wavenet import WaveNet
    a = dict(n_loop=1, n_layer=2, filter_size=2, Qin=1, R=8, D=8, S=8, rows=30, use_logistic=True, Cc=6)
    a.update(kw)
    wn = WaveNet(a['n_loop'], a['n_layer'], a['filter_size'], a['Qin'], a['R'], a['D'], a['S'], 256, a['use_logistic'], a['rows'], -40,
                 a['Cc'], 0)
    rs = np.random.RandomState(0)
    for _, p in wn.namedparams():
        if p.data is None:
            continue
        p.data = rs.standard_normal(p.data.shape).astype(np.float32)
    return wn


def _waves(lengths):
    return [np.linspace(-1, 1, n).astype(np.float32) for n in lengths]


def test_every_refusal_names_its_reason():
    """None of these calls reaches the device."""
    import vqvae_amd as V
    from vqvae_amd import _lib
    cond = V.LatentCondition([1, 2], 4, 2, 64)
    waves = _waves([64, 129])
    with pytest.raises(ValueError, match='softmax output .*score_many'):
        V.score_many_mol(_host_wavenet(use_logistic=False, rows=16), cond, waves)
    with pytest.raises(NotImplementedError, match='mixture-of-logistics'):           # the sibling keeps refusing the same link
        V.score_many(_host_wavenet(), cond, waves)
    for rows in (31, 51, 2):
        with pytest.raises(ValueError, match='writes %d rows; a mixture of M logistics has 3 M .* 1 <= M <= 16' % rows):
            V.score_many_mol(_host_wavenet(rows=rows), cond, waves)
    with pytest.raises(ValueError, match='filter_size 3'):
        V.score_many_mol(_host_wavenet(filter_size=3), cond, waves)
    with pytest.raises(ValueError, match='dilation 1024, outside 1 .. 512'):
        V.score_many_mol(_host_wavenet(n_layer=11), cond, waves)
    wn = _host_wavenet()
    lib = _lib.load()
    before = lib.vqvae_get_matmul_dtype()
    try:
        assert lib.vqvae_set_matmul_dtype(1) == 0
        with pytest.raises(ValueError, match='matmul mode 1'):
            V.score_many_mol(wn, cond, waves)
    finally:
        assert lib.vqvae_set_matmul_dtype(before) == 0
    with pytest.raises(TypeError, match='LatentCondition'):
        V.score_many_mol(wn, np.zeros((2, 6, 128), np.float32), waves)
    with pytest.raises(ValueError, match='4 \\+ 3 channels, the decoder projects 6'):
        V.score_many_mol(wn, V.LatentCondition([1, 2], 4, 3, 64), waves)
    with pytest.raises(ValueError, match='2 utterances against a condition of 3'):
        V.score_many_mol(wn, V.LatentCondition([1, 2, 1], 4, 2, 64), waves)
    with pytest.raises(ValueError, match='utterance 1 has 200 samples, that is 3 latent frames, but the condition holds 2'):
        V.score_many_mol(wn, cond, _waves([64, 200]))
    with pytest.raises(TypeError, match='int32 class arrays, but the target of a mixture of logistics is the sample'):
        V.score_many_mol(wn, cond, [np.zeros(64, np.int32), np.zeros(129, np.int32)])
    with pytest.raises(ValueError, match='return_params'):
        V.score_many_mol(wn, V.LatentCondition([2000], 4, 2, 64), _waves([128000]), return_params=True)
    with pytest.raises(ValueError, match='utterance 1 .* does not fit a chunk'):
        V.score_many_mol(wn, cond, waves, chunk_bytes=4 * 30 * 128 - 1)
    for call in (lambda: V.score_many_mol(wn, cond, waves), lambda: V.score_many_mol(_host_wavenet(Qin=16), cond, waves),
                 lambda: V.ResidentCorpus.describe([64, 129], [0, 1]).score_mol(wn, cond)):
        with pytest.raises((ValueError, RuntimeError), match='not on the device|description only'):   # every host-side check passed
            call()
    with pytest.raises(ValueError, match='softmax output'):                          # before the front end is run
        V.evaluate_many_mol(None, None, None, _host_wavenet(use_logistic=False, rows=16), waves, [0, 1])


# ---- the header scoring_mol.py binds itself --------------------------------------------------------------------------------------
def _code():
    text = open(HEADER).read()
    return re.sub(r'//[^\n]*', '', re.sub(r'/\*.*?\*/', '', text, flags=re.S))


def test_the_header_is_under_csrc_and_outside_the_registry():
    from vqvae_amd import _lib, scoring_mol
    assert os.path.exists(HEADER) and scoring_mol.HEADER == 'ragged_mol.h' and scoring_mol.HEADER not in os.listdir(A.INCLUDE)
    assert 'abi_version' not in open(HEADER).read()
    assert not any(n in h.prototypes for n in scoring_mol.PROTOTYPES for h in _lib.HEADERS.values())
    assert not any('RDMOL' in n.upper() for n in vars(_lib))
    assert '#include "../../include/vqvae_ragged_decoder.h"' in _code() and not re.search(r'typedef\s+struct', _code())
    assert re.findall(r'^[ \t]*#[ \t]*define[ \t]+(VQVAE_\w+)[ \t]+(\d+)', _code(), flags=re.M) == [('VQVAE_RDMOL_MAX_MIX', '16')]
    assert scoring_mol.MAX_MIX == 16


def test_declared_functions_equal_the_bound_table():
    from vqvae_amd import scoring_mol
    declared = sorted(set(re.findall(r'\b(vqvae_[a-z0-9_]+)\s*\(', _code())))
    assert declared == sorted(scoring_mol.PROTOTYPES) and len(declared) == 3
    for name, (res, args) in scoring_mol.PROTOTYPES.items():
        found = re.findall(r'\b%s\s*\(([^()]*)\)\s*;' % name, _code())
        assert len(found) == 1, name
        params = found[0].strip()
        assert (0 if params == 'void' else len(params.split(','))) == len(args), (name, params)
    lib = scoring_mol.load()
    for name, (res, args) in scoring_mol.PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert lib.vqvae_rdmol_revision() == scoring_mol.REVISION == 1


def test_a_bumped_revision_is_the_exact_import_error(monkeypatch):
    from vqvae_amd import _lib, scoring_mol
    monkeypatch.setattr(scoring_mol, '_bound', None)
    monkeypatch.setattr(scoring_mol, 'REVISION', 2)
    with pytest.raises(ImportError) as e:
        scoring_mol.load()
    assert str(e.value) == ('libvqvae_hip.so at %s has mixture-of-logistics scoring revision 1, this package binds 2: rebuild '
                            'it (__graft_entry__.build())' % _lib.LIB_PATH)
    assert scoring_mol._bound is None


def test_the_source_is_built_and_depends_on_its_header():
    srcs = re.search(r'^SRCS\s*:?=\s*(.*)$', A.make_database(), flags=re.M).group(1).split()
    assert 'ragged_mol.hip' in srcs
    assert 'ragged_mol.h' in [os.path.basename(p) for p in A.object_rule_prerequisites()]
    src = open(os.path.join(A.CSRC, 'ragged_mol.hip')).read()
    launched = set(re.findall(r'hipLaunchKernelGGL\(\(?(\w+)', src))
    assert launched == {'rdmol_embed_kernel', 'rdmol_nll_kernel'}
    assert not any(taken in k for k in launched for taken in ('rd_embed_kernel', 'rd_gvec_kernel', 'rd_reduce_kernel', 'rd_gemm_kernel'))


def test_bad_arguments_are_refused_on_the_host_side_of_the_library():
    """The entry points validate before they launch, so the refusals can be had without a device."""
    from vqvae_amd import _lib, scoring_mol
    lib = scoring_mol.load()
    one = C.c_void_p(256)                                                # never dereferenced: every call below is refused
    good = lambda **kw: _lib.RdecDesc(**dict(dict(n=2, R=8, D=8, S=8, Q=30, Cl=4, G=2, n_blocks=2, upscale=64, reserved=0, ttot=100, tltot=3), **kw))
    tb = _lib.RdecTables(256, 256, 256, 256)
    embed = lambda d, t=tb, w=one, woff=one, W=one, x=one: lib.vqvae_rdmol_embed(d, t, w, woff, W, None, x, None)
    nll = lambda d, t=tb, y=one, w=one, woff=one, M=10, q=256, out=one: lib.vqvae_rdmol_nll(d, t, y, w, woff, M, q, -40.0, out, None)
    msg = lambda: lib.vqvae_last_error_string().decode()
    for who, entry in (('rdmol_embed', embed), ('rdmol_nll', nll)):
        assert entry(None) == E_INVALID and who + ': null descriptor' in msg()
        for field, value in (('n', 0), ('D', 7), ('Q', 513), ('Cl', 0), ('ttot', 0), ('ttot', 1 << 31), ('tltot', 0), ('upscale', 0)):
            assert entry(C.byref(good(**{field: value}))) == E_INVALID and who + ': a descriptor the ragged decoder refuses' in msg(), (who, field)
        assert entry(C.byref(good()), t=None) == E_INVALID and who + ': null tables or off' in msg()
        assert entry(C.byref(good()), t=C.byref(_lib.RdecTables(None, 256, 256, 256))) == E_INVALID and who + ': null tables or off' in msg()
    for kw in (dict(w=None), dict(woff=None), dict(W=None), dict(x=None)):
        assert embed(C.byref(good()), **kw) == E_INVALID and 'rdmol_embed: null w, woff, W or x' in msg(), kw
    for kw in (dict(y=None), dict(w=None), dict(woff=None), dict(out=None)):
        assert nll(C.byref(good()), **kw) == E_INVALID and 'rdmol_nll: null y, w, woff or nll' in msg(), kw
    for M in (0, 17, -1):
        assert nll(C.byref(good(Q=max(3 * M, 3))), M=M) == E_INVALID and 'n_mix must be in 1 .. 16 (got %d)' % M in msg()
    assert nll(C.byref(good(Q=29))) == E_INVALID and "Q must be 3 n_mix = 30 (got 29)" in msg()
    assert nll(C.byref(good()), q=1) == E_INVALID and 'quantize must be at least 2 (got 1)' in msg()


def test_the_package_imports_without_a_library_call():
    code = ('import vqvae_amd as V, vqvae_amd._lib as L, vqvae_amd.scoring_mol as S; '
            'assert L._lib is None and S._bound is None; '
            'assert all(getattr(V, n) is getattr(S, n) for n in ("score_many_mol", "evaluate_many_mol", "MolScores"))')
    env = dict(os.environ, PYTHONPATH=os.path.join(A.ROOT, 'chainer-vq-vae_amd'))
    subprocess.check_call([sys.executable, '-c', code], env=env)
