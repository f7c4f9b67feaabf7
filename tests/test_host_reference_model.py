"""The oracle against the reference's own model code, as executed.

tests/golden/ref_*.npz hold what the reference's ``net.py``, ``WaveNet/modules.py``, ``updaters.py`` and the
``VQ`` / ``ExponentialMovingAverage`` links of ``utils.py`` computed in float64 on the Chainer stand-in
(tests/golden/make_golden_model.py).  They pin the COMPOSITION: which half of the gate goes
through tanh, which end the causal crop keeps, what is detached in loss2 / loss3 and where beta sits, the three
backward() calls around vq.cleargrads(), the roles of ``decay`` in the EMA, the concat order of the condition, the
generation queues, the MoL branches.  The primitives under them stay where test_oracle_torch.py left them.

CPU, NumPy only.  Bars: the project's assert_close / assert_close_scaled at 1e-4, except where a docstring below
records a measured float32-oracle-versus-float64 error and a bar of twice that."""
import copy
import importlib.util
import json
import os

import numpy as np
import pytest

import helpers as H
import ref_model as R
import vqvae_oracle as O
from helpers import assert_close, assert_close_scaled

# The float32 oracle against the float64 fixture, MoL model, measured on the CPU as max over the parameters of
# max |g - g_ref| / max |g_ref| (what assert_close_scaled bounds): 3.99e-4 at /decoder/resnet/0/conv/W, then 2.5e-4
# (local_embed3/W), 2.3e-4 (decoder/embed/W), 2.3e-4, 2.3e-4 (encoder/conv1/W), 2.2e-4; the cdf_plus - cdf_min cancellation that
# test_mol_deep_stack_matches_oracle describes.  The SAME oracle run in float64 is within 5.4e-8 of the fixture (the
# float32 rounding of the stored tensors), so the error is float32 arithmetic, not a reading.  Bar: twice the measured.
MOL_ORACLE_ERR = 3.99e-4
MOL_GRAD_BAR = 2 * MOL_ORACLE_ERR
# Gradient tensors are stored rounded to float32: half an ulp, 2^-24 of the element, at most 2^-24 of the tensor's
# maximum.  A float64 evaluation of the same composition differs by that and by float64 summation noise (1e-13):
# the bar is 2^-23.  Measured: 5.5e-8 (softmax), 5.4e-8 (MoL).
F64_GRAD_BAR = 2.0 ** -23


def _to64(P):
    if isinstance(P, dict):
        return {k: _to64(v) for k, v in P.items()}
    if isinstance(P, (list, tuple)):
        return type(P)(_to64(v) for v in P)
    return P.astype(np.float64) if P.dtype.kind == 'f' else P


def _params(meta):
    P = O.make_params(np.random.RandomState(meta['param_seed']), **meta['cfg'])
    H.named_tweak(meta['tweak'])(P)
    return P


def _batch(meta):
    synth = O.synth_batch_raw if meta.get('use_logistic') else O.synth_batch
    return synth(meta['B'], length=meta['length'], n_speaker=meta['cfg']['n_speaker'], seed=meta['batch_seed'])


def _chainer_shape(a):
    return a.shape + (1,) if a.ndim == 3 else a.shape


def oracle_step(fx, float64=False):
    """One oracle train_step at the fixture's seeds -> (losses, cache, gradients by Chainer name)."""
    meta = fx['meta']
    cfg = meta['cfg']
    P, batch = _params(meta), _batch(meta)
    if float64:
        P, batch = _to64(P), _to64(batch)
    losses, cache, G = O.train_step(P, {}, batch, cfg['n_loop'], cfg['n_layer'],
                                    loss_kind='mol' if meta['use_logistic'] else 'softmax')
    return losses, cache, {H._dev_name(n, False): g for n, g in G.items()}


def check_step(name, grad_tol=1e-4, float64=False):
    fx = R.load(name)
    losses, cache, grads = oracle_step(fx, float64)
    R.compare_step(fx, losses, cache['idx'], grads, 1e-10 if float64 else 1e-4, grad_tol, z=cache['z'], e=cache['e'],
                   cond=cache['cond'], y=cache['y'], what='float64 oracle' if float64 else 'oracle')


def check_ema():
    fx = R.load('ref_model_ema.npz')
    meta = fx['meta']
    cfg = meta['cfg']
    batch = _batch(meta)
    for decay in meta['decays']:
        P = _params(meta)
        ema = copy.deepcopy(P['decoder'])
        for call in (1, 2):
            for (_, a), (_, b) in zip(O.flatten_params(ema), O.flatten_params(P['decoder'])):
                O.ema_update(a, b, decay)                                 # what train_step does at forward time
            for i, (n, a) in enumerate(O.flatten_params(ema)):
                got, want = R.sampled(fx, 'ema_%s_call%d_%03d' % (R.decay_tag(decay), call, i), i, a, R.N_EMA, R.N_EMA)
                assert_close(got, want, 1e-5, 'ema %g call %d %s' % (decay, call, n))
            if call == 1:
                R.perturb(meta, [a for _, a in O.flatten_params(P['decoder'])])
        (l1, _, _), _ = O.vae_forward(dict(P, decoder=ema), *batch, cfg['n_loop'], cfg['n_layer'])
        assert_close(float(l1), float(fx['eval_loss1_' + R.decay_tag(decay)]), 1e-4, 'evaluation loss1, decay %g' % decay)


def check_generate():
    fx = R.load('ref_generate.npz')
    for tag in ('softmax', 'mol'):
        meta = fx[tag + '_meta']
        cfg = meta['cfg']
        p = _params(meta)['decoder']
        cond, forced = fx[tag + '_cond'], fx[tag + '_forced']
        T, n = forced.shape
        u = np.full((T, n) if tag == 'softmax' else (T, n, cfg['out_dim'] // 3), 0.5)
        st = O.wavenet_initialize(p, n, cfg['n_loop'], cfg['n_layer'])
        assert [q.shape[2] for q in st['queues']] == [d + 1 for d in O.wavenet_dilations(cfg['n_loop'], cfg['n_layer'])]
        assert not any(q.any() for q in st['queues']) and not st['embed_queue'].any()
        _, logits = O.wavenet_generate(p, cond, u, cfg['n_loop'], cfg['n_layer'], loss_kind=tag, forced=forced)
        assert logits.shape == fx[tag + '_logits'].shape == (meta['steps'], n, cfg['out_dim'])
        assert_close(logits, fx[tag + '_logits'], 1e-4, tag + ' teacher-forced logits')


def check_everything():
    check_step('ref_model_softmax.npz')
    check_ema()
    check_generate()


# --------------------------------------------------------------------------- #
def test_fixture_margins_and_sizes():
    """Every VQ row of the model fixtures is decided by more than 1e-3 of its best squared distance (the generator
    also ran the model in float32 and required equal indices): the bit-exact index comparisons are no coin toss."""
    total = 0
    for name in ('ref_model_softmax.npz', 'ref_model_mol.npz', 'ref_model_ema.npz', 'ref_mol_loss.npz',
                 'ref_generate.npz', 'ref_params.json'):
        size = os.path.getsize(os.path.join(R.GOLD, name))
        assert size <= R.MAX_BYTES, name
        total += size
    assert total < 1000000
    for name in ('ref_model_softmax.npz', 'ref_model_mol.npz'):
        fx = R.load(name)
        assert fx['margins'].shape == (fx['idx'].size,) and fx['margins'].min() > R.MARGIN, name
        assert fx['meta']['B'] == 2 and fx['meta']['length'] == 512 and fx['idx'].size == 16
        W = _params(fx['meta'])['vq']
        np.testing.assert_array_equal(W[fx['idx'].reshape(2, -1)].transpose(0, 2, 1).astype(np.float64),
                                      fx['e'][..., 0])


@pytest.mark.parametrize('name,ema', [('ref_model_softmax.npz', False), ('ref_model_mol.npz', False),
                                      ('ref_model_ema.npz', True)])
def test_parameter_names_and_shapes(name, ema):
    """flatten_params under helpers._dev_name gives the reference's namedparams(): same names, same order, same
    shapes.  The ORDER (registration order; the EMA wrapper lists target before ema) is the stand-in's choice, not a
    fact about Chainer or the reference: it is asserted because the fixtures number their tensors by it and the
    comparisons of this file pair them with flatten_params' arrays by position."""
    fx = R.load(name)
    flat = O.flatten_params(_params(fx['meta']))
    if not ema:
        assert [H._dev_name(n, False) for n, _ in flat] == [str(n) for n in fx['names']]
        assert [list(_chainer_shape(a)) for _, a in flat] == json.loads(str(fx['shapes_json']))
    else:
        dec = [(n, a) for n, a in flat if n.startswith('/decoder/')]
        want = [(n, a) for n, a in flat if not n.startswith('/decoder/')]
        want += [(H._dev_name(n, True), a) for n, a in dec]
        want += [(H._dev_name(n, True).replace('/target', '/ema', 1), a) for n, a in dec]
        assert [n for n, _ in want] == [str(n) for n in fx['model_names']]
        assert [list(_chainer_shape(a)) for _, a in want] == json.loads(str(fx['model_shapes_json']))
        assert ['/decoder/ema' + str(n) for n in fx['names']] == [n for n, _ in want[-len(dec):]]


def test_oracle_softmax_step_matches_reference():
    """vae_forward, vae_backward and train_step's gradient bookkeeping against VAE.__call__ +
    VQVAE_StandardUpdater.update_core: losses, z, indices (bit exact), e, condition, y, every gradient, and the
    set of parameters whose gradient stays None (the last block's res conv)."""
    check_step('ref_model_softmax.npz')


def test_oracle_mol_step_matches_reference():
    """The same for the mixture-of-logistics model (n_loop 1, n_layer 4).  The float32 oracle misses 1e-4 against
    float64 here: measured 3.99e-4 of the tensor's scale at its worst gradient (MOL_ORACLE_ERR above lists the
    rest), bar 2 x 3.99e-4 = 7.98e-4 for the gradients.  Losses, z, e, condition and y keep 1e-4."""
    fx = R.load('ref_model_mol.npz')
    errs = R.grad_errors(fx, oracle_step(fx)[2])
    worst = max(errs, key=errs.get)
    print('float32 oracle vs float64 reference, MoL gradients: worst %.3e at %s' % (errs[worst], worst))
    check_step('ref_model_mol.npz', grad_tol=MOL_GRAD_BAR)


@pytest.mark.parametrize('name', ['ref_model_softmax.npz', 'ref_model_mol.npz'])
def test_float64_oracle_step_matches_reference(name):
    """The oracle is dtype-generic: run in float64 it must reproduce the reference's float64 step to the precision
    the fixture is stored in -- losses and activations (kept float64) to 1e-10, gradients to 2^-23 of their scale
    (F64_GRAD_BAR).  No float32 noise is left to hide a misread term behind."""
    check_step(name, grad_tol=F64_GRAD_BAR, float64=True)


def test_oracle_mol_loss_matches_reference():
    """mol_loss_fwd / mol_loss_bwd against WaveNet.calculate_logistic_loss and its autograd gradient on the
    crafted input: targets at -1 and +1 and on both sides of +-0.999, clamped log-scales, a saturated term."""
    fx = R.load('ref_mol_loss.npz')
    y, t = R.crafted_mol_inputs(fx['meta']['seed'])
    np.testing.assert_array_equal(y, fx['y'])
    np.testing.assert_array_equal(t, fx['t'])
    tt = 127.5 * t.astype(np.float64)
    assert (tt < 127.5 * -0.999).sum() >= 5 and (tt > 127.5 * 0.999).sum() >= 5          # both edge branches ...
    assert ((np.abs(t) > 0.998) & (np.abs(t) < 0.999)).sum() >= 4                         # ... and their near side
    assert (y[:, 20:] < -40).sum() == 2 and (fx['gy'][:, 20:][y[:, 20:] < -40] == 0).all()
    assert_close(O.mol_loss_fwd(y, t), float(fx['loss']), 1e-4, 'mol loss')
    assert_close_scaled(O.mol_loss_bwd(y, t), fx['gy'], 1e-4, 'mol d loss / d y')
    y64, t64 = y.astype(np.float64), t.astype(np.float64)
    assert_close(O.mol_loss_fwd(y64, t64), float(fx['loss']), 1e-9, 'mol loss (float64 oracle)')
    assert_close_scaled(O.mol_loss_bwd(y64, t64), fx['gy'], 1e-9, 'mol d loss / d y (float64 oracle)')


def test_oracle_ema_matches_reference():
    """ema_update against ExponentialMovingAverage.__call__: two training-mode calls with the target moved in
    between, decay 0.9999 and 0.9; then the evaluation-mode loss1, which runs on the EMA copy."""
    check_ema()


def test_oracle_generation_matches_reference():
    """wavenet_initialize / wavenet_generate_step against WaveNet.initialize / generate: 48 (24) teacher-forced
    steps, more than the receptive field, every queue wraps; each sequence has its own condition column."""
    check_generate()


def _swap_gate_halves(monkeypatch):
    orig = O.resblock_fwd

    def swapped(p, x, cond, dil):
        q = dict(p)
        for key in ('conv', 'condition_proj'):
            W, b = p[key]
            Ch = W.shape[0] // 2
            q[key] = (np.roll(W, Ch, axis=0), np.roll(b, Ch))
        return orig(q, x, cond, dil)
    monkeypatch.setattr(O, 'resblock_fwd', swapped)


def _crop_other_end(monkeypatch):
    def causal_conv_fwd(x, W, b, dil):
        K = W.shape[2]
        return O.conv1d_fwd(x, W, b, stride=1, pad=dil * (K - 1), dil=dil)[:, :, -x.shape[2]:]
    monkeypatch.setattr(O, 'causal_conv_fwd', causal_conv_fwd)


def _beta_on_loss2(monkeypatch, losses=True, codebook=True):
    """loss2 = beta * mean(...), loss3 = mean(...).  The three places it shows: the two loss values trade places
    (loss3 = beta * loss2 at identical z, e); W's gradient, which is loss2's alone, shrinks by beta; the encoder's
    commitment gradient, which is loss3's, loses its beta -- vae_backward's own ``beta`` factor, patched to 1.
    ``losses`` / ``codebook`` = False leave those two as the reference has them: the encoder gradients alone must
    give the misreading away."""
    fwd, bwd = O.vae_forward, O.vae_backward

    def vae_forward(*a, **k):
        (l1, l2, l3), cache = fwd(*a, **k)
        return ((l1, l3, l2) if losses else (l1, l2, l3)), cache

    def vae_backward(P, cache, speaker, t, n_loop, n_layer, beta=0.25, *a, **k):
        G = bwd(P, cache, speaker, t, n_loop, n_layer, 1.0, *a, **k)
        if codebook:
            G['vq'] = G['vq'] * G['vq'].dtype.type(beta)       # (vae_backward's W gradient carries no beta of its own)
        return G
    monkeypatch.setattr(O, 'vae_forward', vae_forward)
    monkeypatch.setattr(O, 'vae_backward', vae_backward)


def _e_not_detached(monkeypatch, codebook=True):
    """loss3 = beta * mean((z - e) ** 2) with e still attached.  e's gradient is minus z's; the straight-through
    hands it back to z, so loss3 sends NOTHING into the encoder (vae_backward's ``beta`` factor, patched to 0), and W
    receives beta x loss2's gradient on top of it.  The loss values do not move.  ``codebook`` = False leaves W's
    gradient as the reference has it: the encoder gradients alone must give the misreading away."""
    bwd = O.vae_backward

    def vae_backward(P, cache, speaker, t, n_loop, n_layer, beta=0.25, *a, **k):
        G = bwd(P, cache, speaker, t, n_loop, n_layer, 0.0, *a, **k)
        if codebook:
            G['vq'] = G['vq'] * G['vq'].dtype.type(1 + beta)
        return G
    monkeypatch.setattr(O, 'vae_backward', vae_backward)


def _beta_on_loss2_seen_by_the_encoder_alone(monkeypatch):
    _beta_on_loss2(monkeypatch, losses=False, codebook=False)


def _e_not_detached_seen_by_the_encoder_alone(monkeypatch):
    _e_not_detached(monkeypatch, codebook=False)


def _decay_roles_swapped(monkeypatch):
    def ema_update(ema, target, decay):
        ema[...] = ema.dtype.type(1 - decay) * target + ema.dtype.type(decay) * ema
    monkeypatch.setattr(O, 'ema_update', ema_update)


def _global_condition_first(monkeypatch):
    orig = O.cond_embed_fwd

    def cond_embed_fwd(p, e, speaker, upscale=64):
        cond, hs = orig(p, e, speaker, upscale)
        Cl = hs[-1].shape[1]
        return np.concatenate((cond[:, Cl:], cond[:, :Cl]), axis=1), hs
    monkeypatch.setattr(O, 'cond_embed_fwd', cond_embed_fwd)


MISREADINGS = [_swap_gate_halves, _crop_other_end, _beta_on_loss2, _e_not_detached, _decay_roles_swapped,
               _global_condition_first, _beta_on_loss2_seen_by_the_encoder_alone,
               _e_not_detached_seen_by_the_encoder_alone]


@pytest.mark.parametrize('misread', MISREADINGS, ids=[f.__name__.strip('_') for f in MISREADINGS])
def test_a_misread_oracle_is_caught(monkeypatch, misread):
    """The comparisons can fail: each of six deliberate misreadings of the reference, patched into the oracle,
    makes them raise.  The two about loss2 / loss3 are patched in once more with the loss values and W's gradient
    left right, so that only the encoder's gradients differ: those pin the terms as well."""
    check_everything()                             # sound before the patch
    misread(monkeypatch)
    with pytest.raises(AssertionError):
        check_everything()


def test_reference_defaults():
    """ref_params.json (the names params.py defines, as executed) against what this project calls "the reference's
    default model": tools/default_model_bench.py's CFG, the loss defaults of the oracle and the package's own
    defaults (MoL loss, sampling, synthesis, the EMA link)."""
    with open(os.path.join(R.GOLD, 'ref_params.json')) as f:
        ref = json.load(f)
    spec = importlib.util.spec_from_file_location(
        'default_model_bench', os.path.join(os.path.dirname(R.GOLD), os.pardir, 'tools', 'default_model_bench.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    renamed = dict(residual='residual_channels', dilated='dilated_channels', skip='skip_channels',
                   local_dim='local_condition_dim', global_dim='global_condition_dim', batch_per_gpu='batchsize')
    for key, value in tool.CFG.items():
        if key == 'n_speaker':
            continue                               # a property of the corpus (VCTK), not of params.py
        assert ref[renamed.get(key, key)] == value, key
    import inspect
    for fn in (O.mol_loss_fwd, O.mol_loss_bwd):
        sig = inspect.signature(fn).parameters
        assert sig['quantize'].default == ref['quantize'] and sig['log_scale_min'].default == ref['log_scale_min']
    # the package's own defaults (importing these modules opens no device)
    from vqvae_amd import functions as F, generation, synthesis
    from vqvae_amd.utils import ExponentialMovingAverage
    sig = inspect.signature(F.mixture_of_logistics_nll).parameters
    assert sig['quantize'].default == ref['quantize'] and sig['log_scale_min'].default == ref['log_scale_min']
    assert inspect.signature(generation.sample_logits).parameters['log_scale_min'].default == ref['log_scale_min']
    for fn in (synthesis.synthesize, synthesis.synthesize_many):
        sig = inspect.signature(fn).parameters
        assert sig['quantize'].default == ref['quantize'] and sig['use_logistic'].default == ref['use_logistic'], fn
    # utils.py:133's own default, which train.py overrides with params.ema_mu
    assert inspect.signature(ExponentialMovingAverage.__init__).parameters['decay'].default == 0.999 != ref['ema_mu']
    assert ref['n_mixture'] == 30 == H.MOL['out_dim'] and ref['dropout_zero_rate'] == 0
    assert inspect.signature(O.vae_forward).parameters['beta'].default == ref['beta']
    assert inspect.signature(O.train_step).parameters['alpha'].default == ref['lr']
    assert inspect.signature(O.train_step).parameters['ema_decay'].default == ref['ema_mu']
