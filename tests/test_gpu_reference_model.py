"""The device model against the reference's own model code, as executed.

tests/golden/ref_*.npz hold what the reference's net.py, WaveNet/modules.py, updaters.py and utils.py computed in
float64 on a Chainer stand-in (tests/golden/make_golden_model.py).  Everything else in the GPU
suite compares the device with oracle/vqvae_oracle.py, our restatement; here the device is compared with the
fixtures DIRECTLY, so a reading the oracle and the kernels share cannot hide.  NumPy only: no torch, no reference
checkout."""
import numpy as np
import pytest

import helpers as H
import ref_model as R
from helpers import assert_close, assert_close_scaled

pytestmark = pytest.mark.gpu

# The MoL model's gradients: the float32 ORACLE is 3.99e-4 of the tensor's scale from the float64 fixture at its
# worst parameter (measured on the CPU, tests/test_host_reference_model.py MOL_ORACLE_ERR: the cdf_plus - cdf_min
# cancellation in float32), and its bar there is twice that.  The device evaluates the same float32 formula; it gets
# the same factor over the same measured error.
MOL_GRAD_BAR = 2 * 3.99e-4


class _Iter(object):
    def __init__(self, batch):
        self.batch = batch

    def next(self):
        x_enc, x_dec, spk, t = self.batch
        return [(x_enc[j][..., None], x_dec[j][..., None], spk[j], t[j][..., None])
                for j in range(x_enc.shape[0])]     # Preprocess's 4-tuple (utils.py:99-110)


def _batch(meta):
    import vqvae_oracle as O
    synth = O.synth_batch_raw if meta.get('use_logistic') else O.synth_batch
    return synth(meta['B'], length=meta['length'], n_speaker=meta['cfg']['n_speaker'], seed=meta['batch_seed'])


def _model(meta, ema_decay=None):
    _, model = H.build_model(dict(meta['cfg']), seed=meta['param_seed'], ema_decay=ema_decay,
                             use_logistic=bool(meta.get('use_logistic')), tweak=H.named_tweak(meta['tweak']))
    return model


def _device_step(gpu, fx):
    """VQ indices of the fresh model, then one VQVAE_StandardUpdater step -> (losses, idx, gradients by name)."""
    import vqvae_amd as V
    from vqvae_amd.core import Variable
    from vqvae_amd.optimizers import Adam
    from vqvae_amd.utils import StraightThrough
    meta = fx['meta']
    model = _model(meta)
    model.to_gpu()
    batch = _batch(meta)
    with V.core.no_backprop_mode():
        z = model.encoder(Variable(gpu.to_device(np.ascontiguousarray(batch[0][..., None]))))
        st = StraightThrough()
        st.apply((z, model.vq.W))
        idx = st.indexes.get()
    opt = Adam(2e-4)
    opt.setup(model)
    upd = V.VQVAE_StandardUpdater(_Iter(batch), opt, device=0)
    upd.update()
    losses = [float(l.data.get()) for l in upd.last_losses]
    grads = {n: p.grad.get() for n, p in model.namedparams() if p._grad_slot is not None and p.grad is not None}
    return losses, idx, grads


def test_softmax_step_matches_reference(gpu, matmul_mode):
    """One updater step of the softmax model in each fp32-accurate matmul mode against VAE.__call__ +
    VQVAE_StandardUpdater.update_core as executed: losses, VQ indices (bit exact; the fixture's margins make that
    no coin toss), every gradient by name and the set of parameters left without one, at test_train_steps_match_oracle's
    1e-4."""
    fx = R.load('ref_model_softmax.npz')
    losses, idx, grads = _device_step(gpu, fx)
    errs = R.grad_errors(fx, grads)
    worst = max(errs, key=errs.get)
    print('%s: losses %r (reference %r), worst gradient %.3e at %s' % (matmul_mode, losses, list(fx['losses']), errs[worst], worst))
    R.compare_step(fx, losses, idx, grads, 1e-4, 1e-4, what=matmul_mode)


def test_softmax_step_bfloat16_matches_reference(gpu):
    """'bfloat16' at the bars of that mode's whole-step test (test_bf16_operand_mode_training_step, default path):
    loss1 within 2e-2, every gradient's direction (cosine > 0.9 over the stored elements), and the same set of
    parameters without a gradient."""
    fx = R.load('ref_model_softmax.npz')
    gpu.set_matmul_dtype('bfloat16')
    try:
        losses, idx, grads = _device_step(gpu, fx)
    finally:
        gpu.set_matmul_dtype(gpu.default_matmul_dtype())
    names = [str(n) for n in fx['names']]
    print('bfloat16: losses %r (reference %r), %d of %d VQ indices equal' % (
        losses, list(fx['losses']), int((idx.reshape(-1) == fx['idx'].reshape(-1)).sum()), idx.size))
    assert_close(losses[0], float(fx['losses'][0]), 2e-2, 'bf16 vs reference loss1')
    assert sorted(set(names) - set(grads)) == sorted(n for n, m in zip(names, fx['grad_none']) if m)
    for i, n in enumerate(names):
        if fx['grad_none'][i]:
            continue
        got, want = R.sampled(fx, 'g%03d' % i, i, grads[n], R.WHOLE_MAX, R.N_GRAD)
        cos = float((got * want).sum() / (np.linalg.norm(got) * np.linalg.norm(want) + 1e-30))
        assert cos > 0.9, (n, cos)


@pytest.mark.parametrize('mode', ['float32', 'float32x2'])
def test_mol_step_matches_reference(gpu, mode):
    """The mixture-of-logistics model (n_loop 1, n_layer 4): losses and indices as above at 1e-4, gradients at
    MOL_GRAD_BAR = 2 x 3.99e-4, the factor and the measured float32 error of the oracle's own bar."""
    fx = R.load('ref_model_mol.npz')
    gpu.set_matmul_dtype(mode)
    gpu.set_f32x2_min_gflop(0.0)
    try:
        losses, idx, grads = _device_step(gpu, fx)
    finally:
        gpu.set_f32x2_min_gflop(8.0)
        gpu.set_matmul_dtype(gpu.default_matmul_dtype())
    errs = R.grad_errors(fx, grads)
    worst = max(errs, key=errs.get)
    print('mol %s: losses %r (reference %r), worst gradient %.3e at %s' % (mode, losses, list(fx['losses']), errs[worst], worst))
    R.compare_step(fx, losses, idx, grads, 1e-4, MOL_GRAD_BAR, what='mol ' + mode)


@pytest.mark.parametrize('ema', [False, True])
def test_namedparams_match_reference(gpu, ema):
    """model.namedparams(): the reference's names and shapes, with and without the EMA wrapper.  (Compared as a
    mapping: the order in which Chainer lists them is not something the reference's code decides.)"""
    fx = R.load('ref_model_ema.npz' if ema else 'ref_model_softmax.npz')
    import json
    names = [str(n) for n in fx['model_names' if ema else 'names']]
    shapes = json.loads(str(fx['model_shapes_json' if ema else 'shapes_json']))
    got = [(n, list(p.shape)) for n, p in _model(fx['meta'], 0.9 if ema else None).namedparams()]
    assert len(got) == len(names) == len(set(names))
    assert dict(got) == dict(zip(names, shapes))


@pytest.mark.parametrize('decay', [0.9, 0.9999])
def test_ema_matches_reference(gpu, decay):
    """Two training-mode calls with the target moved in between (the fixture's recorded perturbation) reproduce
    ExponentialMovingAverage's parameters at 1e-5; one evaluation-mode call then gives the reference's loss1, which
    ran on the EMA copy."""
    from vqvae_amd.core import using_config
    fx = R.load('ref_model_ema.npz')
    meta = fx['meta']
    model = _model(meta, ema_decay=decay)
    model.to_gpu()
    x_enc, x_dec, spk, t = _batch(meta)
    args = [gpu.to_device(np.ascontiguousarray(a)) for a in (x_enc[..., None], x_dec[..., None], spk, t[..., None])]
    named = dict(model.namedparams())
    names = [str(n) for n in fx['names']]
    for call in (1, 2):
        model(*args)
        for i, n in enumerate(names):
            got, want = R.sampled(fx, 'ema_%s_call%d_%03d' % (R.decay_tag(decay), call, i), i,
                                  named['/decoder/ema' + n].data.get(), R.N_EMA, R.N_EMA)
            assert_close(got, want, 1e-5, 'ema %g call %d %s' % (decay, call, n))
        if call == 1:
            host = [named['/decoder/target' + n].data.get().astype(np.float64) for n in names]
            R.perturb(meta, host)
            for n, a in zip(names, host):
                named['/decoder/target' + n].data.set(a.astype(np.float32))
    with using_config('train', False):
        losses = model(*args)
    assert_close(float(losses[0].data.get()), float(fx['eval_loss1_' + R.decay_tag(decay)]), 1e-4, 'evaluation loss1')


def test_mol_nll_matches_reference(gpu):
    """F.mixture_of_logistics_nll forward and backward against WaveNet.calculate_logistic_loss and its autograd
    gradient on the crafted input (both edge branches and their near side, clamped scales, a saturated term)."""
    from vqvae_amd import functions as F
    from vqvae_amd.core import Variable
    fx = R.load('ref_mol_loss.npz')
    vy = Variable(gpu.to_device(H.to4(fx['y'])))
    loss = F.mixture_of_logistics_nll(vy, gpu.to_device(H.to4(fx['t'])))
    assert_close(loss.data.get(), float(fx['loss']), 1e-4, 'mol loss')
    loss.backward()
    assert_close_scaled(vy.grad.get()[..., 0], fx['gy'], 1e-4, 'mol d loss / d y')


@pytest.mark.parametrize('road', ['per_step', 'persistent', 'lockstep'])
@pytest.mark.parametrize('kind', ['softmax', 'mol'])
def test_generation_matches_reference(gpu, kind, road):
    """Teacher-forced generation against WaveNet.initialize / generate as executed, every step's logits at 1e-4:
    more steps than the receptive field, so every queue wraps; each sequence has its own condition column."""
    fx = R.load('ref_generate.npz')
    meta = fx[kind + '_meta']
    cfg = meta['cfg']
    model = _model(meta)
    model.to_gpu()
    dec = model.decoder
    cond, forced, want = fx[kind + '_cond'], fx[kind + '_forced'], fx[kind + '_logits']
    T, n = forced.shape
    u = np.full((T, n) if kind == 'softmax' else (T, n, cfg['out_dim'] // 3), 0.5)
    if road == 'lockstep':
        _, logits = dec.generate_lockstep(gpu.to_device(cond), u, forced=forced, return_logits=True)
    else:
        _, logits = dec.generate_sequence(gpu.to_device(cond), u, forced=forced, return_logits=True,
                                          persistent=(road == 'persistent'))
        assert (getattr(dec._gen, '_last_ws', None) is not None) == (road == 'persistent')
        logits = logits.get()
    assert logits.shape == want.shape == (meta['steps'], n, cfg['out_dim'])
    assert_close(logits, want, 1e-4, '%s %s logits' % (kind, road))
