#!/usr/bin/env python
"""Generates the tests/golden/ref_*.npz / ref_params.json fixtures by EXECUTING the reference's own model code.

Dev-container tooling only, like make_golden.py (whose outputs this script does not touch): it needs the
read-only reference checkout and torch.  ``chainer_standin.install()`` puts a stand-in ``chainer`` on
torch-CPU float64 autograd into sys.modules; the reference's ``net.py``,
``WaveNet/modules.py``, ``updaters.py`` and ``utils.py`` are then imported from the checkout through
sys.path and run unmodified -- nothing of them is copied.  What ends up in the fixtures:

  * VAE.__call__ + VQVAE_StandardUpdater.update_core      (net.py:79-96, updaters.py:6-19)
  * ExponentialMovingAverage.__call__                     (utils.py:140-158)
  * WaveNet.calculate_logistic_loss                       (modules.py:169-230)
  * WaveNet.initialize / generate                         (modules.py:58-74, 98-110, 232-255)
  * the names params.py defines

Parameters are ``O.make_params`` of a recorded seed and configuration (+ a tweak recorded by name, see
helpers.named_tweak), inputs ``O.synth_batch[_raw]`` of a recorded seed: the fixtures hold seeds and results,
not weights.  Gradient tensors are stored rounded to float32 (6e-8, far below every bar); their float64 sum
and sum of squares, the losses and the activations stay float64.

Run:  python tests/golden/make_golden_model.py
"""
import copy
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = '/root/reference'
for p in (HERE, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'oracle')):
    sys.path.insert(0, p)

import chainer_standin as S          # noqa: E402
import helpers as H                  # noqa: E402
import ref_model as R                # noqa: E402
import vqvae_oracle as O             # noqa: E402


def import_reference():
    ch = S.install()
    sys.modules.setdefault('librosa', types.ModuleType('librosa'))     # utils.py imports it at the top
    sys.path.insert(0, REF)
    import net
    import updaters
    import utils
    from WaveNet import modules
    return ch, net, modules, updaters, utils


def build_reference(ref, cfg, P, use_logistic, ema_decay=None):
    """train.py:76-98 with the fixture's configuration, then every parameter loaded BY NAME."""
    ch, net, modules, updaters, utils = ref
    encoder = net.Encoder(cfg['d'])
    wavenet = modules.WaveNet(cfg['n_loop'], cfg['n_layer'], cfg['filter_size'], cfg['input_dim'], cfg['residual'],
                              cfg['dilated'], cfg['skip'], 256, use_logistic, cfg['out_dim'], -40,
                              cfg['local_dim'] + cfg['global_dim'], 0)
    condition_embed = net.ConditionEmbed(cfg['n_speaker'], cfg['global_dim'], cfg['local_dim'])
    decoder = wavenet if ema_decay is None else utils.ExponentialMovingAverage(wavenet, ema_decay)
    loss_fun = wavenet.calculate_logistic_loss if use_logistic else ch.functions.softmax_cross_entropy
    model = net.VAE(encoder, decoder, condition_embed, cfg['d'], cfg['k'], 0.25, loss_fun)
    named = dict(model.namedparams())
    seen = set()
    for name, arr in O.flatten_params(P):
        a4 = arr.reshape(arr.shape + (1,)) if arr.ndim == 3 else arr
        dn = H._dev_name(name, ema_decay is not None)
        for n in ([dn, dn.replace('/target', '/ema', 1)] if '/target' in dn else [dn]):
            named[n].array = a4
            seen.add(n)
    assert seen == set(named), sorted(set(named) ^ seen)
    return model, wavenet


def make_P(meta):
    P = O.make_params(np.random.RandomState(meta['param_seed']), **meta['cfg'])
    H.named_tweak(meta['tweak'])(P)
    return P


def examples(batch):
    x_enc, x_dec, spk, t = batch
    return [(x_enc[j][..., None], x_dec[j][..., None], spk[j], t[j][..., None]) for j in range(x_enc.shape[0])]


def forward_parts(ref, model, wavenet, batch):
    """z, idx, e, condition, y of VAE.__call__, by calling the model's own links in its order (net.py:81-86)."""
    ch, net, modules, updaters, utils = ref
    x_enc, x_dec, spk, t = S.concat_examples(examples(batch))
    z = model.encoder(x_enc)
    node = utils.StraightThrough()
    e, = node.apply((z, model.vq.W))
    cond = model.condition_embed(e, spk)
    y = wavenet(x_dec, cond)
    return z.data, node.indexes.copy(), e.data, cond.data, y.data


def vq_margins(z, W):
    """Per latent row: (second-best - best) / best squared distance, float64."""
    rows = np.moveaxis(z.reshape(z.shape[:3]), 1, 2).reshape(-1, z.shape[1])
    d2 = ((rows[:, None, :] - W[None, :, :]) ** 2).sum(axis=2)
    s = np.sort(d2, axis=1)
    return (s[:, 1] - s[:, 0]) / s[:, 0]


def model_step(ref, meta):
    ch, net, modules, updaters, utils = ref
    cfg, logistic = meta['cfg'], meta['use_logistic']
    synth = O.synth_batch_raw if logistic else O.synth_batch
    P = make_P(meta)
    for seed in range(meta['batch_seed'], meta['batch_seed'] + 64):       # until the VQ margin condition holds
        batch = synth(meta['B'], length=meta['length'], n_speaker=cfg['n_speaker'], seed=seed)
        S.set_dtype(np.float64)
        model, wavenet = build_reference(ref, cfg, P, logistic)
        z, idx, e, cond, y = forward_parts(ref, model, wavenet, batch)
        S.set_dtype(np.float32)
        m32, w32 = build_reference(ref, cfg, P, logistic)
        idx32 = forward_parts(ref, m32, w32, batch)[1]
        S.set_dtype(np.float64)
        margins = vq_margins(z, P['vq'].astype(np.float64))
        if (idx32 == idx).all() and margins.min() > R.MARGIN:
            break
    else:
        raise SystemExit('no batch seed satisfies the VQ margin condition')
    meta = dict(meta, batch_seed=seed)
    opt = S.SnapshotOptimizer().setup(model)
    upd = updaters.VQVAE_StandardUpdater(S.ListIterator(examples(batch)), opt)
    upd.update()
    rep = ch.reporter.state.last
    losses = np.array([float(rep['loss%d' % i].data) for i in (1, 2, 3)])
    out = dict(meta_json=json.dumps(meta, sort_keys=True), losses=losses, z=z, idx=idx, e=e, margins=margins)
    out['names'] = np.array([n for n, _ in opt.grads])
    out['shapes_json'] = json.dumps([list(p.shape) for _, p in model.namedparams()])
    out['cond_val'] = cond.reshape(-1)[R.positions(meta['sample_seed'], 1000, cond.size, R.N_COND)]
    out['y_val'] = y.reshape(-1)[R.positions(meta['sample_seed'], 1001, y.size, R.N_Y)]
    n = len(opt.grads)
    out['grad_none'] = np.array([g is None for _, g in opt.grads])
    out['grad_sum'], out['grad_sumsq'], out['grad_absmax'] = np.zeros(n), np.zeros(n), np.zeros(n)
    for i, (name, g) in enumerate(opt.grads):
        if g is None:
            continue
        out['grad_sum'][i], out['grad_sumsq'][i], out['grad_absmax'][i] = g.sum(), (g * g).sum(), np.abs(g).max()
        flat = g.reshape(-1)
        if flat.size > R.WHOLE_MAX:
            flat = flat[R.positions(meta['sample_seed'], i, flat.size, R.N_GRAD)]
        out['g%03d' % i] = flat.astype(np.float32)
    return out


def model_ema(ref, meta):
    ch, net, modules, updaters, utils = ref
    cfg = meta['cfg']
    P = make_P(meta)
    batch = O.synth_batch(meta['B'], length=meta['length'], n_speaker=cfg['n_speaker'], seed=meta['batch_seed'])
    args = S.concat_examples(examples(batch))
    out = dict(meta_json=json.dumps(meta, sort_keys=True))
    for decay in meta['decays']:
        model, wavenet = build_reference(ref, cfg, P, False, ema_decay=decay)
        names = [n for n, _ in model.decoder.ema.namedparams()]
        out['model_names'] = np.array([n for n, _ in model.namedparams()])
        out['model_shapes_json'] = json.dumps([list(p.shape) for _, p in model.namedparams()])
        for call in (1, 2):
            model(*args)                                                 # config.train is True: the blend runs
            for i, (n, p) in enumerate(model.decoder.ema.namedparams()):
                flat = p.array.reshape(-1)
                if flat.size > R.N_EMA:
                    flat = flat[R.positions(meta['sample_seed'], i, flat.size, R.N_EMA)]
                out['ema_%s_call%d_%03d' % (R.decay_tag(decay), call, i)] = flat.astype(np.float32)
            if call == 1:                                                # the target moves, as an optimizer would move it
                rs = np.random.RandomState(meta['perturb_seed'])
                for n, p in model.decoder.target.namedparams():
                    p.array = p.array + meta['perturb_scale'] * rs.standard_normal(p.shape)
        with ch.using_config('train', False):
            l1, l2, l3 = model(*args)
        out['eval_loss1_%s' % R.decay_tag(decay)] = np.float64(l1.data)
    out['names'] = np.array(names)
    return out


def mol_loss(ref, meta):
    ch, net, modules, updaters, utils = ref
    y, t = R.crafted_mol_inputs(meta['seed'])
    wn = modules.WaveNet(1, 1, 2, 1, 4, 4, 4, 256, True, 30, -40, 4, 0)
    vy = ch.Variable(y[..., None])
    loss = wn.calculate_logistic_loss(vy, t[..., None].astype(np.float64))
    loss.backward()
    return dict(meta_json=json.dumps(meta, sort_keys=True), y=y, t=t, loss=np.float64(loss.data),
                gy=vy.grad[..., 0].copy())


def generation(ref, meta, out, tag):
    ch, net, modules, updaters, utils = ref
    cfg, logistic, steps, n = meta['cfg'], meta['use_logistic'], meta['steps'], meta['n']
    P = make_P(meta)
    model, wavenet = build_reference(ref, cfg, P, logistic)
    trainer = copy.deepcopy(wavenet)                       # initialize() strips the paddings of the copy it runs on
    rs = np.random.RandomState(meta['input_seed'])
    T = steps + 1                                          # the device loop runs T - 1 steps (generate.py:103-105)
    cond = rs.standard_normal((n, cfg['local_dim'] + cfg['global_dim'], T)).astype(np.float32)
    if logistic:
        forced = rs.uniform(-1, 1, (T, n)).astype(np.float32)
        x_seq = np.zeros((n, 1, steps))
        x_seq[:, 0, 1:] = forced[:steps - 1].T
    else:
        forced = rs.randint(0, cfg['input_dim'], (T, n)).astype(np.int32)
        forced[7, 1] = -1                                  # an all-zero input vector in mid-sequence
        x_seq = np.zeros((n, cfg['input_dim'], steps))
        for i in range(1, steps):
            for b in range(n):
                if forced[i - 1, b] >= 0:
                    x_seq[b, forced[i - 1, b], i] = 1
    wavenet.initialize(n)
    logits = np.zeros((steps, n, cfg['out_dim']))
    for i in range(steps):
        yv = wavenet.generate(ch.Variable(x_seq[:, :, i:i + 1, None]),
                              ch.Variable(cond[:, :, i:i + 1, None].astype(np.float64)))
        logits[i] = yv.data[:, :, 0, 0]
    want = trainer(ch.Variable(x_seq[..., None]), ch.Variable(cond[:, :, :steps, None].astype(np.float64))).data
    err = np.abs(logits - want[:, :, :, 0].transpose(2, 0, 1)).max()
    assert err <= 1e-10, 'generation and the training forward of the reference disagree: %.3e' % err
    out[tag + '_meta_json'] = json.dumps(meta, sort_keys=True)
    out[tag + '_cond'], out[tag + '_forced'] = cond, forced
    out[tag + '_logits'] = logits.astype(np.float32)
    return err


def params_json():
    ns = {}
    with open(os.path.join(REF, 'params.py')) as f:
        exec(compile(f.read(), 'params.py', 'exec'), ns)
    return {k: (list(v) if isinstance(v, tuple) else v) for k, v in ns.items() if not k.startswith('__')}


def save(name, arrays):
    path = os.path.join(HERE, name)
    # a zip member's timestamp would change the bytes from run to run: write through a fixed-date archive
    import zipfile
    import io
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as zf:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[key]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(),
                        compress_type=zipfile.ZIP_DEFLATED)
    print('%-24s %7d bytes' % (name, os.path.getsize(path)))
    assert os.path.getsize(path) <= R.MAX_BYTES, name


def main():
    ref = import_reference()
    common = dict(param_seed=1, batch_seed=71, B=2, length=512, sample_seed=2024)
    save('ref_model_softmax.npz', model_step(ref, dict(common, cfg=dict(H.SMALL), use_logistic=False,
                                                       tweak='biases:101')))
    save('ref_model_mol.npz', model_step(ref, dict(common, param_seed=3, batch_seed=9, cfg=dict(H.MOL_SHALLOW),
                                                   use_logistic=True, tweak='mol_output+biases:103')))
    save('ref_model_ema.npz', model_ema(ref, dict(common, cfg=dict(H.SMALL), tweak='biases:101', decays=[0.9999, 0.9],
                                                  perturb_seed=55, perturb_scale=0.05)))
    save('ref_mol_loss.npz', mol_loss(ref, dict(seed=8)))
    gen = {}
    e1 = generation(ref, dict(cfg=dict(H.SMALL), use_logistic=False, param_seed=22, tweak='biases:23', input_seed=10,
                              steps=48, n=2), gen, 'softmax')
    e2 = generation(ref, dict(cfg=dict(H.MOL_SHALLOW), use_logistic=True, param_seed=25, tweak='biases:26',
                              input_seed=14, steps=24, n=2), gen, 'mol')
    print('generate vs training forward (float64): %.2e softmax, %.2e mol' % (e1, e2))
    save('ref_generate.npz', gen)
    with open(os.path.join(HERE, 'ref_params.json'), 'w') as f:
        json.dump(params_json(), f, indent=1, sort_keys=True)
        f.write('\n')
    print('reference-model fixtures written to', HERE)


if __name__ == '__main__':
    main()
