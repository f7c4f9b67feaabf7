"""Does k-means initialisation keep the codebook alive on the 300-step run?

The run of tests/test_gpu_trained_live.py (same model, seeds, minibatches, step size and step count, imported from there and
from tests/test_gpu_trained.py) four ways: plain; with the codebook initialised by k-means after WARMUP steps; that plus the
monitor's re-seeding schedule; that plus the EMA rule.  The pool is the encoder's output on 16 synthetic minibatches (1 920
rows for 512 codes) at the moment of the call.  The distinct-code counts of all four are printed, the measured ones are kept
below as MEASURED_*, and only what was measured is asserted.  ONE step from the state with the most codes in use is then
held against the oracle by the existing test body in the three fp32 matmul modes."""
import copy

import numpy as np
import pytest

import helpers as H
import vqvae_oracle as O
import test_gpu_trained as TT
import test_gpu_trained_live as TL
from test_gpu_configs import CFG0
from test_gpu_model import _Iter

pytestmark = pytest.mark.gpu

WARMUP = 20                 # steps before the initialisation: a random encoder's outputs are a poor sample
POOL_BATCHES = 16
ITERS = 10
# measured on an MI355X, one run: distinct codes among the 120 latents of minibatch seed 301 at the trained state
# (re-seeding alone: 6, the EMA rule alone: 2 -- tests/test_gpu_trained_live.py, tests/test_gpu_vq_ema.py)
MEASURED = {'plain': 1, 'kmeans': 2, 'kmeans+reseed': 12, 'kmeans+ema': 6}
BAR = {'plain': 1, 'kmeans': 1, 'kmeans+reseed': 6, 'kmeans+ema': 3}          # a margin under the measurement


def _train(gpu, kmeans, reseed=False, ema=False):
    import vqvae_amd as V
    from vqvae_amd import core
    from vqvae_amd.optimizers import Adam
    cfg = dict(CFG0)
    P, model = H.build_model(cfg, seed=5, ema_decay=0.9999)
    model.to_gpu()
    opt = Adam(TT.TRAIN_LR)
    opt.setup(model)
    batches = [O.synth_batch(1, length=TT.T, n_speaker=cfg['n_speaker'], seed=300 + s) for s in range(4)]
    upd = V.VQVAE_StandardUpdater(_Iter(batches), opt, device=0)
    mon = V.CodebookMonitor(model.vq, decay=0.9, seed=0)
    model.vq.monitor = mon
    if ema:
        model.vq.codebook_ema = V.EMACodebook(model.vq, decay=0.99)
    first = last = report = None
    replaced = []
    try:
        for step in range(TT.TRAIN_STEPS):
            upd.update()
            if step in (0, TT.TRAIN_STEPS - 1):
                l = [float(v.data.get()) for v in upd.last_losses]
                first, last = (l, last) if step == 0 else (first, l)
            it = step + 1
            if kmeans and it == WARMUP:
                pool = [O.synth_batch(1, length=TT.T, n_speaker=cfg['n_speaker'], seed=400 + s) for s in range(POOL_BATCHES)]
                report = V.kmeans_init(model, _Iter(pool), rows=POOL_BATCHES * (TT.T // 64), iters=ITERS, seed=0, optimizer=opt)
            if reseed and it % TL.RESEED_EVERY == 0 and it < TT.TRAIN_STEPS:
                replaced.append(mon.reseed(opt, threshold=TL.THRESHOLD))
    finally:
        model.vq.monitor = None
        model.vq.codebook_ema = None
    arrays = V.concat_examples(_Iter([batches[1]]).next(), 0)
    with core.using_config('train', False), core.no_backprop_mode():
        model(*arrays)
    distinct = int(np.unique(model.vq._cache[3][0].get()).size)
    named = dict(model.namedparams())
    for name, arr in O.flatten_params(P):
        arr[...] = named[H._dev_name(name, True)].data.get().reshape(arr.shape)
    P_ema = copy.deepcopy(P['decoder'])
    for name, arr in O.flatten_params(P_ema):
        arr[...] = named['/decoder/ema' + name.replace('/blocks/', '/resnet/')].data.get().reshape(arr.shape)
    return dict(P=P, P_ema=P_ema, losses=(first, last), distinct=distinct, replaced=replaced, report=report)


@pytest.fixture(scope='module')
def four_runs(gpu):
    gpu.set_matmul_dtype('float32')
    try:
        runs = {'plain': _train(gpu, False), 'kmeans': _train(gpu, True), 'kmeans+reseed': _train(gpu, True, reseed=True),
                'kmeans+ema': _train(gpu, True, ema=True)}
    finally:
        gpu.set_matmul_dtype(gpu.default_matmul_dtype())
    for name, r in runs.items():
        rep = r['report']
        print('trained state, %d steps, %s: %d distinct codes among %d latents; loss1 %.3f -> %.3f, loss2 %.2e; codes replaced '
              'per re-seed %s; k-means at step %d: %s'
              % (TT.TRAIN_STEPS, name, r['distinct'], TT.T // 64, r['losses'][0][0], r['losses'][1][0], r['losses'][1][1],
                 r['replaced'], WARMUP,
                 None if rep is None else 'inertia %.4g -> %.4g, %d of %d codes with pool rows, empty per iteration %s'
                 % (rep['inertia'][0], rep['inertia'][-1], int((rep['counts'] > 0).sum()), rep['counts'].size, rep['empty'])))
    return runs


def test_the_four_runs_train_and_the_counts_are_what_was_measured(four_runs):
    for name, r in four_runs.items():
        first, last = r['losses']
        assert np.isfinite(last).all() and last[0] < first[0] - 0.5, (name, first, last)      # it still trains
        assert r['distinct'] >= BAR[name], '%s: %d distinct codes (measured: %s)' % (name, r['distinct'], MEASURED[name])
        rep = r['report']
        if rep is not None:
            assert len(rep['inertia']) == ITERS + 1 and rep['counts'].sum() == POOL_BATCHES * (TT.T // 64)
            assert rep['inertia'][-1] <= rep['inertia'][0]


def test_one_step_from_the_state_with_most_codes_matches_oracle(gpu, matmul_mode, four_runs, capsys):
    """The whole-step parity of tests/test_gpu_trained.py from the best of the three initialised states."""
    best = max(('kmeans', 'kmeans+reseed', 'kmeans+ema'), key=lambda n: four_runs[n]['distinct'])
    r = four_runs[best]
    TT.test_one_step_from_a_trained_snapshot_matches_oracle(gpu, matmul_mode, (r['P'], r['P_ema'], r['losses']))
    out = capsys.readouterr().out
    print('from the %s state:\n%s' % (best, out))
