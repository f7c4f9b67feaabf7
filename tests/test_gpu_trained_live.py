"""Parity at a trained state with a LIVE codebook.

tests/test_gpu_trained.py trains the configs[0] model for 300 device steps and finds the quantiser collapsed onto one
code: its VQ parity (indices, loss2, loss3, gW) is parity on a constant.  Here the same run (same seeds, minibatches,
step size and step count, imported from that file) carries a CodebookMonitor and re-seeds unused codes every
RESEED_EVERY steps; the run without re-seeding is repeated beside it so that both distinct-code counts are printed.  The
trained state must use well over one code, and ONE step from that snapshot is then held against the oracle by the
existing test body (imported, not edited): argmin indices bit-exact, three losses 1e-4, every gradient (gW among them)
1e-4 of its scale, parameters after Adam 1e-4, EMA 1e-5.  Re-seeding happens between steps and the compared step starts
from a snapshot, so the oracle needs nothing new."""
import copy

import numpy as np
import pytest

import helpers as H
import vqvae_oracle as O
import test_gpu_trained as TT
from test_gpu_configs import CFG0
from test_gpu_model import _Iter

pytestmark = pytest.mark.gpu

RESEED_EVERY = 50
THRESHOLD = 0.05            # of the running usage (decay 0.9): not chosen once in the last ~30 steps
# measured on an MI355X at the trained state, minibatch seed 301 (120 latents, 512 codes): 1 distinct code without
# re-seeding, MEASURED_LIVE with it; the bar keeps a margin under the measurement
MEASURED_LIVE = 6
LIVE_BAR = 3


def _train(gpu, reseed):
    """The training run of test_gpu_trained.trained; returns (P, P_ema, (first, last), distinct codes at the trained state,
    codes replaced per re-seed, the monitor's last summary)."""
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
    first = last = None
    replaced, summary = [], None
    try:
        for step in range(TT.TRAIN_STEPS):
            upd.update()
            if step in (0, TT.TRAIN_STEPS - 1):
                l = [float(v.data.get()) for v in upd.last_losses]
                first, last = (l, last) if step == 0 else (first, l)
            it = step + 1
            if it % RESEED_EVERY == 0 and it < TT.TRAIN_STEPS:
                summary = mon.summary(reset=True, threshold=THRESHOLD)
                if reseed:
                    replaced.append(mon.reseed(opt, threshold=THRESHOLD))
        summary = mon.summary(threshold=THRESHOLD)
    finally:
        model.vq.monitor = None
    assert mon.steps_seen() == TT.TRAIN_STEPS
    # the quantiser's assignment of one training minibatch (the one the compared step uses) at the trained state
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
    return P, P_ema, (first, last), distinct, replaced, summary


@pytest.fixture(scope='module')
def trained_live(gpu):
    gpu.set_matmul_dtype('float32')
    try:
        plain = _train(gpu, reseed=False)
        live = _train(gpu, reseed=True)
    finally:
        gpu.set_matmul_dtype(gpu.default_matmul_dtype())
    print('trained state, %d steps: %d distinct codes among %d latents WITHOUT re-seeding (monitor: %s); '
          '%d WITH a re-seed every %d steps (codes replaced per re-seed: %s; monitor: %s); loss1 %.3f -> %.3f / %.3f'
          % (TT.TRAIN_STEPS, plain[3], TT.T // 64, plain[5], live[3], RESEED_EVERY, live[4], live[5],
             live[2][0][0], plain[2][1][0], live[2][1][0]))
    return plain, live


def test_reseeding_keeps_the_codebook_alive(trained_live):
    plain, live = trained_live
    first, last = live[2]
    assert np.isfinite(last).all() and last[0] < first[0] - 0.5, (first, last)        # it still trains
    assert live[3] >= LIVE_BAR > 1, 'only %d distinct codes at the trained state (measured: %d)' % (live[3], MEASURED_LIVE)
    assert live[3] > plain[3]
    assert all(n > 0 for n in live[4])
    assert live[5]['main/codes_used'] > plain[5]['main/codes_used']
    assert live[5]['main/perplexity'] > plain[5]['main/perplexity'] >= 1.0


def test_one_step_from_the_live_snapshot_matches_oracle(gpu, matmul_mode, trained_live, capsys):
    """The whole-step parity of tests/test_gpu_trained.py, from the state with a live codebook."""
    P, P_ema, losses = trained_live[1][:3]
    TT.test_one_step_from_a_trained_snapshot_matches_oracle(gpu, matmul_mode, (P, P_ema, losses))
    out = capsys.readouterr().out
    print(out)
    line = [l for l in out.splitlines() if 'distinct codes among' in l][-1]
    assert int(line.split(':')[1].split('distinct')[0]) >= LIVE_BAR            # the oracle's own count of the compared step
