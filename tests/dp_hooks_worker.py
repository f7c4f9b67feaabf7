"""Worker for test_gpu_optim_hooks.py::test_two_process_parallel_updater_with_hooks: tests/dp_gpu_worker.py's two modes
with the optimizer hooks attached.

  rank <r> <n> <dir> <threshold>          one of n processes sharing GPU 0 (host-staged exchange, dp_gpu_worker.py);
  single <n> <dir> <threshold> <tag>      ONE process that sums the n strided shard gradients in rank order and steps.

Both attach GradientClipping(threshold) (none for 'inf'), NonFiniteGuard and GradientNorms, and save the parameters, the
clip rate and the gradient norm of every step."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import dp_gpu_worker as W  # noqa: E402  (puts the package and the oracle on sys.path)


def _hooked(n, threshold):
    import vqvae_amd as V
    model, opt = W._build(n)
    if np.isfinite(threshold):
        opt.add_hook(V.GradientClipping(threshold))
    opt.add_hook(V.NonFiniteGuard())
    opt.add_hook(V.GradientNorms())
    return model, opt


def _record(opt, rates, norms):
    st = opt.hook_state()
    rates.append(st['rate'])
    norms.append(st['norm'])


def run_rank(rank, n, directory, threshold):
    import vqvae_amd as V
    model, opt = _hooked(n, threshold)
    comm = W.HostStagedCommunicator(rank, n, directory)
    comm.always_reduce = True
    upd = V.VQVAE_ParallelUpdater(W._Iter(W._examples()), opt, comm=comm, device=0, overlap_comm=False)
    rates, norms = [], []
    for _ in range(W.STEPS):
        upd.update()
        _record(opt, rates, norms)
    assert comm.calls == W.STEPS and opt.skipped_steps() == 0
    np.save(os.path.join(directory, 'params_rank%d.npy' % rank), opt.params.get())
    np.save(os.path.join(directory, 'rates_rank%d.npy' % rank), np.array(rates, np.float64))
    np.save(os.path.join(directory, 'losses_rank%d.npy' % rank),
            np.array([float(l.data.get()) for l in upd.last_losses]))


def run_single(n, directory, threshold, tag):
    from vqvae_amd import core
    from vqvae_amd.updaters import concat_examples, three_loss_backward
    model, opt = _hooked(n, threshold)
    ex = W._examples()
    n_shadow = opt.params.size - opt.n_train
    rates, norms = [], []
    for _ in range(W.STEPS):
        total = None
        for r in range(n):
            shadow = opt.params.flat_view(opt.n_train, n_shadow)
            keep = shadow.get() if r > 0 else None
            with core.force_backprop_mode():
                losses = model(*concat_examples(ex[r::n], 0))
            three_loss_backward(model, losses)
            g = opt.grads.get()
            total = g if total is None else total + g
            if keep is not None:
                shadow.set(keep)
        opt.grads.set(total)
        opt.update()
        _record(opt, rates, norms)
    np.save(os.path.join(directory, 'params_%s.npy' % tag), opt.params.get())
    np.save(os.path.join(directory, 'rates_%s.npy' % tag), np.array(rates, np.float64))
    np.save(os.path.join(directory, 'norms_%s.npy' % tag), np.array(norms, np.float64))


if __name__ == '__main__':
    if sys.argv[1] == 'rank':
        run_rank(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], float(sys.argv[5]))
    else:
        run_single(int(sys.argv[2]), sys.argv[3], float(sys.argv[4]), sys.argv[5])
