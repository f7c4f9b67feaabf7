"""Worker for test_gpu_vq_kmeans.py: KMeansCodebookInit.run with real processes sharing GPU 0 and the host-staged
communicator of tests/dp_gpu_worker.py.

  rank <r> <n> <dir>   one of n processes: its own pool (seeded by the rank), run(comm=...), saves W and the counts;
  single <n> <dir>     ONE process with rank 0's pool and no communicator: what every rank's W must equal bit for bit.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, 'chainer-vq-vae_amd'), os.path.join(ROOT, 'oracle'), HERE):
    sys.path.insert(0, p)

from dp_gpu_worker import HostStagedCommunicator  # noqa: E402

K, D, B, T, CALLS, ITERS, SEED = 48, 32, 2, 150, 3, 3, 5


def _run(rank, comm):
    import vqvae_amd as V
    from vqvae_amd import backend
    backend.init(0)
    vq = V.VQ(K, D)
    vq.W.data = (np.random.RandomState(100 + rank).standard_normal((K, D)) * 0.01).astype(np.float32)   # differs per rank: overwritten
    vq.to_gpu()
    init = V.KMeansCodebookInit(vq, rows=B * T * CALLS, iters=ITERS, seed=SEED)
    rs = np.random.RandomState(rank)
    for _ in range(CALLS):
        init.collect(backend.to_device((rs.standard_normal((B, D, T)) + rank).astype(np.float32)))
    rep = init.run(comm=comm)
    return vq.W.data.get(), rep


if __name__ == '__main__':
    if sys.argv[1] == 'rank':
        rank, n, directory = int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
        comm = HostStagedCommunicator(rank, n, directory)
        W, rep = _run(rank, comm)
        assert (rep['rows'] is None) == (rank != 0) and len(rep['inertia']) == (ITERS + 1 if rank == 0 else 1)
        np.save(os.path.join(directory, 'W_rank%d.npy' % rank), W)
        np.save(os.path.join(directory, 'counts_rank%d.npy' % rank), rep['counts'])
        np.save(os.path.join(directory, 'calls_rank%d.npy' % rank), np.array(comm.calls))
    else:
        W, rep = _run(0, None)
        np.save(os.path.join(sys.argv[3], 'W_single.npy'), W)
