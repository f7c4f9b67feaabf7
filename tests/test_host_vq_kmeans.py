"""CPU checks of the k-means codebook initialisation's surface (include/vqvae_kmeans.h, vqvae_amd/codebook_init.py): a fourth
header beside the three existing ones, argument validation before anything touches a device, the Python object on a
host-resident link, the snapshot keys, the NumPy restatement (tests/vq_kmeans_ref.py) on examples small enough to check by
hand, and the compiled kernels' resources."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import vq_ema_ref as E
import vq_kmeans_ref as R
from test_host_vq_ema import _Upd, _meta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'chainer-vq-vae_amd', 'csrc')
NAMES = {'vqvae_kmeans_abi_version', 'vqvae_kmeans_workspace_bytes', 'vqvae_kmeans_collect', 'vqvae_kmeans_seed',
         'vqvae_kmeans_update', 'vqvae_kmeans_inertia'}


def test_header_matches_its_prototype_table_and_the_library():
    """The header, the library, the version and the macros: tests/test_host_abi.py, for every header."""
    from vqvae_amd import _lib
    assert set(_lib.HEADERS['vqvae_kmeans.h'].prototypes) == NAMES
    assert _lib.KMEANS_MAX_N == 1 << 24 == _lib.VQ_EMA_MAX_N
    assert R.BLOCK == _lib.KMEANS_BLOCK
    assert 'vq_kmeans.hip' in open(os.path.join(CSRC, 'Makefile')).read()


def test_entry_points_reject_bad_arguments_without_a_device():
    from vqvae_amd import _lib
    lib = _lib.load()
    one = 256           # never dereferenced: validation fails first
    err = lib.vqvae_last_error_string
    big = 1 << 30
    bad_shapes = ((0, 4, 8, b'N ='), (-5, 4, 8, b'N ='), (1 << 24, 4, 8, b'2^24'), (100, 0, 8, b'positive'),
                  (100, 4, 0, b'positive'), (100, 4, -1, b'positive'), (100, _lib.KMEANS_MAX_D + 1, 8, b'range'))
    for N, d, k, _ in bad_shapes:
        assert lib.vqvae_kmeans_workspace_bytes(N, d, k) == 0
    # the workspace: the centre and one float64 per block of 256 rows, each padded to 256 bytes
    for N, d, k in ((1, 1, 1), (7680, 512, 128), (30720, 64, 512), (524288, 128, 8192), ((1 << 24) - 1, 4096, 3)):
        need = lib.vqvae_kmeans_workspace_bytes(N, d, k)
        least = d * 4 + -(-N // 256) * 8
        assert least <= need <= least + 2 * 256 and need % 256 == 0
    # collect(z, B, d, T, count, pool, N, row0, stream)
    for z, pool in ((None, one), (one, None)):
        assert lib.vqvae_kmeans_collect(z, 2, 4, 8, 16, pool, 100, 0, None) == -1
        assert b'null' in err()
    for B, d, T in ((0, 4, 8), (2, 0, 8), (2, 4, 0), (2, -4, 8)):
        assert lib.vqvae_kmeans_collect(one, B, d, T, 1, one, 100, 0, None) == -1
        assert b'positive' in err()
    for N in (0, -1, 1 << 24):
        assert lib.vqvae_kmeans_collect(one, 2, 4, 8, 1, one, N, 0, None) == -1
        assert b'N =' in err()
    for count in (0, -1, 17):
        assert lib.vqvae_kmeans_collect(one, 2, 4, 8, count, one, 100, 0, None) == -1
        assert b'count' in err()
    for row0, count in ((-1, 16), (85, 16), (100, 1), (2 ** 31 - 1, 16)):           # row0 + count overflows the pool (or an int)
        assert lib.vqvae_kmeans_collect(one, 2, 4, 8, count, one, 100, row0, None) == -1
        assert b'do not fit' in err(), err()
    # seed(pool, N, d, k, seed, W, rows, mind, ws, ws_bytes, stream)
    for i in range(5):
        ptrs = [one] * 5
        ptrs[i] = None
        pool, W, rows, mind, ws = ptrs
        assert lib.vqvae_kmeans_seed(pool, 100, 4, 8, 0, W, rows, mind, ws, big, None) == -1
        assert b'null' in err()
    for N, d, k, word in bad_shapes:
        assert lib.vqvae_kmeans_seed(one, N, d, k, 0, one, one, one, one, big, None) == -1
        assert word in err(), (N, d, k, err())
    need = lib.vqvae_kmeans_workspace_bytes(30720, 64, 512)
    assert lib.vqvae_kmeans_seed(one, 30720, 64, 512, 0, one, one, one, one, need - 1, None) == -1
    assert b'workspace' in err()
    # update(pool, N, d, k, stats, seed, iter, W, n_empty, stream)
    for i in range(4):
        ptrs = [one] * 4
        ptrs[i] = None
        pool, stats, W, ne = ptrs
        assert lib.vqvae_kmeans_update(pool, 100, 4, 8, stats, 0, 0, W, ne, None) == -1
        assert b'null' in err()
    for N, d, k, word in bad_shapes:
        assert lib.vqvae_kmeans_update(one, N, d, k, one, 0, 0, one, one, None) == -1
        assert word in err(), (N, d, k, err())
    assert lib.vqvae_kmeans_update(one, 100, 4, 8, one, 0, -1, one, one, None) == -1
    assert b'iter' in err()
    # inertia(pool, W, idx, N, d, k, out, ws, ws_bytes, stream)
    for i in range(5):
        ptrs = [one] * 5
        ptrs[i] = None
        pool, W, idx, out, ws = ptrs
        assert lib.vqvae_kmeans_inertia(pool, W, idx, 100, 4, 8, out, ws, big, None) == -1
        assert b'null' in err()
    for N, d, k, word in bad_shapes:
        assert lib.vqvae_kmeans_inertia(one, one, one, N, d, k, one, one, big, None) == -1
        assert word in err(), (N, d, k, err())
    assert lib.vqvae_kmeans_inertia(one, one, one, 30720, 64, 512, one, one, need - 1, None) == -1
    assert b'workspace' in err()


def test_hash_fixed_vectors():
    """The hash is the monitor's (codebook.reservoir_rows) with the counter's high word as the stream; the values below
    were computed once with Python integers."""
    from vqvae_amd.codebook import reservoir_rows

    def py(seed, word, j):
        M = (1 << 64) - 1
        x = (seed + (((word << 32) | j) + 1) * 0x9E3779B97F4A7C15) & M
        x ^= x >> 30
        x = x * 0xBF58476D1CE4E5B9 & M
        x ^= x >> 27
        x = x * 0x94D049BB133111EB & M
        return x ^ (x >> 31)
    assert py(0, 0, 0) == 0xE220A8397B1DCDAF                   # splitmix64's first output for seed 0
    for seed, word in ((0, 0), (12345, 0), (2 ** 64 - 1, 3), (0x1234567890ABCDEF, 11)):
        x = R.hash64(seed, word, np.arange(40))
        assert [int(v) for v in x] == [py(seed, word, j) for j in range(40)]
        for n in (1, 7, 1920, (1 << 24) - 1):
            assert (reservoir_rows(seed, word, 40, n) == (x % np.uint64(n)).astype(np.int64)).all()
    u = R.uniform(np.uint64(0xFFFFFFFFFFFFFFFF))
    assert u == 1.0 - 2.0 ** -24 and R.uniform(np.uint64((1 << 40) - 1)) == 0.0 and R.uniform(np.uint64(1 << 63)) == 0.5


def test_restatement_on_examples_checked_by_hand():
    f = np.float32
    # the distance: sequential over the channels, every operation rounded to float32
    pool = np.array([[0.0, 3.0, 1e8], [0.0, 4.0, 1.0]], f)           # d = 2, N = 3
    assert R.dist(pool, f([0, 0])).tolist() == [0.0, 25.0, float(f(f(1e8) * f(1e8)) + f(1.0))]
    # the tree: pairs first; padding with +0 changes nothing; the order is NOT left to right
    v = f([1.0, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 5.0])
    lv = R.tree(v)
    assert [l.size for l in lv] == [8, 4, 2, 1]
    assert lv[1].tolist() == [1.0 + 2.0 ** -24, 2.0 ** -23, 5.0, 0.0] and lv[3][0] == (1.0 + 2.0 ** -24 + 2.0 ** -23) + 5.0
    big = np.float64(2.0 ** 53)
    assert R.tree_sum(f([2.0 ** 53, 0.0, 1.0, 1.0])) == big + 2.0 != (big + 1.0) + 1.0
    # the walk: t in [0, 1) -> leaf 0, [1, 3) -> leaf 1, leaf 2 holds 0 and is never reached, [3, 7) -> leaf 3
    lv = R.tree(f([1.0, 2.0, 0.0, 4.0]))
    assert [R.descend(lv, t) for t in (0.0, 0.999, 1.0, 2.999, 3.0, 6.999)] == [0, 0, 1, 1, 3, 3]
    assert R.descend(lv, 7.5) == 3 and R.descend(R.tree(f([1.0, 2.0, 4.0, 0.0])), 99.0) == 2      # never a leaf that holds 0
    # seeding a pool with three distinct rows, k = 5: rounds 3 and 4 meet total == 0 and fall back to the hash
    pool = np.array([[0.0, 0.0, 10.0, 10.0, 0.0, 1.0]], f)            # d = 1, N = 6; rows 0, 1, 4 coincide, so do 2, 3
    W, rows, mind, totals = R.seed(pool, 5, 7)
    x = R.hash64(7, 0, np.arange(5))
    assert rows[0] == int(x[0] % np.uint64(6))
    assert len(set(pool[0, rows[:3]].tolist())) == 3                   # three rounds, three distinct values
    assert totals[2:] == [0.0, 0.0] and totals[0] > totals[1] > 0
    assert rows[3:].tolist() == [int(x[3] % np.uint64(6)), int(x[4] % np.uint64(6))]
    assert (mind == 0).all() and W[:, 0].tolist() == pool[0, rows].tolist()
    # round 1 by hand: D after round 0, the walk with u_1 * total
    D = R.dist(pool, pool[:, rows[0]])
    assert totals[0] == R.tree_sum(D) == float(D.astype(np.float64).sum())
    assert rows[1] == R.descend(R.tree(D), R.uniform(x[1]) * totals[0]) and D[rows[1]] > 0
    # k = 1 and k > N
    assert R.seed(pool, 1, 7)[1].tolist() == [rows[0]] and R.seed(pool[:, :2], 4, 1)[3] == [0.0, 0.0, 0.0]
    # the update: means where a code has rows, a hashed pool row where it has none
    pool = np.array([[1.0, 2.0, 4.0, 100.0], [0.0, 1.0, 0.0, 7.0]], f)
    idx = np.array([[2, 2, 2, 0]], np.int32)
    n, S = E.accumulate(idx, pool[None], 3)
    assert n.tolist() == [1.0, 0.0, 3.0]
    W, n_empty = R.update(pool, n, S, 9, 4)
    row = int(R.hash64(9, 5, 1) % np.uint64(4))
    assert n_empty == 1 and W.tolist() == [[100.0, 7.0], pool[:, row].tolist(), [float(f(7.0) / f(3.0)), float(f(1.0) / f(3.0))]]
    # the inertia: distances to the row's own code, indices outside the codebook count nothing
    Wt = np.array([[100.0, 7.0], [0.0, 0.0], [2.0, 0.0]], f)
    assert R.inertia(pool, Wt, idx) == 1.0 + 1.0 + 4.0 + 0.0
    assert R.inertia(pool, Wt, np.array([2, -1, 3, 0])) == 1.0
    assert R.argmin_exact(pool, Wt).tolist() == [1, 2, 2, 0]           # row 0 is 1 from code 1 and from code 2: the first minimum wins
    # Lloyd from the seeding never increases the inertia while no cluster is empty
    rs = np.random.RandomState(3)
    pool = np.concatenate([rs.standard_normal((3, 40)) * 0.1 + c for c in (-3, 0, 3)], 1).astype(f)
    W = R.seed(pool, 3, 0)[0]
    last = None
    for it in range(4):
        idx = R.argmin_exact(pool, W)
        cur = R.inertia(pool, W, idx)
        assert last is None or cur <= last
        last = cur
        n, S = E.accumulate(idx[None], pool[None], 3)
        W, n_empty = R.update(pool, n, S, 0, it)
        assert n_empty == 0 and n.tolist() == [40.0, 40.0, 40.0]


def test_init_object_on_a_host_link_raises_and_launches_nothing(monkeypatch):
    import vqvae_amd as V
    from vqvae_amd import _lib, codebook_init, core
    assert V.KMeansCodebookInit is codebook_init.KMeansCodebookInit and V.kmeans_init is codebook_init.kmeans_init
    calls = []
    monkeypatch.setattr(_lib, 'call', lambda name, *a: calls.append(name))
    vq = V.VQ(16, 4)                                          # W is a host array
    lazy = V.VQ(16)                                           # no shape yet: allowed, created at the first collect()
    e0 = [core.param_epoch(kind) for kind in ('load', 'monitor', 'layout', 'init')]
    with pytest.raises(ValueError, match='host'):
        V.KMeansCodebookInit(vq, rows=64)
    for bad in (dict(rows=0), dict(rows=-3), dict(rows=1 << 24), dict(rows=64, iters=-1)):
        with pytest.raises(ValueError):
            V.KMeansCodebookInit(lazy, **bad)
    init = V.KMeansCodebookInit(lazy, rows=64, iters=0, seed=-1)
    assert (init.k, init.d, init.rows, init.iters, init.missing, init.seed) == (16, None, 64, 0, 64, (1 << 64) - 1)
    with pytest.raises(ValueError):                           # host latents: no CPU compute path
        init.collect(np.zeros((2, 4, 8), np.float32))
    with pytest.raises(TypeError):
        init.collect([1, 2, 3])
    with pytest.raises(RuntimeError, match='64 of 64 rows are missing'):
        init.run()
    assert lazy.W.data is None and init.pool is None
    assert [n for n, _ in vq.namedparams()] == ['/W']
    assert calls == [] and e0 == [core.param_epoch(kind) for kind in ('load', 'monitor', 'layout', 'init')]


def test_snapshot_keys_do_not_change(tmp_path):
    """The result of the initialisation is W itself: an init object adds nothing to a snapshot."""
    import vqvae_amd as V
    from vqvae_amd import serializers
    import helpers as H
    P, model = H.build_model(dict(H.SMALL), seed=0)
    upd = _Upd(model)

    def keys(name):
        path = str(tmp_path / name)
        serializers.save_npz(path, upd)
        with np.load(path) as f:
            return set(f.files)
    want = keys('plain.npz')
    assert want == set(serializers.model_state(model)) | {'updater/optimizer:main/t', 'updater/optimizer:main/epoch',
                                                          'updater/iteration'}
    with pytest.raises(ValueError, match='host'):
        V.KMeansCodebookInit(model.vq, rows=128)
    lazy = V.VQ(8)
    init = V.KMeansCodebookInit(lazy, rows=128)
    assert keys('again.npz') == want and init.missing == 128


@pytest.fixture(scope='module')
def kmeans_asm(tmp_path_factory):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    out = str(tmp_path_factory.mktemp('vq_kmeans') / 'vq_kmeans.s')
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-S',
                           '--cuda-device-only', os.path.join(CSRC, 'vq_kmeans.hip'), '-o', out], stderr=subprocess.DEVNULL)
    return open(out).read()


def test_compiled_kernels_keep_their_rows_in_registers(kmeans_asm, record_property):
    meta = _meta(kmeans_asm)
    kernels = ('kmeans_dist_kernel', 'kmeans_inertia_kernel', 'kmeans_pick_kernel', 'kmeans_total_kernel',
               'kmeans_collect_kernel', 'kmeans_update_kernel')
    by = {want: [m for name, m in meta.items() if want in name] for want in kernels}
    assert all(by.values()), [k for k, v in by.items() if not v]
    assert len(by['kmeans_dist_kernel']) == 4                      # four rows or one row a thread x first round or later
    for want, ms in by.items():
        for m in ms:
            record_property(want, '%(vgpr)d VGPRs, %(lds)d B LDS, %(threads)d threads' % m)
            assert (m['scratch'], m['spill'], m['wave']) == (0, 0, 64), (want, m)
    assert all(m['threads'] == 256 and m['vgpr'] <= 64 for m in by['kmeans_dist_kernel'] + by['kmeans_inertia_kernel'])
    assert sorted(m['lds'] for m in by['kmeans_dist_kernel']) == [0, 0, 32, 32]      # four wave sums where a workgroup is a block
    # the pick kernel's tree: 2 x 2 048 float64 nodes of a chunk, 2 x 32 chunk roots, the two hand-over words
    assert by['kmeans_pick_kernel'][0]['threads'] == 1024 and 2 * 2048 * 8 + 2 * 32 * 8 <= by['kmeans_pick_kernel'][0]['lds'] <= 34 * 1024
    assert 'scratch_' not in kmeans_asm
    assert not re.search(r'atomic_(add|pk_add)_f(32|64)|atomic_fadd', kmeans_asm)     # one integer atomic (n_empty), no float ones
    assert 's_load_dword' in kmeans_asm                            # the round's centre comes through the scalar path
