"""CPU checks of the EMA codebook's surface (include/vqvae_vq_ema.h, vqvae_amd/codebook_ema.py): a third header beside the
two existing ones, argument validation before anything touches a device, the Python object on a host-resident link, the
snapshot keys, the NumPy restatement of the rule (tests/vq_ema_ref.py) on a worked example, and the compiled kernels'
resources."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import vq_ema_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'chainer-vq-vae_amd', 'csrc')
NAMES = {'vqvae_vq_ema_abi_version', 'vqvae_vq_ema_workspace_bytes', 'vqvae_vq_ema_accumulate', 'vqvae_vq_ema_apply',
         'vqvae_vq_ema_reset'}


def test_header_matches_its_prototype_table_and_the_library():
    """The header, the library, the version and the macros: tests/test_host_abi.py, for every header."""
    from vqvae_amd import _lib
    assert set(_lib.HEADERS['vqvae_vq_ema.h'].prototypes) == NAMES
    assert _lib.VQ_EMA_MAX_N == 1 << 24
    assert R.PIECE == _lib.VQ_EMA_PIECE


def test_entry_points_reject_bad_arguments_without_a_device():
    from vqvae_amd import _lib
    lib = _lib.load()
    one = 256           # never dereferenced: validation fails first
    err = lib.vqvae_last_error_string
    big = 1 << 30
    # accumulate(idx, z, B, d, T, k, stats, ws, ws_bytes, stream)
    for args in ((None, one, 1, 4, 8, 8, one, one, big), (one, None, 1, 4, 8, 8, one, one, big),
                 (one, one, 1, 4, 8, 8, None, one, big), (one, one, 1, 4, 8, 8, one, None, big)):
        assert lib.vqvae_vq_ema_accumulate(*(args + (None,))) == -1
        assert b'null' in err()
    for B, d, T, k in ((0, 4, 8, 8), (1, 0, 8, 8), (1, 4, 0, 8), (1, 4, 8, 0), (1, 4, 8, -3)):
        assert lib.vqvae_vq_ema_accumulate(one, one, B, d, T, k, one, one, big, None) == -1
        assert b'positive' in err()
        assert lib.vqvae_vq_ema_workspace_bytes(B, d, T, k) == 0
    assert lib.vqvae_vq_ema_accumulate(one, one, 1 << 12, 4, 1 << 12, 8, one, one, big, None) == -1      # N = 2^24
    assert b'2^24' in err()
    assert lib.vqvae_vq_ema_workspace_bytes(1 << 12, 4, 1 << 12, 8) == 0
    for B, d, T, k in ((2, 64, 960, 512), (16, 128, 65535, 8192)):            # one launch / the bucketed form
        need = lib.vqvae_vq_ema_workspace_bytes(B, d, T, k)
        assert need > 0
        assert lib.vqvae_vq_ema_accumulate(one, one, B, d, T, k, one, one, need - 1, None) == -1
        assert b'workspace' in err()
    # the bucketed form's workspace: chunk histograms, two offset tables, the sorted rows, one float64 row per piece
    N, k, d = 16 * 65535, 8192, 128
    need = lib.vqvae_vq_ema_workspace_bytes(16, d, 65535, k)
    least = -(-N // 4096) * k * 4 + 2 * (k + 1) * 4 + N * 4 + (k + N // _lib.VQ_EMA_PIECE) * d * 8
    assert least <= need <= least + 5 * 256
    # apply(W, count, sum, stats, k, d, decay, eps, stream)
    for args in ((None, one, one, one), (one, None, one, one), (one, one, None, one), (one, one, one, None)):
        assert lib.vqvae_vq_ema_apply(*(args + (8, 4, 0.99, 1e-5, None))) == -1
        assert b'null' in err()
    for k, d, decay, eps, word in ((0, 4, 0.99, 1e-5, b'positive'), (8, 0, 0.99, 1e-5, b'positive'), (8, 4, -0.01, 1e-5, b'decay'),
                                   (8, 4, 1.01, 1e-5, b'decay'), (8, 4, float('nan'), 1e-5, b'decay'), (8, 4, 0.99, 0.0, b'eps'),
                                   (8, 4, 0.99, -1.0, b'eps'), (8, 4, 0.99, float('nan'), b'eps')):
        assert lib.vqvae_vq_ema_apply(one, one, one, one, k, d, decay, eps, None) == -1
        assert word in err(), (k, d, decay, eps, err())
    # reset(W, count, sum, k, d, mask, stream)
    for args in ((None, one, one), (one, None, one), (one, one, None)):
        assert lib.vqvae_vq_ema_reset(*(args + (8, 4, None, None))) == -1
        assert b'null' in err()
    assert lib.vqvae_vq_ema_reset(one, one, one, 0, 4, None, None) == -1
    assert lib.vqvae_vq_ema_reset(one, one, one, 8, -1, one, None) == -1


def test_restatement_on_a_worked_example():
    """Two codes, one dimension, by hand: n = (3, 0), S = (6, 0); decay 0.5 from N = 1, m = W."""
    idx = np.array([[0, 0, 5, 0, -1]], np.int32)                  # 5 and -1 are outside [0, 2): ignored
    z = np.array([[[1.0, 2.0, 100.0, 3.0, 100.0]]], np.float32)
    for ordered in (True, False):
        n, S = R.accumulate(idx, z, 2, ordered)
        assert n.tolist() == [3.0, 0.0] and S.tolist() == [[6.0], [0.0]]
    W0 = np.array([[4.0], [8.0]], np.float32)
    W, N, m = R.apply(W0, np.ones(2, np.float32), W0.copy(), n, S, 0.5, 1e-5)
    assert N.tolist() == [2.0, 0.5] and m.tolist() == [[5.0], [4.0]]
    eps = float(np.float32(1e-5))
    nt = [np.float32((v + eps) / (2.5 + 2 * eps) * 2.5) for v in (2.0, 0.5)]
    assert W.tolist() == [[float(np.float32(5.0) / nt[0])], [float(np.float32(4.0) / nt[1])]]
    np.testing.assert_allclose(W[:, 0], [2.5, 8.0], rtol=1e-4)    # the means of what each code has seen
    # total == 0 (decay 0, no valid index): W stays
    W2, N2, m2 = R.apply(W0, np.ones(2, np.float32), W0.copy(), np.zeros(2, np.float32), np.zeros((2, 1), np.float32), 0.0, 1e-5)
    assert W2.tolist() == W0.tolist() and N2.tolist() == [0.0, 0.0] and m2.tolist() == [[0.0], [0.0]]
    # the ordered sum differs from a naive one in the order only: a long list, to within float64 re-association
    rs = np.random.RandomState(0)
    idx = rs.randint(0, 3, (2, 1500)).astype(np.int32)
    z = rs.standard_normal((2, 5, 1500)).astype(np.float32)
    (n1, S1), (n2, S2) = R.accumulate(idx, z, 3, True), R.accumulate(idx, z, 3, False)
    assert n1.tolist() == n2.tolist() == np.bincount(idx.reshape(-1), minlength=3).astype(np.float32).tolist()
    assert np.abs(S1.view(np.int32) - S2.view(np.int32)).max() <= 1


def test_ema_object_on_a_host_link_launches_nothing_and_is_noticed_by_recordings(monkeypatch):
    import vqvae_amd as V
    from vqvae_amd import _lib, codebook_ema, core
    assert V.EMACodebook is codebook_ema.EMACodebook
    calls = []
    monkeypatch.setattr(_lib, 'call', lambda name, *a: calls.append(name))
    vq = V.VQ(16, 4)
    assert vq.codebook_ema is None and vq._codebook_ema is None
    e0 = core.param_epoch('monitor')
    ema = V.EMACodebook(vq)
    assert (ema.k, ema.d, ema.decay, ema.eps) == (16, None, 0.99, 1e-5)
    vq.codebook_ema = ema
    assert vq.codebook_ema is ema and core.param_epoch('monitor') == e0 + 1
    vq.codebook_ema = ema
    assert core.param_epoch('monitor') == e0 + 1
    ema.decay = 0.9                                       # a kernel argument of a recorded step
    assert core.param_epoch('monitor') == e0 + 2 and ema.decay == 0.9
    ema.decay = 0.9
    ema.eps = 1e-5
    assert core.param_epoch('monitor') == e0 + 2
    ema.eps = 1e-3
    assert core.param_epoch('monitor') == e0 + 3
    ema.load_state({'decay': np.asarray(0.9), 'eps': np.asarray(1e-3)})
    assert core.param_epoch('monitor') == e0 + 3
    ema.load_state({'decay': np.asarray(0.5)})
    assert core.param_epoch('monitor') == e0 + 4 and (ema.decay, ema.eps) == (0.5, 1e-3)
    for bad in (dict(decay=-0.1), dict(decay=1.5), dict(eps=0.0), dict(eps=-1.0)):
        with pytest.raises(ValueError):
            V.EMACodebook(vq, **bad)
    with pytest.raises(ValueError):
        ema.decay = 2.0
    with pytest.raises(RuntimeError, match='accumulated'):
        ema.step()
    with pytest.raises(RuntimeError, match='device storage'):
        ema.counts()
    assert codebook_ema.attached_emas(vq) == [('', ema)]
    assert [n for n, _ in vq.namedparams()] == ['/W']     # the object is not a parameter or a child link
    vq.codebook_ema = None
    assert codebook_ema.attached_emas(vq) == [] and core.param_epoch('monitor') == e0 + 5
    assert calls == []


class _Opt(object):
    """What serializers.save_npz reads of an optimizer, over host parameters."""
    t = 3

    def __init__(self, target):
        self.target = target
        self.n_train = 0

    def layout(self):
        return []

    def adopt_new_params(self):
        return False

    class _Z(object):
        @staticmethod
        def get():
            return np.zeros(0, np.float32)

        @staticmethod
        def set(a):
            pass
    m = v = _Z()


class _Upd(object):
    iteration = 7

    def __init__(self, model):
        self.opt = _Opt(model)

    def get_optimizer(self, name):
        return self.opt


def test_snapshot_keys_change_only_when_an_ema_object_is_attached(tmp_path):
    import vqvae_amd as V
    from vqvae_amd import codebook, codebook_ema, serializers
    import helpers as H
    P, model = H.build_model(dict(H.SMALL), seed=0)
    upd = _Upd(model)
    want = set(serializers.model_state(model)) | {'updater/optimizer:main/t', 'updater/optimizer:main/epoch',
                                                  'updater/iteration'}

    def keys(name):
        path = str(tmp_path / name)
        serializers.save_npz(path, upd)
        with np.load(path) as f:
            return path, set(f.files)
    assert keys('plain.npz')[1] == want
    assert codebook_ema.attached_emas(model) == []
    model.vq.monitor = V.CodebookMonitor(model.vq, decay=0.75, seed=5)
    try:
        mon_keys = {codebook.SNAPSHOT_PREFIX + 'vq/seed', codebook.SNAPSHOT_PREFIX + 'vq/decay'}
        assert keys('mon.npz')[1] == want | mon_keys
        ema = V.EMACodebook(model.vq, decay=0.75, eps=1e-4)
        model.vq.codebook_ema = ema
        assert codebook_ema.attached_emas(model) == [('vq', ema)]
        pre = codebook_ema.SNAPSHOT_PREFIX + 'vq/'
        assert pre == 'updater/codebook_ema:main/vq/'
        path, got = keys('both.npz')
        assert got == want | mon_keys | {pre + 'decay', pre + 'eps'}           # a host codebook: no device state yet
        model.vq.monitor = None
        assert keys('ema.npz')[1] == want | {pre + 'decay', pre + 'eps'}
        # round trip: the hyper-parameters come from the file; state that arrives before the device state waits
        ema2 = V.EMACodebook(model.vq)
        model.vq.codebook_ema = ema2
        serializers.load_npz(path, upd)
        assert (ema2.decay, ema2.eps, upd.iteration) == (0.75, 1e-4, 7)
        k, d = model.vq.W.data.shape
        state = dict(ema.state(), count=np.arange(k, dtype=np.float32), sum=np.ones((k, d), np.float32))
        ema2.load_state(state)
        back = ema2.state()
        assert sorted(back) == ['count', 'decay', 'eps', 'sum']
        assert back['count'].tolist() == state['count'].tolist() and (back['sum'] == 1).all()
    finally:
        model.vq.monitor = None
        model.vq.codebook_ema = None
    assert keys('again.npz')[1] == want


@pytest.fixture(scope='module')
def ema_asm(tmp_path_factory):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    out = str(tmp_path_factory.mktemp('vq_ema') / 'vq_ema.s')
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-S',
                           '--cuda-device-only', os.path.join(CSRC, 'vq_ema.hip'), '-o', out], stderr=subprocess.DEVNULL)
    return open(out).read()


def _meta(asm):
    out = {}
    for m in re.finditer(r'\.group_segment_fixed_size:\s*(\d+).*?\.max_flat_workgroup_size:\s*(\d+).*?\.name:\s*(\S+)'
                         r'.*?\.private_segment_fixed_size:\s*(\d+).*?\.vgpr_count:\s*(\d+).*?\.vgpr_spill_count:\s*(\d+)'
                         r'.*?\.wavefront_size:\s*(\d+)', asm, re.S):
        out[m.group(3)] = dict(lds=int(m.group(1)), threads=int(m.group(2)), scratch=int(m.group(4)), vgpr=int(m.group(5)),
                               spill=int(m.group(6)), wave=int(m.group(7)))
    return out


def test_compiled_kernels_keep_their_sums_in_registers(ema_asm, record_property):
    from vqvae_amd import _lib
    meta = _meta(ema_asm)
    kernels = ('ema_scan_kernel', 'ema_hist_kernel', 'ema_colscan_kernel', 'ema_basescan_kernel', 'ema_place_kernel',
               'ema_sum_kernel', 'ema_combine_kernel', 'ema_count_kernel', 'ema_rows_kernel', 'ema_reset_kernel')
    by = {want: [m for name, m in meta.items() if want in name] for want in kernels}
    assert all(by.values()), [k for k, v in by.items() if not v]
    assert len(by['ema_place_kernel']) == 2                       # cursors in LDS / in global memory
    for want, ms in by.items():
        for m in ms:
            record_property(want, '%(vgpr)d VGPRs, %(lds)d B LDS, %(threads)d threads' % m)
            assert (m['scratch'], m['spill'], m['wave']) == (0, 0, 64), (want, m)
    # static LDS is what the source declares: the compacted list of element offsets (8 bytes a row) plus the wave counts
    assert by['ema_scan_kernel'][0]['lds'] == _lib.VQ_EMA_SMALL_MAX_N * 8 + 16 * 4 and by['ema_scan_kernel'][0]['threads'] == 1024
    assert by['ema_sum_kernel'][0]['lds'] == _lib.VQ_EMA_PIECE * 8
    assert all(m['lds'] == 0 for m in by['ema_place_kernel'])     # dynamic: k * 4 bytes, at most 64 KB
    assert all(m['lds'] <= 64 * 1024 for ms in by.values() for m in ms)
    assert 'scratch_' not in ema_asm
    assert not re.search(r'atomic_(add|pk_add)_f(32|64)|atomic_fadd', ema_asm)      # integer atomics only
