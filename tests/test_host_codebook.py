"""CPU checks of the codebook monitor's surface (include/vqvae_codebook.h, vqvae_amd/codebook.py): the new entry points
live beside the existing ABI without touching it, the reservoir hash and the data-parallel owner rule are what the header
says (restated here in plain Python integers), and nothing changes for a model without a monitor."""
import numpy as np

M64 = (1 << 64) - 1


def test_codebook_header_matches_its_prototype_table_and_the_library():
    """The header, the library, the version and the macros: tests/test_host_abi.py, for every header."""
    from vqvae_amd import _lib
    assert set(_lib.HEADERS['vqvae_codebook.h'].prototypes) == {'vqvae_codebook_abi_version', 'vqvae_codebook_observe',
                                                                'vqvae_codebook_reseed'}
    assert not [e for e in _lib.PROTOTYPES if 'codebook' in e]            # vqvae_hip.h does not speak of the monitor


def test_entry_points_reject_bad_arguments_without_a_device():
    from vqvae_amd import _lib
    lib = _lib.load()
    assert lib.vqvae_codebook_observe(None, None, 1, 1, 1, 1, 0.5, 0, None, None, None, None, None, None) == -1
    assert b'null' in lib.vqvae_last_error_string()
    one = 256           # never dereferenced: validation fails first
    assert lib.vqvae_codebook_observe(one, one, 1, 0, 1, 1, 0.5, 0, one, one, one, one, one, None) == -1
    assert lib.vqvae_codebook_observe(one, one, 1, 4, 1, 8, 1.5, 0, one, one, one, one, one, None) == -1
    assert lib.vqvae_codebook_observe(one, one, 1 << 20, 4, 1 << 12, 8, 0.5, 0, one, one, one, one, one, None) == -1
    assert lib.vqvae_codebook_reseed(one, one, None, 8, 4, one, one, 0.1, 0.1, one, one, None) == -1
    assert b'both' in lib.vqvae_last_error_string()
    assert lib.vqvae_codebook_reseed(one, None, None, 0, 4, one, one, 0.1, 0.1, one, one, None) == -1


def _hash(seed, step, j):
    """include/vqvae_codebook.h, in Python integers."""
    ctr = ((step & 0xFFFFFFFF) << 32) | (j & 0xFFFFFFFF)
    x = (seed + (ctr + 1) * 0x9E3779B97F4A7C15) & M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x


def test_reservoir_hash_fixed_vectors():
    from vqvae_amd.codebook import reservoir_rows
    # seed 0, step 0, j = 0 is splitmix64's first output for state 0
    assert _hash(0, 0, 0) == 0xE220A8397B1DCDAF
    assert [_hash(0, 0, j) % 1920 for j in range(4)] == [175, 1140, 79, 364]
    assert [_hash(M64, 3, j) % 1000003 for j in range(4)] == [284764, 947688, 968427, 917815]
    for seed, step, k, n in ((0, 0, 512, 1920), (12345678901234567890, 7, 8192, 1048560), (M64, 2 ** 31 - 1, 130, 7),
                             (1, 1, 3, 1)):
        got = reservoir_rows(seed, step, k, n)
        assert got.dtype == np.int64 and got.shape == (k,)
        assert got.tolist() == [_hash(seed, step, j) % n for j in range(k)]
        assert got.min() >= 0 and got.max() < n
    # a draw per step: consecutive steps and seeds give different rows
    assert (reservoir_rows(0, 0, 512, 1920) != reservoir_rows(0, 1, 512, 1920)).mean() > 0.95
    assert (reservoir_rows(0, 0, 512, 1920) != reservoir_rows(1, 0, 512, 1920)).mean() > 0.95


def test_owner_rule():
    from vqvae_amd.codebook import reservoir_owner
    assert reservoir_owner(np.arange(6), 0, 2).tolist() == [0, 1, 0, 1, 0, 1]
    assert reservoir_owner(np.arange(6), 3, 2).tolist() == [1, 0, 1, 0, 1, 0]
    assert reservoir_owner(np.arange(7), 5, 3).tolist() == [(j + 5) % 3 for j in range(7)]
    assert reservoir_owner(np.arange(5), 123, 1).tolist() == [0] * 5
    # what reseed() copies for rank r: rows first, first + size, ... with first = (r - steps) mod size
    for size in (2, 3, 8):
        for steps in (0, 1, 7, 500):
            owners = reservoir_owner(np.arange(37), steps, size)
            for r in range(size):
                first = (r - steps) % size
                assert np.nonzero(owners == r)[0].tolist() == list(range(first, 37, size))


def test_vq_has_no_monitor_by_default_and_attaching_is_noticed_by_recordings():
    import vqvae_amd as V
    from vqvae_amd import core
    assert V.CodebookMonitor is V.codebook.CodebookMonitor
    vq = V.VQ(16, 4)
    assert vq.monitor is None and vq._monitor is None
    e0 = core.param_epoch('monitor')
    mon = V.CodebookMonitor(vq, decay=0.9, seed=3)       # host codebook: no device state yet, nothing launched
    assert mon.d is None and (mon.k, mon.decay, mon.seed) == (16, 0.9, 3)
    vq.monitor = mon
    assert vq.monitor is mon and core.param_epoch('monitor') == e0 + 1
    vq.monitor = mon
    assert core.param_epoch('monitor') == e0 + 1
    vq.monitor = None
    assert vq.monitor is None and core.param_epoch('monitor') == e0 + 2
    assert [n for n, _ in vq.namedparams()] == ['/W']     # the monitor is not a parameter or a child link


class _Opt(object):
    """What serializers.save_npz reads of an optimizer, over host parameters."""
    t = 3

    def __init__(self, target):
        self.target = target
        self.n_train = 0

    def layout(self):
        return []

    class _Z(object):
        @staticmethod
        def get():
            return np.zeros(0, np.float32)
    m = v = _Z()


class _Upd(object):
    iteration = 7

    def __init__(self, model):
        self.opt = _Opt(model)

    def get_optimizer(self, name):
        return self.opt


def test_snapshot_keys_change_only_when_a_monitor_is_attached(tmp_path):
    import vqvae_amd as V
    from vqvae_amd import serializers
    from vqvae_amd.codebook import SNAPSHOT_PREFIX
    import helpers as H
    P, model = H.build_model(dict(H.SMALL), seed=0)
    upd = _Upd(model)
    plain = str(tmp_path / 'plain.npz')
    serializers.save_npz(plain, upd)
    with np.load(plain) as f:
        keys = set(f.files)
    want = set(serializers.model_state(model)) | {'updater/optimizer:main/t', 'updater/optimizer:main/epoch',
                                                  'updater/iteration'}
    assert keys == want and not [k for k in keys if 'codebook' in k]
    mon = V.CodebookMonitor(model.vq, decay=0.75, seed=2 ** 63 + 5)
    model.vq.monitor = mon
    try:
        with_mon = str(tmp_path / 'mon.npz')
        serializers.save_npz(with_mon, upd)
        with np.load(with_mon) as f:
            assert set(f.files) == want | {SNAPSHOT_PREFIX + 'vq/seed', SNAPSHOT_PREFIX + 'vq/decay'}   # no device state yet
            assert int(f[SNAPSHOT_PREFIX + 'vq/seed']) == 2 ** 63 + 5 and float(f[SNAPSHOT_PREFIX + 'vq/decay']) == 0.75
    finally:
        model.vq.monitor = None
    again = str(tmp_path / 'again.npz')
    serializers.save_npz(again, upd)
    with np.load(again) as f:
        assert set(f.files) == want
