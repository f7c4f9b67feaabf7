"""Host side of the ragged front end (vqvae_amd.frontend, include/vqvae_ragged.h): the length rule, the chunk planner,
LatentCodes, every argument error (all raised before anything touches a device) and the exported symbols."""
import ctypes as C
import os

import numpy as np
import pytest

import ragged_frontend_ref as R
import vqvae_oracle as O
from vqvae_amd import _lib, backend, frontend
from vqvae_amd.backend import DeviceArray
from vqvae_amd.corpus import ResidentCorpus
from vqvae_amd.frontend import LatentCodes, plan_chunks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'chainer-vq-vae_amd', 'csrc')


# ---- the length rule -------------------------------------------------------------------------------------------------
def test_length_rule_is_the_oracles_for_every_length():
    for t in range(2, 301):
        want = O.conv_out_len(t, 4, 2, 1, 1)
        assert R.length_rule(t) == want == int(frontend.conv_out_len(t)) == (t - 2) // 2 + 1
    lengths = np.arange(2, 301)
    got = frontend.stage_lengths(lengths)
    assert got.shape == (7, 299) and got.dtype == np.int64
    for col, t in enumerate(lengths):
        assert got[:, col].tolist() == R.stage_lengths(t)
    assert int(frontend.conv_out_len(1)) == 0 and int(frontend.conv_out_len(0)) == 0
    assert R.latent_length(64) == 1 and R.latent_length(63) == 0 and R.latent_length(2623) == 40
    assert R.stage_lengths(2623) == [2623, 1311, 655, 327, 163, 81, 40]


# ---- the chunk planner -----------------------------------------------------------------------------------------------
WIDTHS = [1, 8, 8, 8, 8, 8, 8]


def _largest_stage_bytes(lengths, widths):
    per = frontend.stage_lengths(lengths, len(widths) - 1) * np.asarray(widths)[:, None]
    return 4 * int(per.sum(axis=1).max())


def test_planner_keeps_order_and_budget():
    rs = np.random.RandomState(5)
    lengths = rs.randint(64, 6000, 40)
    for budget in (1, 20000, 100000, 1 << 30):
        chunks = plan_chunks(lengths, WIDTHS, budget)
        assert chunks == R.plan_chunks(lengths.tolist(), WIDTHS, budget)
        assert chunks[0][0] == 0 and chunks[-1][1] == len(lengths)
        assert all(a[1] == b[0] for a, b in zip(chunks, chunks[1:])) and all(b > a for a, b in chunks)
        for a, b in chunks:
            if b - a > 1:                                    # a run of several fits; only a single utterance may exceed
                assert _largest_stage_bytes(lengths[a:b], WIDTHS) <= budget
            if b < len(lengths):                             # greedy: the next utterance did not fit
                assert _largest_stage_bytes(lengths[a:b + 1], WIDTHS) > budget
    assert plan_chunks(lengths, WIDTHS, 1) == [(i, i + 1) for i in range(40)]
    assert plan_chunks(lengths, WIDTHS, 1 << 30) == [(0, 40)]


def test_planner_leaves_an_oversize_utterance_alone():
    lengths = [100, 100, 50000, 100, 100]
    budget = _largest_stage_bytes([100, 100], WIDTHS)
    assert plan_chunks(lengths, WIDTHS, budget) == [(0, 2), (2, 3), (3, 5)]
    assert plan_chunks([50000], WIDTHS, 8) == [(0, 1)]


def test_planner_caps_a_stage_below_2_to_the_31_elements():
    big = (1 << 20) + 2                                      # stage 1: 2^19 columns of 512 channels = 2^28 elements
    chunks = plan_chunks([big] * 9, [1, 512], 1 << 62)
    assert chunks == R.plan_chunks([big] * 9, [1, 512], 1 << 62) == [(0, 7), (7, 9)]
    for a, b in chunks:
        assert 512 * int(frontend.stage_lengths([big] * (b - a), 1)[1].sum()) < 1 << 31
    with pytest.raises(ValueError, match='utterance 1 .* alone reaches 2\\^31'):
        plan_chunks([64, 1 << 23], [1, 512], 1 << 30)
    with pytest.raises(ValueError, match='widths'):
        plan_chunks([64], [], 1)
    with pytest.raises(ValueError, match='chunk_bytes'):
        plan_chunks([64], [1], 0)


# ---- LatentCodes -----------------------------------------------------------------------------------------------------
def test_latent_codes_round_trip(tmp_path):
    tl = [1, 4, 2]
    idx = np.array([3, 0, 1, 2, 3, 6, 5], np.int32)
    codes = LatentCodes(tl, idx, 7)
    assert len(codes) == 3 and codes.k == 7 and codes.offsets.tolist() == [0, 1, 5, 7] and codes.tl.dtype == np.int32
    assert [c.tolist() for c in codes.to_host()] == [[3], [0, 1, 2, 3], [6, 5]]
    for name in ('codes', 'codes.npz'):
        codes.save(str(tmp_path / name))
        assert sorted(os.listdir(str(tmp_path))) == ['codes.npz']
        with np.load(str(tmp_path / 'codes.npz')) as f:
            assert sorted(f.files) == ['indices', 'k', 'tl'] and int(f['k']) == 7 and f['indices'].dtype == np.int32
        back = LatentCodes.load(str(tmp_path / name))
        assert back.k == 7 and back.tl.tolist() == tl
        assert all(np.array_equal(a, b) and a.dtype == np.int32 for a, b in zip(back.to_host(), codes.to_host()))
    np.savez(str(tmp_path / 'bad.npz'), tl=np.array(tl), indices=np.array([3, 0, 1, 7, 3, 6, 5]), k=7)
    with pytest.raises(ValueError, match='code 7 at position 3 is outside the codebook \\(k = 7\\)'):
        LatentCodes.load(str(tmp_path / 'bad.npz'))
    np.savez(str(tmp_path / 'short.npz'), tl=np.array(tl), indices=np.array([3, 0]), k=7)
    with pytest.raises(ValueError, match='sum\\(tl\\) = 7'):
        LatentCodes.load(str(tmp_path / 'short.npz'))
    np.savez(str(tmp_path / 'nok.npz'), tl=np.array(tl), indices=idx)
    with pytest.raises(ValueError, match='lacks k'):
        LatentCodes.load(str(tmp_path / 'nok.npz'))
    with pytest.raises(ValueError, match='tl must be'):
        LatentCodes([0, 2], [1, 1], 4)
    with pytest.raises(ValueError, match='outside the codebook'):
        LatentCodes([2], [0, -1], 4)
    with pytest.raises(IndexError):
        codes.codes(3)


# ---- argument errors: all before the first device call ---------------------------------------------------------------
def _fake(shape):
    """A DeviceArray that owns nothing: the checks below must refuse the call before any pointer is used."""
    return DeviceArray(shape, np.float32, _block=object(), _ptr=0x10000)


def _links(d=8, Cl=6, k=5, G=4, n_speaker=3, device=True, shaped=True):
    from vqvae_amd.net import ConditionEmbed, Encoder
    from vqvae_amd.utils import VQ
    mk = _fake if device else (lambda shape: np.zeros(shape, np.float32))
    enc, vq, ce = Encoder(d), VQ(k, d), ConditionEmbed(n_speaker, G, Cl)
    ci = 1
    for s in range(1, 7):
        conv = getattr(enc, 'conv%d' % s)
        conv.W.data, conv.b.data = mk((d, ci, 4, 1)), mk((d,))
        ci = d
    vq.W.data = mk((k, d))
    ci = d
    for i in range(1, 6):
        conv = getattr(ce, 'local_embed%d' % i)
        if shaped:
            conv.W.data = mk((Cl, ci, 3, 1))
        conv.b.data = mk((Cl,))
        ci = Cl
    ce.global_embed.W.data = mk((n_speaker, G))
    return enc, vq, ce


def test_argument_errors_name_the_problem():
    enc, vq, ce = _links()
    waves = [np.zeros(200, np.float32), np.zeros(63, np.float32), np.zeros(64, np.float32)]
    with pytest.raises(ValueError, match='encode_many: utterance 1 has 63 samples, too short for one latent frame'):
        frontend.encode_many(enc, vq, waves)
    with pytest.raises(ValueError, match='frontend_many: utterance 1 has 63 samples'):
        frontend.frontend_many(enc, vq, ce, waves, [0, 1, 2])
    ok = [waves[0], waves[2]]
    with pytest.raises(ValueError, match='frontend_many: one integer speaker id per utterance \\(2\\)'):
        frontend.frontend_many(enc, vq, ce, ok, [0, 1, 2])
    with pytest.raises(ValueError, match='speaker ids must be in \\[0, 3\\)'):
        frontend.frontend_many(enc, vq, ce, ok, [0, 3])
    with pytest.raises(ValueError, match='no utterances'):
        frontend.encode_many(enc, vq, [])
    _, _, lazy = _links(shaped=False)
    with pytest.raises(ValueError, match='condition_embed.local_embed1.W has not been created yet'):
        frontend.frontend_many(enc, vq, lazy, ok, [0, 1])
    henc, hvq, hce = _links(device=False)
    with pytest.raises(ValueError, match='encoder.conv1.W is not on the device'):
        frontend.encode_many(henc, vq, ok)
    with pytest.raises(ValueError, match='vq.W is not on the device'):
        frontend.encode_many(enc, hvq, ok)
    with pytest.raises(ValueError, match='condition_embed.local_embed1.W is not on the device'):
        frontend.frontend_many(enc, vq, hce, ok, [0, 1])
    codes = LatentCodes([2, 1], [0, 4, 5], 6)                 # code 5 fits k = 6, not this codebook's k = 5
    with pytest.raises(ValueError, match='condition_many: the codes were taken from a codebook of k = 6, this one has k = 5'):
        frontend.condition_many(vq, ce, codes, [0, 1])
    with pytest.raises(TypeError, match='condition_many: codes must be a LatentCodes'):
        frontend.condition_many(vq, ce, [0, 1], [0, 1])
    with pytest.raises(ValueError, match='condition_many: one integer speaker id per utterance \\(2\\)'):
        frontend.condition_many(vq, ce, LatentCodes([2, 1], [0, 4, 1], 5), [0])
    wide = _links(d=16)[0]
    with pytest.raises(ValueError, match='the encoder writes 16 channels, the codebook has d = 8'):
        frontend.encode_many(wide, vq, ok)
    with pytest.raises(RuntimeError, match='description only'):
        ResidentCorpus.describe([200, 64], [0, 1]).encode(enc, vq)
    with pytest.raises(ValueError, match='encode: utterance 1 has 10 samples'):
        c = ResidentCorpus.describe([200, 10], [0, 1])
        c.samples = _fake((210,))
        c.encode(enc, vq)


def test_synthesize_many_refuses_the_batched_front_end_without_the_latent_condition():
    from vqvae_amd.synthesis import synthesize_many
    with pytest.raises(ValueError, match='batched_frontend needs latent_condition=True'):
        synthesize_many(None, None, None, None, [np.zeros(64, np.float32)], [0], batched_frontend=True)


# ---- the header, the table, the library ------------------------------------------------------------------------------
NAMES = {'vqvae_ragged_abi_version', 'vqvae_ragged_conv_workspace_bytes', 'vqvae_ragged_conv_fwd',
         'vqvae_ragged_code_gather', 'vqvae_ragged_speaker_gather'}


def test_header_exports_are_the_bound_table():
    import vqvae_amd as V
    for name in ('LatentCodes', 'encode_many', 'condition_many', 'frontend_many', 'plan_chunks'):
        assert getattr(V, name) is getattr(frontend, name)
    table = _lib.HEADERS['vqvae_ragged.h'].prototypes          # against the header and the library: tests/test_host_abi.py
    assert set(table) == NAMES
    for name, n_args in (('vqvae_ragged_conv_fwd', 11), ('vqvae_ragged_code_gather', 7), ('vqvae_ragged_speaker_gather', 7)):
        assert len(table[name][1]) == n_args
    assert 'ragged' not in open(os.path.join(ROOT, 'include', 'vqvae_hip.h')).read()
    assert 'ragged_front.hip' in open(os.path.join(CSRC, 'Makefile')).read()


def test_c_side_validation_needs_no_device():
    lib = _lib.load()
    fake = 0x10000                                           # never dereferenced: every call below is rejected first

    def desc(**kw):
        d = _lib.RaggedConvDesc()
        d.n, d.cin, d.cout, d.K, d.stride, d.pad, d.dil, d.ttot_out, d.x_cstride = 2, 8, 8, 4, 2, 1, 1, 10, 22
        for name, v in kw.items():
            setattr(d, name, v)
        return d

    def conv(d, x=fake, off_out=fake):
        return lib.vqvae_ragged_conv_fwd(C.byref(d), x, fake, fake, off_out, fake, None, fake, None, 0, None)

    assert lib.vqvae_ragged_conv_workspace_bytes(C.byref(desc())) == 0
    assert lib.vqvae_ragged_conv_workspace_bytes(C.byref(desc(K=3, stride=1, pad=16, dil=16))) == 0
    for kw, msg in ((dict(n=0), 'n, cin and cout'), (dict(cout=0), 'n, cin and cout'), (dict(ttot_out=0), 'ttot_out'),
                    (dict(K=3), '(K, stride, pad, dil)'), (dict(K=3, stride=1, pad=3, dil=3), '(K, stride, pad, dil)'),
                    (dict(K=3, stride=1, pad=1, dil=2), '(K, stride, pad, dil)'), (dict(x_cstride=-1), 'x_cstride'),
                    (dict(ttot_out=1 << 40), 'column tiles')):
        d = desc(**kw)
        assert conv(d) == -1 and msg in lib.vqvae_last_error_string().decode(), kw
        if 'column tiles' not in msg:
            assert lib.vqvae_ragged_conv_workspace_bytes(C.byref(d)) == C.c_size_t(-1).value
    assert conv(desc(), x=None) == -1 and 'null x' in lib.vqvae_last_error_string().decode()
    assert conv(desc(), off_out=None) == -1
    assert lib.vqvae_ragged_conv_fwd(None, fake, fake, fake, fake, fake, None, fake, None, 0, None) == -1
    assert lib.vqvae_ragged_code_gather(None, fake, 4, 8, 5, fake, None) == -1
    assert lib.vqvae_ragged_code_gather(fake, fake, 0, 8, 5, fake, None) == -1
    assert 'ttot, d and k' in lib.vqvae_last_error_string().decode()
    assert lib.vqvae_ragged_speaker_gather(fake, None, 2, 4, 3, fake, None) == -1
    assert lib.vqvae_ragged_speaker_gather(fake, fake, 2, 0, 3, fake, None) == -1
    assert 'n, G and n_speaker' in lib.vqvae_last_error_string().decode()
