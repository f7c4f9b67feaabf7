"""GPU parity of the persistent generation kernel's WIDE class (csrc/generate.hip, MegaWide: vectors of up
to 512 channels, condition up to 640, 256 workgroups) -- the reference's default decoder (params.py: 512 /
512 / 256, condition 640) and the shapes between the two classes -- against the NumPy oracle, the per-step
kernels and the training forward.

tests/test_gpu_generate.py::test_wide_model_runs_on_the_per_step_kernels (320 / 288 channels) predates this
class: with its default arguments that decoder now takes the persistent road too, at the same 1e-4 bar."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import vqvae_oracle as O
from helpers import assert_close, assert_close_scaled
from test_gpu_generate import _cond, _decoder

pytestmark = pytest.mark.gpu


def _wide(residual, dilated, skip, cond, **kw):
    cfg = dict(H.SMALL, residual=residual, dilated=dilated, skip=skip, local_dim=cond - 32, global_dim=32)
    cfg.update(kw)
    return cfg


def _took_persistent_road(dec):
    """GenerationState.run keeps the persistent launch's workspace; the per-step road has none."""
    return getattr(dec._gen, '_last_ws', None) is not None


def _workspace_bytes(dec):
    from vqvae_amd import _lib
    return _lib.load().vqvae_wavenet_gen_run_workspace_bytes(C.byref(dec._gen.desc))


@pytest.mark.parametrize('shape', [(320, 320, 288, 200), (512, 512, 256, 640), (384, 512, 512, 257),
                                   (512, 256, 512, 640)])
def test_teacher_forced_logits(gpu, shape):
    """(residual, dilated, skip, condition), sizes that leave lanes idle in the last chunk of 64 included:
    every step's logits against the oracle (1e-4) and against the per-step kernels (1e-5)."""
    cfg = _wide(*shape)
    p, dec = _decoder(cfg, 61)
    n, T = 2, 24
    cond = _cond(cfg, n, T, 21)
    rs = np.random.RandomState(22)
    forced = rs.randint(0, cfg['input_dim'], (T, n)).astype(np.int32)
    forced[5, 0] = -1
    u = rs.random_sample((T, n))
    _, want = O.wavenet_generate(p, cond, u, cfg['n_loop'], cfg['n_layer'], forced=forced)
    _, got = dec.generate_sequence(gpu.to_device(cond), u, forced=forced, return_logits=True, persistent=True)
    assert _took_persistent_road(dec)
    _, per_step = dec.generate_sequence(gpu.to_device(cond), u, forced=forced, return_logits=True, persistent=False)
    assert not _took_persistent_road(dec)
    assert_close(got.get(), want, 1e-4, 'wide class vs oracle')
    assert_close(got.get(), per_step.get(), 1e-5, 'wide class vs per-step kernels')


def test_free_running_equals_oracle_and_lockstep_equals_alone(gpu):
    """generate.py:105-145 free running on a 512-channel decoder: the oracle's bins for the same uniforms,
    for one sequence and for four in lockstep; a sequence of the group gets what it gets alone."""
    cfg = _wide(512, 512, 256, 640)
    p, dec = _decoder(cfg, 62)
    n, T = 4, 64
    cond = _cond(cfg, n, T, 23)
    u = np.random.RandomState(24).random_sample((T, n))
    want, _ = O.wavenet_generate(p, cond, u, cfg['n_loop'], cfg['n_layer'])
    got4 = dec.generate_sequence(gpu.to_device(cond), u).get()
    assert _took_persistent_road(dec)
    np.testing.assert_array_equal(got4, want)
    for b in range(n):
        alone = dec.generate_sequence(gpu.to_device(cond[b:b + 1]), u[:, b:b + 1]).get()
        np.testing.assert_array_equal(alone, got4[b:b + 1])
    got3 = dec.generate_sequence(gpu.to_device(cond[:3]), u[:, :3]).get()      # the n < 4 instantiation
    np.testing.assert_array_equal(got3, got4[:3])
    assert len(np.unique(got4)) > 10


def test_mol_wide_decoder_matches_oracle(gpu):
    """Mixture-of-logistics output (out_dim 30, scalar feedback into a 1-channel embed) on 384 channels."""
    cfg = dict(H.MOL, n_loop=2, n_layer=4, residual=384, dilated=384, skip=320, local_dim=300, global_dim=32)
    p, dec = _decoder(cfg, 63, use_logistic=True)
    n, T = 2, 60
    cond = _cond(cfg, n, T, 25)
    rs = np.random.RandomState(26)
    u = rs.uniform(0.02, 0.98, (T, n, 10))
    forced = rs.uniform(-1, 1, (T, n)).astype(np.float32)
    want_out, want_logits = O.wavenet_generate(p, cond, u, cfg['n_loop'], cfg['n_layer'], loss_kind='mol', forced=forced)
    out, logits = dec.generate_sequence(gpu.to_device(cond), u, forced=forced, return_logits=True)
    assert _took_persistent_road(dec)
    assert_close(logits.get(), want_logits, 1e-4, 'mol logits')
    np.testing.assert_allclose(out.get(), want_out, rtol=0, atol=2e-5)
    want_out, _ = O.wavenet_generate(p, cond, u, cfg['n_loop'], cfg['n_layer'], loss_kind='mol', n_steps=32)
    got = dec.generate_sequence(gpu.to_device(cond), u, n_steps=32).get()
    np.testing.assert_allclose(got, want_out, rtol=0, atol=1e-3)


def test_partial_steps_and_restart_across_chunks(gpu):
    """Dilations up to 512 (every queue ring wraps), launches of 250 steps: the seams at t0 = 250 and 500
    change nothing, a partial run is a prefix of the full one, logits agree with the per-step kernels."""
    cfg = _wide(320, 320, 288, 200, n_loop=1, n_layer=10)
    p, dec = _decoder(cfg, 64)
    n, T = 2, 600
    cond = _cond(cfg, n, T, 27)
    rs = np.random.RandomState(28)
    u = rs.random_sample((T, n))
    full = dec.generate_sequence(gpu.to_device(cond), u).get()
    dec.initialize(n)
    chunked = dec._gen.run(gpu.to_device(cond), u, 1, persistent=True, chunk=250).get()
    assert _took_persistent_road(dec)
    np.testing.assert_array_equal(chunked, full)
    part = dec.generate_sequence(gpu.to_device(cond), u, n_steps=301).get()
    np.testing.assert_array_equal(part[:, :301], full[:, :301])
    assert (part[:, 301:] == 0).all()
    forced = rs.randint(0, cfg['input_dim'], (T, n)).astype(np.int32)
    dec.initialize(n)
    _, got = dec._gen.run(gpu.to_device(cond), u, 1, forced=forced, return_logits=True, persistent=True, chunk=250)
    _, per_step = dec.generate_sequence(gpu.to_device(cond), u, forced=forced, return_logits=True, persistent=False)
    assert_close(got.get(), per_step.get(), 1e-5, 'chunked wide class vs per-step kernels')


def test_generate_batch_on_a_wide_model(gpu):
    cfg = _wide(512, 512, 256, 640)
    p, dec = _decoder(cfg, 65)
    N, T = 5, 32
    cond = _cond(cfg, N, T, 29)
    u = np.random.RandomState(30).random_sample((T, N))
    got = dec.generate_batch(gpu.to_device(cond), u, group=2, max_streams=4)
    assert got.shape == (N, T)
    for i in range(N):
        alone = dec.generate_sequence(gpu.to_device(cond[i:i + 1]), u[:, i:i + 1]).get()
        np.testing.assert_array_equal(got[i:i + 1], alone)


@pytest.mark.parametrize('shape,inside', [((512, 512, 512, 640), True), ((513, 512, 256, 640), False),
                                          ((512, 512, 256, 641), False), ((512, 514, 256, 640), False)])
def test_dispatch_at_the_class_limits(gpu, shape, inside):
    """Workspace bytes are non-zero exactly inside the class; one channel past it the same call falls back
    to the per-step kernels and still matches the oracle."""
    cfg = _wide(*shape)
    p, dec = _decoder(cfg, 66)
    n, T = 1, 12
    cond = _cond(cfg, n, T, 31)
    rs = np.random.RandomState(32)
    forced = rs.randint(0, cfg['input_dim'], (T, n)).astype(np.int32)
    u = rs.random_sample((T, n))
    _, want = O.wavenet_generate(p, cond, u, cfg['n_loop'], cfg['n_layer'], forced=forced)
    _, got = dec.generate_sequence(gpu.to_device(cond), u, forced=forced, return_logits=True)
    assert_close(got.get(), want, 1e-4, 'logits at %s' % (shape,))
    assert _took_persistent_road(dec) == inside
    assert (_workspace_bytes(dec) > 0) == inside
    with pytest.raises(ValueError):
        dec.initialize(5)                                              # more than 4 lockstep sequences


def test_reference_default_decoder_equals_training_forward(gpu):
    """params.py unedited: 3 x 10 blocks, 512 / 512 / 256, condition 512 + 128.  Step i of the persistent
    loop equals column i of the training forward of the same weights (modules.py:148-160)."""
    from vqvae_amd.core import Variable
    cfg = dict(d=64, k=512, n_loop=3, n_layer=10, filter_size=2, input_dim=256, residual=512,
               dilated=512, skip=256, out_dim=256, local_dim=512, global_dim=128, n_speaker=5)
    p, dec = _decoder(cfg, 67)
    n, T = 1, 64
    cond = _cond(cfg, n, T, 33)
    rs = np.random.RandomState(34)
    forced = rs.randint(0, 256, (T, n)).astype(np.int32)
    u = rs.random_sample((T, n))
    out, logits = dec.generate_sequence(gpu.to_device(cond), u, forced=forced, return_logits=True)
    assert _took_persistent_road(dec)
    x = np.zeros((n, 256, T), np.float32)
    for i in range(T - 1):
        x[0, forced[i, 0], i + 1] = 1
    y = dec(Variable(gpu.to_device(x[..., None])), Variable(gpu.to_device(cond[..., None]))).data.get()
    y = y.reshape(n, 256, T).transpose(2, 0, 1)[:T - 1]
    assert_close_scaled(logits.get(), y, 1e-4, 'wide incremental vs training forward')
