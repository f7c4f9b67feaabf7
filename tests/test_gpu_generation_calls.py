"""Which C entry points a generation call issues, and in which order: the run-length-encoded sequence of every
`vqvae_wavenet_gen_*`, `vqvae_gen_*`, `vqvae_sample_*` and `vqvae_graph_*` call behind WaveNet.generate,
generate_sequence, generate_batch and generate_lockstep, compared with a literal list.  Allocations and copies are not
recorded, so they may move freely; the values are held to the oracle by the other generation tests and are not checked
again here, only that a second identical call returns the same arrays (the recorder calls through and changes nothing).

The lists of EXPECTED were printed by this file's own recorder on the commit before generation.py was reorganised around
GenerationState.bind, the step launcher and the replay helper; that change had to leave them as they were."""
import contextlib
import itertools

import numpy as np
import pytest

import helpers as H
from test_gpu_gen_cond import _latent
from test_gpu_generate import _cond, _decoder

pytestmark = pytest.mark.gpu

PREFIXES = ('vqvae_wavenet_gen_', 'vqvae_gen_', 'vqvae_sample_', 'vqvae_graph_')
T = 6
LENGTHS = np.array([6, 5, 4, 3, 2, 2, 1])            # group=5: [6 5 4 3 2] and [2 1 1 1 1] (padded with repeats, 0 steps)
CONTROLS = dict(temperature=[0.0, 1.0, 0.7, 1.0, 1.3, 1.0, 1.0], top_k=[0, 3, 0, 0, 0, 5, 0],
                top_p=[1.0, 1.0, 0.9, 1.0, 1.0, 1.0, 0.5])


@contextlib.contextmanager
def recording():
    """vqvae_amd._lib.call wrapped by a recorder that still calls through; yields the list of recorded names."""
    from vqvae_amd import _lib
    names, real = [], _lib.call

    def call(name, *args):
        if name.startswith(PREFIXES):
            names.append(name)
        return real(name, *args)

    _lib.call = call
    try:
        yield names
    finally:
        _lib.call = real


def rle(names):
    return [(k, len(list(g))) for k, g in itertools.groupby(names)]


def _host(res):
    """What a generate_* call returned as a list of host arrays."""
    return [a.get() if hasattr(a, 'get') else a for a in (res if isinstance(res, tuple) else (res,))]


@pytest.fixture(scope='module')
def decoders(gpu):
    return {'small': (dict(H.SMALL), _decoder(dict(H.SMALL), 140)[1]),
            'mol': (dict(H.MOL, input_dim=1), _decoder(dict(H.MOL, input_dim=1), 141, use_logistic=True)[1])}


def _step(gpu, decoders):
    from vqvae_amd.core import Variable
    cfg, dec = decoders['small']
    x = np.zeros((2, cfg['input_dim'], 1, 1), np.float32)
    x[0, 3] = x[1, 200] = 1
    dec.initialize(2)
    return dec.generate(Variable(gpu.to_device(x)), Variable(gpu.to_device(_cond(cfg, 2, 1, 60)[..., None]))).data


def _sequence(uniforms=None, **kw):
    def run(gpu, decoders):
        cfg, dec = decoders['small']
        u = np.random.RandomState(61).random_sample((T, 2)) if uniforms is None else uniforms()
        return dec.generate_sequence(gpu.to_device(_cond(cfg, 2, T, 62)), u, **kw)
    return run


def _device_uniforms():
    from vqvae_amd.generation import DeviceUniforms
    return DeviceUniforms(7)


def _batch(gpu, decoders):
    cfg, dec = decoders['small']
    return dec.generate_batch(gpu.to_device(_cond(cfg, 3, T, 63)), np.random.RandomState(64).random_sample((T, 3)), group=2)


def _lockstep(model='small', latent=False, device_uniforms=False, controls=False, refill=False, graph_steps=3):
    def run(gpu, decoders):
        cfg, dec = decoders[model]
        N = len(LENGTHS)
        if latent:
            cond = _latent(gpu, cfg, (3, 3, 2, 2, 1, 1, 1), 65, upscale=2)[0]
            assert cond.shape[2] == T
        else:
            cond = gpu.to_device(_cond(cfg, N, T, 66))
        if device_uniforms:
            u = _device_uniforms()
        elif model == 'mol':
            u = np.random.RandomState(67).uniform(0.02, 0.98, (T, N, cfg['out_dim'] // 3))
        else:
            u = np.random.RandomState(67).random_sample((T, N))
        return dec.generate_lockstep(cond, u, lengths=LENGTHS, group=5, graph_steps=graph_steps, refill=refill,
                                     **(CONTROLS if controls else {}))
    return run


CASES = {
    'generate': _step,
    'sequence-persistent': _sequence(persistent=True),
    'sequence-graph4-5steps': _sequence(persistent=False, graph_steps=4),
    'sequence-eager': _sequence(persistent=False, graph_steps=0),
    'sequence-temperature': _sequence(temperature=0.7),
    'sequence-device-uniforms': _sequence(uniforms=_device_uniforms),
    'batch-3-group2': _batch,
    'lockstep-mol': _lockstep(model='mol'),
    'lockstep-eager-sorted': _lockstep(graph_steps=0),
    'lockstep-eager-refill': _lockstep(graph_steps=0, refill=True),
}
for _lat, _du, _ctl, _ref in itertools.product((False, True), repeat=4):
    CASES['lockstep-%s-%s-%s-%s' % ('latent' if _lat else 'dense', 'rng' if _du else 'array', 'controls' if _ctl else 'plain',
                                    'refill' if _ref else 'sorted')] = _lockstep(latent=_lat, device_uniforms=_du,
                                                                                 controls=_ctl, refill=_ref)

EXPECTED = {
    'batch-3-group2': [('vqvae_wavenet_gen_run', 2)],
    'generate': [('vqvae_wavenet_gen_step', 1)],
    'lockstep-dense-array-controls-refill': [('vqvae_gen_slots_init', 1), ('vqvae_graph_capture_begin', 1),
        ('vqvae_wavenet_gen_step_slots', 3), ('vqvae_graph_capture_end', 1), ('vqvae_graph_launch', 2),
        ('vqvae_graph_destroy', 1)],
    'lockstep-dense-array-controls-sorted': [('vqvae_graph_capture_begin', 1), ('vqvae_wavenet_gen_step_sampled', 3),
        ('vqvae_graph_capture_end', 1), ('vqvae_graph_launch', 2), ('vqvae_graph_destroy', 1),
        ('vqvae_graph_capture_begin', 1), ('vqvae_wavenet_gen_step_sampled', 1), ('vqvae_graph_capture_end', 1),
        ('vqvae_graph_launch', 1), ('vqvae_graph_destroy', 1)],
    'lockstep-dense-array-plain-refill': [('vqvae_gen_slots_init', 1), ('vqvae_graph_capture_begin', 1),
        ('vqvae_wavenet_gen_step_slots', 3), ('vqvae_graph_capture_end', 1), ('vqvae_graph_launch', 2),
        ('vqvae_graph_destroy', 1)],
    'lockstep-dense-array-plain-sorted': [('vqvae_graph_capture_begin', 1), ('vqvae_wavenet_gen_step', 3),
        ('vqvae_graph_capture_end', 1), ('vqvae_graph_launch', 2), ('vqvae_graph_destroy', 1),
        ('vqvae_graph_capture_begin', 1), ('vqvae_wavenet_gen_step', 1), ('vqvae_graph_capture_end', 1),
        ('vqvae_graph_launch', 1), ('vqvae_graph_destroy', 1)],
    'lockstep-dense-rng-controls-refill': [('vqvae_gen_slots_init', 1), ('vqvae_graph_capture_begin', 1),
        ('vqvae_wavenet_gen_step_slots_rng', 3), ('vqvae_graph_capture_end', 1), ('vqvae_graph_launch', 2),
        ('vqvae_graph_destroy', 1)],
    'lockstep-dense-rng-controls-sorted': [('vqvae_graph_capture_begin', 1), ('vqvae_wavenet_gen_step_rng', 3),
        ('vqvae_graph_capture_end', 1), ('vqvae_graph_launch', 2), ('vqvae_graph_destroy', 1),
        ('vqvae_graph_capture_begin', 1), ('vqvae_wavenet_gen_step_rng', 1), ('vqvae_graph_capture_end', 1),
        ('vqvae_graph_launch', 1), ('vqvae_graph_destroy', 1)],
    'lockstep-dense-rng-plain-refill': [('vqvae_gen_slots_init', 1), ('vqvae_graph_capture_begin', 1),
        ('vqvae_wavenet_gen_step_slots_rng', 3), ('vqvae_graph_capture_end', 1), ('vqvae_graph_launch', 2),
        ('vqvae_graph_destroy', 1)],
    'lockstep-dense-rng-plain-sorted': [('vqvae_graph_capture_begin', 1), ('vqvae_wavenet_gen_step_rng', 3),
        ('vqvae_graph_capture_end', 1), ('vqvae_graph_launch', 2), ('vqvae_graph_destroy', 1),
        ('vqvae_graph_capture_begin', 1), ('vqvae_wavenet_gen_step_rng', 1), ('vqvae_graph_capture_end', 1),
        ('vqvae_graph_launch', 1), ('vqvae_graph_destroy', 1)],
    'lockstep-eager-refill': [('vqvae_gen_slots_init', 1), ('vqvae_wavenet_gen_step_slots', 5)],
    'lockstep-eager-sorted': [('vqvae_wavenet_gen_step', 6)],
    'lockstep-latent-array-controls-refill': [('vqvae_gen_slots_init', 1), ('vqvae_graph_capture_begin', 1),
        ('vqvae_gen_cond_column', 1), ('vqvae_wavenet_gen_step_slots', 1), ('vqvae_gen_cond_column', 1),
        ('vqvae_wavenet_gen_step_slots', 1), ('vqvae_gen_cond_column', 1), ('vqvae_wavenet_gen_step_slots', 1),
        ('vqvae_graph_capture_end', 1), ('vqvae_graph_launch', 2), ('vqvae_graph_destroy', 1)],
    'lockstep-latent-array-controls-sorted': [('vqvae_graph_capture_begin', 1), ('vqvae_gen_cond_column', 1),
        ('vqvae_wavenet_gen_step_sampled', 1), ('vqvae_gen_cond_column', 1), ('vqvae_wavenet_gen_step_sampled', 1),
        ('vqvae_gen_cond_column', 1), ('vqvae_wavenet_gen_step_sampled', 1), ('vqvae_graph_capture_end', 1),
        ('vqvae_graph_launch', 2), ('vqvae_graph_destroy', 1), ('vqvae_graph_capture_begin', 1),
        ('vqvae_gen_cond_column', 1), ('vqvae_wavenet_gen_step_sampled', 1), ('vqvae_graph_capture_end', 1),
        ('vqvae_graph_launch', 1), ('vqvae_graph_destroy', 1)],
    'lockstep-latent-array-plain-refill': [('vqvae_gen_slots_init', 1), ('vqvae_graph_capture_begin', 1),
        ('vqvae_gen_cond_column', 1), ('vqvae_wavenet_gen_step_slots', 1), ('vqvae_gen_cond_column', 1),
        ('vqvae_wavenet_gen_step_slots', 1), ('vqvae_gen_cond_column', 1), ('vqvae_wavenet_gen_step_slots', 1),
        ('vqvae_graph_capture_end', 1), ('vqvae_graph_launch', 2), ('vqvae_graph_destroy', 1)],
    'lockstep-latent-array-plain-sorted': [('vqvae_graph_capture_begin', 1), ('vqvae_gen_cond_column', 1),
        ('vqvae_wavenet_gen_step', 1), ('vqvae_gen_cond_column', 1), ('vqvae_wavenet_gen_step', 1),
        ('vqvae_gen_cond_column', 1), ('vqvae_wavenet_gen_step', 1), ('vqvae_graph_capture_end', 1),
        ('vqvae_graph_launch', 2), ('vqvae_graph_destroy', 1), ('vqvae_graph_capture_begin', 1),
        ('vqvae_gen_cond_column', 1), ('vqvae_wavenet_gen_step', 1), ('vqvae_graph_capture_end', 1),
        ('vqvae_graph_launch', 1), ('vqvae_graph_destroy', 1)],
    'lockstep-latent-rng-controls-refill': [('vqvae_gen_slots_init', 1), ('vqvae_graph_capture_begin', 1),
        ('vqvae_gen_cond_column', 1), ('vqvae_wavenet_gen_step_slots_rng', 1), ('vqvae_gen_cond_column', 1),
        ('vqvae_wavenet_gen_step_slots_rng', 1), ('vqvae_gen_cond_column', 1),
        ('vqvae_wavenet_gen_step_slots_rng', 1), ('vqvae_graph_capture_end', 1), ('vqvae_graph_launch', 2),
        ('vqvae_graph_destroy', 1)],
    'lockstep-latent-rng-controls-sorted': [('vqvae_graph_capture_begin', 1), ('vqvae_gen_cond_column', 1),
        ('vqvae_wavenet_gen_step_rng', 1), ('vqvae_gen_cond_column', 1), ('vqvae_wavenet_gen_step_rng', 1),
        ('vqvae_gen_cond_column', 1), ('vqvae_wavenet_gen_step_rng', 1), ('vqvae_graph_capture_end', 1),
        ('vqvae_graph_launch', 2), ('vqvae_graph_destroy', 1), ('vqvae_graph_capture_begin', 1),
        ('vqvae_gen_cond_column', 1), ('vqvae_wavenet_gen_step_rng', 1), ('vqvae_graph_capture_end', 1),
        ('vqvae_graph_launch', 1), ('vqvae_graph_destroy', 1)],
    'lockstep-latent-rng-plain-refill': [('vqvae_gen_slots_init', 1), ('vqvae_graph_capture_begin', 1),
        ('vqvae_gen_cond_column', 1), ('vqvae_wavenet_gen_step_slots_rng', 1), ('vqvae_gen_cond_column', 1),
        ('vqvae_wavenet_gen_step_slots_rng', 1), ('vqvae_gen_cond_column', 1),
        ('vqvae_wavenet_gen_step_slots_rng', 1), ('vqvae_graph_capture_end', 1), ('vqvae_graph_launch', 2),
        ('vqvae_graph_destroy', 1)],
    'lockstep-latent-rng-plain-sorted': [('vqvae_graph_capture_begin', 1), ('vqvae_gen_cond_column', 1),
        ('vqvae_wavenet_gen_step_rng', 1), ('vqvae_gen_cond_column', 1), ('vqvae_wavenet_gen_step_rng', 1),
        ('vqvae_gen_cond_column', 1), ('vqvae_wavenet_gen_step_rng', 1), ('vqvae_graph_capture_end', 1),
        ('vqvae_graph_launch', 2), ('vqvae_graph_destroy', 1), ('vqvae_graph_capture_begin', 1),
        ('vqvae_gen_cond_column', 1), ('vqvae_wavenet_gen_step_rng', 1), ('vqvae_graph_capture_end', 1),
        ('vqvae_graph_launch', 1), ('vqvae_graph_destroy', 1)],
    'lockstep-mol': [('vqvae_graph_capture_begin', 1), ('vqvae_wavenet_gen_step', 3), ('vqvae_graph_capture_end', 1),
        ('vqvae_graph_launch', 2), ('vqvae_graph_destroy', 1), ('vqvae_graph_capture_begin', 1),
        ('vqvae_wavenet_gen_step', 1), ('vqvae_graph_capture_end', 1), ('vqvae_graph_launch', 1),
        ('vqvae_graph_destroy', 1)],
    'sequence-device-uniforms': [('vqvae_gen_rng_fill', 1), ('vqvae_wavenet_gen_run', 1)],
    'sequence-eager': [('vqvae_wavenet_gen_step', 5)],
    'sequence-graph4-5steps': [('vqvae_graph_capture_begin', 1), ('vqvae_wavenet_gen_step', 4),
        ('vqvae_graph_capture_end', 1), ('vqvae_graph_launch', 2), ('vqvae_graph_destroy', 1)],
    'sequence-persistent': [('vqvae_wavenet_gen_run', 1)],
    'sequence-temperature': [('vqvae_graph_capture_begin', 1), ('vqvae_wavenet_gen_step_sampled', 5),
        ('vqvae_graph_capture_end', 1), ('vqvae_graph_launch', 1), ('vqvae_graph_destroy', 1)],
}


@pytest.mark.parametrize('case', sorted(CASES))
def test_generation_call_sequence(gpu, decoders, case):
    with recording() as names:
        first = _host(CASES[case](gpu, decoders))
    second = _host(CASES[case](gpu, decoders))
    assert rle(names) == EXPECTED[case]
    assert len(first) == len(second)
    for a, b in zip(first, second):
        assert a.shape == b.shape and a.dtype == b.dtype
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
