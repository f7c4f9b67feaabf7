"""Which C entry points the ragged-list calls issue, and in which order: the run-length-encoded sequence of EVERY name that
goes through `_lib.call` -- launches, uploads, copies back and `vqvae_copy_list` alike, since how many uploads a chunk
costs is part of what must not change -- behind encode_many, frontend_many, condition_many, ResidentCorpus.encode,
features_many, compare_many, LatentCondition.dense and synthesize_many, compared with a literal list.  Every chunked call
is cut into three chunks.  Left out is only what depends on what ran earlier in the process, not on the call: `vqvae_malloc`
and `vqvae_free` (whether a buffer is a new allocation or a block of the pool), and the `vqvae_stream_synchronize` of a stream
other than the main one (backend.synchronize() also waits for the side stream and the stream pool once an earlier test has
created them; the main stream's wait is recorded).  Each case runs once unrecorded first (the
table caches, the workspace and the pool are warm whatever ran before), then recorded, and both runs return the same bits.

The lists of EXPECTED were printed by this file's own recorder on the commit before corpus, front end, metrics and the
latent-rate condition were put on vqvae_amd.ragged; that change had to leave them as they were.

Last, the three ways a list of waves is staged (all host, all device, both) give the same bits."""
import contextlib
import itertools

import numpy as np
import pytest

import helpers as H
import vqvae_oracle as O
from vqvae_amd import metrics

pytestmark = pytest.mark.gpu

SKIPPED = ('vqvae_malloc', 'vqvae_free')
SIZES = (128, 64, 193, 300, 255)                     # latent lengths 2 1 3 4 3; 7 3 11 17 14 frames (one fewer sample: 6 2 11 17 14)
SPEAKERS = np.array([2, 5, 2, 0, 6], np.int32)
RUNS = [(0, 3), (3, 4), (4, 5)]
ENCODE_BYTES = 24576                                 # stage 1 (32 channels of 64 32 96 150 127 columns) is the largest: the first three fill it
CONDITION_BYTES = 768                                # 32 channels of 2 1 3 | 4 | 3 latent frames
FEATURE_BYTES = 700                                  # 8 mel rows of 7 3 11 | 17 | 14 frames
MAGNITUDE_BYTES = 1500                               # 17 bins of 7 3 11 | 17 | 14 frames
COMPARE_BYTES = 4000                                 # 2 (17 + 8) values of 6 2 11 | 17 | 14 frames


@contextlib.contextmanager
def recording():
    """vqvae_amd._lib.call wrapped by a recorder that still calls through; yields the list of recorded names."""
    from vqvae_amd import _lib, backend
    names, real = [], _lib.call

    def call(name, *args):
        if name not in SKIPPED and not (name == 'vqvae_stream_synchronize' and args[0] is not backend.stream()):
            names.append(name)
        return real(name, *args)

    _lib.call = call
    try:
        yield names
    finally:
        _lib.call = real


def rle(names):
    return [(k, len(list(g))) for k, g in itertools.groupby(names)]


class Model(object):
    pass


@pytest.fixture(scope='module')
def model(gpu):
    """Built once and left unchanged: the small model, the five waves, the corpus of them and their codes and condition."""
    import vqvae_amd as V
    from vqvae_amd.metrics import MelConfig
    m = Model()
    cfg = dict(H.SMALL)
    _, net = H.build_model(cfg, seed=145)
    net.to_gpu()
    m.enc, m.vq, m.dec, m.ce = net.encoder, net.vq, net.decoder, net.condition_embed
    m.waves = [O.synth_batch(1, length=L - 1, n_speaker=cfg['n_speaker'], seed=16 + i)[0].reshape(-1).copy() for i, L in enumerate(SIZES)]
    for w in m.waves:
        w.setflags(write=False)
    m.shorter = [w[:-1] for w in m.waves]
    m.cfg = MelConfig(n_fft=32, hop=16, n_mels=8, n_mcep=4)
    m.corpus = V.ResidentCorpus(m.waves, SPEAKERS)
    m.cond, m.codes = V.frontend_many(m.enc, m.vq, m.ce, m.waves, SPEAKERS, return_codes=True)
    d = cfg['d']
    assert V.plan_chunks(SIZES, [1] + [d] * 6, ENCODE_BYTES) == RUNS and V.plan_chunks(m.codes.tl, [d], CONDITION_BYTES) == RUNS
    frames = metrics.frame_count(np.array(SIZES), m.cfg)
    assert metrics.plan_chunks(frames, m.cfg.n_mels, FEATURE_BYTES) == metrics.plan_chunks(frames, m.cfg.nb, MAGNITUDE_BYTES) == RUNS
    assert metrics.plan_chunks(metrics.frame_count(np.array(SIZES) - 1, m.cfg), 2 * (m.cfg.nb + m.cfg.n_mels), COMPARE_BYTES) == RUNS
    return m


def _codes(codes):
    return codes.to_host()


def _condition(cond):
    return [cond.tl, cond.local.get(), cond.global_vec.get()]


def _features(feats):
    return [feats.frames, feats.log_mel.get()] + ([] if feats.mag is None else [feats.mag.get()])


def _synthesize(**kw):
    def run(V, m):
        res = V.synthesize_many(m.enc, m.vq, m.dec, m.ce, m.waves, SPEAKERS, rng=np.random.RandomState(5), n_steps=4, group=5,
                                return_output=True, **kw)
        return [np.asarray(a) for pair in res for a in pair]
    return run


CASES = {
    'encode_many': lambda V, m: _codes(V.encode_many(m.enc, m.vq, m.waves, chunk_bytes=ENCODE_BYTES)),
    'frontend_many': lambda V, m: _condition(V.frontend_many(m.enc, m.vq, m.ce, m.waves, SPEAKERS, chunk_bytes=ENCODE_BYTES)),
    'condition_many': lambda V, m: _condition(V.condition_many(m.vq, m.ce, m.codes, SPEAKERS, chunk_bytes=CONDITION_BYTES)),
    'corpus-encode': lambda V, m: _codes(m.corpus.encode(m.enc, m.vq, chunk_bytes=ENCODE_BYTES)),
    'features_many-list': lambda V, m: _features(V.features_many(m.waves, m.cfg, chunk_bytes=FEATURE_BYTES)),
    'features_many-corpus': lambda V, m: _features(V.features_many(m.corpus, m.cfg, chunk_bytes=FEATURE_BYTES)),
    'compare_many': lambda V, m: [v for _, v in sorted(V.compare_many(m.waves, m.shorter, m.cfg, chunk_bytes=COMPARE_BYTES).items())],
    'dense-unequal': lambda V, m: [m.cond.dense().get()],
    'synthesize_many-dense': _synthesize(),
    'synthesize_many-latent': _synthesize(latent_condition=True),
    'synthesize_many-batched': _synthesize(latent_condition=True, batched_frontend=True),
}

EXPECTED = {
    'compare_many': [('vqvae_memcpy_h2d', 5), ('vqvae_metrics_stft_mel', 1), ('vqvae_memcpy_h2d', 2),
        ('vqvae_metrics_stft_mel', 1), ('vqvae_metrics_distances', 1), ('vqvae_memcpy_h2d', 2),
        ('vqvae_metrics_stft_mel', 1), ('vqvae_memcpy_h2d', 2), ('vqvae_metrics_stft_mel', 1),
        ('vqvae_metrics_distances', 1), ('vqvae_memcpy_h2d', 2), ('vqvae_metrics_stft_mel', 1), ('vqvae_memcpy_h2d', 2),
        ('vqvae_metrics_stft_mel', 1), ('vqvae_metrics_distances', 1), ('vqvae_memcpy_d2h', 1)],
    'condition_many': [('vqvae_memcpy_h2d', 1), ('vqvae_ragged_code_gather', 1), ('vqvae_ragged_conv_fwd', 5),
        ('vqvae_memcpy_h2d', 1), ('vqvae_ragged_code_gather', 1), ('vqvae_ragged_conv_fwd', 5), ('vqvae_memcpy_h2d', 1),
        ('vqvae_ragged_code_gather', 1), ('vqvae_ragged_conv_fwd', 5), ('vqvae_memcpy_h2d', 1),
        ('vqvae_ragged_speaker_gather', 1), ('vqvae_memcpy_d2h', 2)],
    'corpus-encode': [('vqvae_memcpy_h2d', 1), ('vqvae_ragged_conv_fwd', 6), ('vqvae_vq_nearest_fwd', 1),
        ('vqvae_memcpy_h2d', 1), ('vqvae_ragged_conv_fwd', 6), ('vqvae_vq_nearest_fwd', 1), ('vqvae_memcpy_h2d', 1),
        ('vqvae_ragged_conv_fwd', 6), ('vqvae_vq_nearest_fwd', 1), ('vqvae_memcpy_d2h', 1)],
    'dense-unequal': [('vqvae_memcpy_h2d', 1), ('vqvae_memset', 1), ('vqvae_upsample_linear_fwd', 1),
        ('vqvae_embed_broadcast_fwd', 1), ('vqvae_upsample_linear_fwd', 1), ('vqvae_embed_broadcast_fwd', 1),
        ('vqvae_upsample_linear_fwd', 1), ('vqvae_embed_broadcast_fwd', 1), ('vqvae_upsample_linear_fwd', 1),
        ('vqvae_embed_broadcast_fwd', 1), ('vqvae_upsample_linear_fwd', 1), ('vqvae_embed_broadcast_fwd', 1),
        ('vqvae_copy_list', 1), ('vqvae_stream_synchronize', 1), ('vqvae_memcpy_d2h', 1)],
    'encode_many': [('vqvae_memcpy_h2d', 2), ('vqvae_ragged_conv_fwd', 6), ('vqvae_vq_nearest_fwd', 1),
        ('vqvae_memcpy_h2d', 2), ('vqvae_ragged_conv_fwd', 6), ('vqvae_vq_nearest_fwd', 1), ('vqvae_memcpy_h2d', 2),
        ('vqvae_ragged_conv_fwd', 6), ('vqvae_vq_nearest_fwd', 1), ('vqvae_memcpy_d2h', 1)],
    'features_many-corpus': [('vqvae_memcpy_h2d', 3), ('vqvae_metrics_stft_mel', 1), ('vqvae_memcpy_h2d', 1),
        ('vqvae_metrics_stft_mel', 1), ('vqvae_memcpy_h2d', 1), ('vqvae_metrics_stft_mel', 1), ('vqvae_memcpy_d2h', 1)],
    'features_many-list': [('vqvae_memcpy_h2d', 4), ('vqvae_metrics_stft_mel', 1), ('vqvae_memcpy_h2d', 2),
        ('vqvae_metrics_stft_mel', 1), ('vqvae_memcpy_h2d', 2), ('vqvae_metrics_stft_mel', 1), ('vqvae_memcpy_d2h', 1)],
    'frontend_many': [('vqvae_memcpy_h2d', 2), ('vqvae_ragged_conv_fwd', 6), ('vqvae_vq_nearest_fwd', 1),
        ('vqvae_ragged_conv_fwd', 5), ('vqvae_memcpy_h2d', 2), ('vqvae_ragged_conv_fwd', 6),
        ('vqvae_vq_nearest_fwd', 1), ('vqvae_ragged_conv_fwd', 5), ('vqvae_memcpy_h2d', 2),
        ('vqvae_ragged_conv_fwd', 6), ('vqvae_vq_nearest_fwd', 1), ('vqvae_ragged_conv_fwd', 5),
        ('vqvae_memcpy_h2d', 1), ('vqvae_ragged_speaker_gather', 1), ('vqvae_memcpy_d2h', 2)],
    'synthesize_many-batched': [('vqvae_memcpy_h2d', 2), ('vqvae_ragged_conv_fwd', 6), ('vqvae_vq_nearest_fwd', 1),
        ('vqvae_ragged_conv_fwd', 5), ('vqvae_memcpy_h2d', 1), ('vqvae_ragged_speaker_gather', 1), ('vqvae_memset', 15),
        ('vqvae_memcpy_h2d', 3), ('vqvae_memset', 5), ('vqvae_memcpy_h2d', 1), ('vqvae_memset', 1),
        ('vqvae_memcpy_h2d', 2), ('vqvae_gen_slots_init', 1), ('vqvae_graph_capture_begin', 1),
        ('vqvae_gen_cond_column', 1), ('vqvae_wavenet_gen_step_slots', 1), ('vqvae_gen_cond_column', 1),
        ('vqvae_wavenet_gen_step_slots', 1), ('vqvae_gen_cond_column', 1), ('vqvae_wavenet_gen_step_slots', 1),
        ('vqvae_gen_cond_column', 1), ('vqvae_wavenet_gen_step_slots', 1), ('vqvae_graph_capture_end', 1),
        ('vqvae_graph_launch', 1), ('vqvae_stream_synchronize', 1), ('vqvae_memcpy_d2h', 1),
        ('vqvae_stream_synchronize', 1), ('vqvae_graph_destroy', 1)],
    'synthesize_many-dense': [('vqvae_memcpy_h2d', 1), ('vqvae_conv1d_fwd', 6), ('vqvae_vq_nearest_fwd', 1),
        ('vqvae_memcpy_h2d', 1), ('vqvae_convstack_fwd', 1), ('vqvae_upsample_linear_fwd', 1),
        ('vqvae_embed_broadcast_fwd', 1), ('vqvae_upsample_linear_fwd', 1), ('vqvae_embed_broadcast_fwd', 1),
        ('vqvae_memcpy_h2d', 1), ('vqvae_conv1d_fwd', 6), ('vqvae_vq_nearest_fwd', 1), ('vqvae_memcpy_h2d', 1),
        ('vqvae_convstack_fwd', 1), ('vqvae_upsample_linear_fwd', 1), ('vqvae_embed_broadcast_fwd', 1),
        ('vqvae_memcpy_h2d', 1), ('vqvae_conv1d_fwd', 6), ('vqvae_vq_nearest_fwd', 1), ('vqvae_memcpy_h2d', 1),
        ('vqvae_convstack_fwd', 1), ('vqvae_upsample_linear_fwd', 1), ('vqvae_embed_broadcast_fwd', 1),
        ('vqvae_upsample_linear_fwd', 1), ('vqvae_embed_broadcast_fwd', 1), ('vqvae_memcpy_h2d', 1),
        ('vqvae_conv1d_fwd', 6), ('vqvae_vq_nearest_fwd', 1), ('vqvae_memcpy_h2d', 1), ('vqvae_convstack_fwd', 1),
        ('vqvae_upsample_linear_fwd', 1), ('vqvae_embed_broadcast_fwd', 1), ('vqvae_upsample_linear_fwd', 1),
        ('vqvae_embed_broadcast_fwd', 1), ('vqvae_memcpy_h2d', 1), ('vqvae_conv1d_fwd', 6), ('vqvae_vq_nearest_fwd', 1),
        ('vqvae_memcpy_h2d', 1), ('vqvae_convstack_fwd', 1), ('vqvae_upsample_linear_fwd', 1),
        ('vqvae_embed_broadcast_fwd', 1), ('vqvae_upsample_linear_fwd', 1), ('vqvae_embed_broadcast_fwd', 1),
        ('vqvae_memset', 1), ('vqvae_copy_list', 1), ('vqvae_memset', 15), ('vqvae_memcpy_h2d', 3), ('vqvae_memset', 5),
        ('vqvae_memcpy_h2d', 1), ('vqvae_gen_slots_init', 1), ('vqvae_graph_capture_begin', 1),
        ('vqvae_wavenet_gen_step_slots', 4), ('vqvae_graph_capture_end', 1), ('vqvae_graph_launch', 1),
        ('vqvae_stream_synchronize', 1), ('vqvae_memcpy_d2h', 1), ('vqvae_stream_synchronize', 1),
        ('vqvae_graph_destroy', 1)],
    'synthesize_many-latent': [('vqvae_memcpy_h2d', 1), ('vqvae_conv1d_fwd', 6), ('vqvae_vq_nearest_fwd', 1),
        ('vqvae_memcpy_h2d', 1), ('vqvae_convstack_fwd', 1), ('vqvae_upsample_linear_fwd', 1),
        ('vqvae_embed_broadcast_fwd', 1), ('vqvae_memcpy2d_d2d', 2), ('vqvae_memcpy_h2d', 1), ('vqvae_conv1d_fwd', 6),
        ('vqvae_vq_nearest_fwd', 1), ('vqvae_memcpy_h2d', 1), ('vqvae_convstack_fwd', 1),
        ('vqvae_upsample_linear_fwd', 1), ('vqvae_embed_broadcast_fwd', 1), ('vqvae_memcpy2d_d2d', 2),
        ('vqvae_memcpy_h2d', 1), ('vqvae_conv1d_fwd', 6), ('vqvae_vq_nearest_fwd', 1), ('vqvae_memcpy_h2d', 1),
        ('vqvae_convstack_fwd', 1), ('vqvae_upsample_linear_fwd', 1), ('vqvae_embed_broadcast_fwd', 1),
        ('vqvae_memcpy2d_d2d', 2), ('vqvae_memcpy_h2d', 1), ('vqvae_conv1d_fwd', 6), ('vqvae_vq_nearest_fwd', 1),
        ('vqvae_memcpy_h2d', 1), ('vqvae_convstack_fwd', 1), ('vqvae_upsample_linear_fwd', 1),
        ('vqvae_embed_broadcast_fwd', 1), ('vqvae_memcpy2d_d2d', 2), ('vqvae_memcpy_h2d', 1), ('vqvae_conv1d_fwd', 6),
        ('vqvae_vq_nearest_fwd', 1), ('vqvae_memcpy_h2d', 1), ('vqvae_convstack_fwd', 1),
        ('vqvae_upsample_linear_fwd', 1), ('vqvae_embed_broadcast_fwd', 1), ('vqvae_memcpy2d_d2d', 2),
        ('vqvae_copy_list', 1), ('vqvae_memset', 15), ('vqvae_memcpy_h2d', 3), ('vqvae_memset', 5),
        ('vqvae_memcpy_h2d', 1), ('vqvae_memset', 1), ('vqvae_memcpy_h2d', 2), ('vqvae_gen_slots_init', 1),
        ('vqvae_graph_capture_begin', 1), ('vqvae_gen_cond_column', 1), ('vqvae_wavenet_gen_step_slots', 1),
        ('vqvae_gen_cond_column', 1), ('vqvae_wavenet_gen_step_slots', 1), ('vqvae_gen_cond_column', 1),
        ('vqvae_wavenet_gen_step_slots', 1), ('vqvae_gen_cond_column', 1), ('vqvae_wavenet_gen_step_slots', 1),
        ('vqvae_graph_capture_end', 1), ('vqvae_graph_launch', 1), ('vqvae_stream_synchronize', 1),
        ('vqvae_memcpy_d2h', 1), ('vqvae_stream_synchronize', 1), ('vqvae_graph_destroy', 1)],
}


@pytest.mark.parametrize('case', sorted(CASES))
def test_ragged_call_sequence(gpu, model, case):
    import vqvae_amd as V
    first = CASES[case](V, model)
    with recording() as names:
        second = CASES[case](V, model)
    print('%r: %r,' % (case, rle(names)))
    assert rle(names) == EXPECTED[case]
    assert len(first) == len(second)
    for a, b in zip(first, second):
        H._same(a, b, case)


@pytest.mark.parametrize('call', ['encode_many', 'features_many'])
def test_the_three_ways_of_staging_give_the_same_bits(gpu, model, call):
    import vqvae_amd as V
    m = model

    def run(waves):
        if call == 'encode_many':
            codes, z = V.encode_many(m.enc, m.vq, waves, chunk_bytes=ENCODE_BYTES, return_latents=True)
            return _codes(codes) + z
        return _features(V.features_many(waves, m.cfg, magnitudes=True, chunk_bytes=MAGNITUDE_BYTES))

    host = run(m.waves)
    on_device = [gpu.to_device(w) for w in m.waves]
    for what, waves in (('all device', on_device), ('host and device', [d if i % 2 else w for i, (w, d) in enumerate(zip(m.waves, on_device))])):
        got = run(waves)
        assert len(got) == len(host)
        for a, b in zip(got, host):
            H._same(a, b, '%s, %s' % (call, what))
