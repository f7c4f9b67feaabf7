"""CPU checks of the uniforms of generation drawn on the device (include/vqvae_gen_rng.h, csrc/gen_rng.hip,
vqvae_amd.DeviceUniforms): the generator's two known answers on the independent restatement (tests/gen_rng_ref.py) and on
the package's NumPy form, their agreement, the double construction, stream independence, argument errors, the wiring of
run_lockstep / run_lockstep_refill on stubs in place of the device, the header against the table Python binds, the entry
points' validation, and the compiled kernels' resources.  Every comparison is an equality."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import gen_rng_ref as R
import vqvae_amd
from vqvae_amd import _lib
from vqvae_amd.generation import (DeviceUniforms, LatentCondition, philox4x32_10, run_lockstep, run_lockstep_refill,
                                  words_to_double)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'vqvae_gen_rng.h')
IDS = [0, 5, 2 ** 40 + 3, 2 ** 64 - 1]
SEED = 0x9E3779B97F4A7C15


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the generator ------------------------------------------------------------------------------------------------------
def test_known_answers_on_the_restatement_and_on_the_package():
    for counter, key, want in R.KNOWN_ANSWERS:
        assert R.block(counter, key) == want
        got = philox4x32_10(np.array(counter, np.uint64), np.array(key, np.uint64))
        assert got.dtype == np.uint32 and tuple(int(w) for w in got) == want
    both = philox4x32_10(np.array([k[0] for k in R.KNOWN_ANSWERS], np.uint64), np.array([k[1] for k in R.KNOWN_ANSWERS], np.uint64))
    assert [tuple(int(w) for w in row) for row in both] == [k[2] for k in R.KNOWN_ANSWERS]      # vectorised over blocks


def test_known_answers_in_the_header_are_the_restatements():
    text = open(HEADER).read()
    for counter, key, want in R.KNOWN_ANSWERS:
        line = '%s ; %s -> %s' % (' '.join('%08x' % c for c in counter), ' '.join('%08x' % k for k in key),
                                  ' '.join('%08x' % w for w in want))
        assert line in text, line


@pytest.mark.parametrize('n_uniform', [1, 3, 10])
def test_host_form_is_the_restatement(n_uniform):
    want = R.uniforms(SEED, IDS, 7, n_uniform)
    got = DeviceUniforms(SEED, IDS).host(7, n_uniform)
    assert got.shape == (7, 4, n_uniform) and got.dtype == np.float64
    np.testing.assert_array_equal(_bits(got), _bits(want))
    assert (got >= 0).all() and (got < 1).all() and (want >= 0).all() and (want < 1).all()
    np.testing.assert_array_equal(_bits(DeviceUniforms(SEED).host(7, n_uniform, ids=IDS)), _bits(want))
    later = DeviceUniforms(SEED, IDS).host(7, n_uniform, t0=5)                       # steps 5..11, as the fill kernel is asked
    np.testing.assert_array_equal(_bits(later), _bits(R.uniforms(SEED, IDS, 7, n_uniform, t0=5)))
    np.testing.assert_array_equal(_bits(later[:2]), _bits(got[5:]))
    # the counter and the key are what the header says: uniform (id, t, j) from the raw words
    for (t, q, j) in ((0, 0, 0), (6, 2, n_uniform - 1), (3, 3, n_uniform // 2)):
        sid = IDS[q]
        w = R.block((t, j >> 1, sid & 0xFFFFFFFF, sid >> 32), (SEED & 0xFFFFFFFF, SEED >> 32))
        assert got[t, q, j] == R.to_double(w[2 * (j & 1)], w[2 * (j & 1) + 1])


def test_double_construction_on_hand_picked_words():
    for fn in (R.to_double, lambda a, b: float(words_to_double(a, b))):
        assert fn(0, 0) == 0.0
        assert fn(0xFFFFFFFF, 0xFFFFFFFF) == 1.0 - 2.0 ** -53
        assert fn(1 << 5, 0) == 2.0 ** -27 and fn(0, 1 << 6) == 2.0 ** -53
        assert fn(31, 63) == 0.0                                                   # the discarded low bits
    a = np.array([0, 0xFFFFFFFF, 0x80000000], np.uint32)
    np.testing.assert_array_equal(words_to_double(a, a), [R.to_double(int(x), int(x)) for x in a])


def test_streams_do_not_depend_on_their_neighbours_or_on_the_number_of_steps():
    g = DeviceUniforms(7)
    for n_uniform in (1, 3):
        three = g.host(9, n_uniform, ids=[3, 5, 9])
        np.testing.assert_array_equal(_bits(g.host(9, n_uniform, ids=[5])[:, 0]), _bits(three[:, 1]))
        np.testing.assert_array_equal(_bits(g.host(4, n_uniform, ids=[3, 5, 9])), _bits(three[:4]))
        np.testing.assert_array_equal(_bits(g.host(20, n_uniform, ids=[3, 5, 9])[:9]), _bits(three))
        wide = g.host(9, 10, ids=[3, 5, 9])                                         # and not on how many uniforms a step takes
        np.testing.assert_array_equal(_bits(wide[:, :, :n_uniform]), _bits(three))
    assert not np.array_equal(DeviceUniforms(8).host(9, ids=[3]), g.host(9, ids=[3]))
    dup = g.host(5, ids=[4, 4])                                                     # duplicates share a stream
    np.testing.assert_array_equal(_bits(dup[:, 0]), _bits(dup[:, 1]))


# ---- argument errors ----------------------------------------------------------------------------------------------------
def test_argument_errors_name_the_caller():
    assert vqvae_amd.DeviceUniforms is DeviceUniforms
    for seed in (-1, 2 ** 64):
        with pytest.raises(ValueError, match='DeviceUniforms: seed'):
            DeviceUniforms(seed)
    for seed in (1.5, '3', None, True):
        with pytest.raises(TypeError, match='DeviceUniforms: seed'):
            DeviceUniforms(seed)
    assert DeviceUniforms(2 ** 64 - 1).seed == 2 ** 64 - 1 and DeviceUniforms(np.int64(3)).seed == 3
    for ids in ([0, -1], [0, 2 ** 64], np.array([-5, 2])):
        with pytest.raises(ValueError, match='DeviceUniforms: stream_ids'):
            DeviceUniforms(1, ids)
    for ids in ([0.5, 1.0], ['a']):
        with pytest.raises(TypeError, match='DeviceUniforms: stream_ids'):
            DeviceUniforms(1, ids)
    for ids in (3, [[0, 1], [2, 3]]):
        with pytest.raises(ValueError, match=r'DeviceUniforms: stream_ids must be \(N,\)'):
            DeviceUniforms(1, ids)
    assert DeviceUniforms(1, IDS).stream_ids.dtype == np.uint64 and DeviceUniforms(1, IDS).stream_ids.tolist() == IDS
    with pytest.raises(ValueError, match='DeviceUniforms.host'):
        DeviceUniforms(1).host(3)                                                   # N is not known
    with pytest.raises(ValueError, match='DeviceUniforms.host'):
        DeviceUniforms(1, [0]).host(3, n_uniform=0)
    with pytest.raises(ValueError, match='DeviceUniforms.host: ids'):
        DeviceUniforms(1).host(3, ids=[-1])
    # a count that differs from N, before anything needs a device
    lc = LatentCondition([2, 2, 1, 2, 1, 2], 2, 1, 4)
    g3 = DeviceUniforms(1, [0, 1, 2])
    with pytest.raises(ValueError, match='generate_lockstep: the DeviceUniforms has 3 stream_ids for 6 sequences'):
        run_lockstep(_StubNet(), lc, g3, _lib.GEN_SOFTMAX, _run_group=lambda *a: None)
    with pytest.raises(ValueError, match='generate_lockstep: the DeviceUniforms has 3 stream_ids for 6 sequences'):
        run_lockstep_refill(_StubNet(), lc, g3, _lib.GEN_SOFTMAX, _run=lambda *a: None)
    with pytest.raises(ValueError, match='sample_logits'):
        g3.ids_for(6, 'sample_logits')


def test_generate_batch_refuses_the_object_by_name():
    from vqvae_amd.wavenet import WaveNet
    dec = WaveNet(1, 2, 2, 16, 8, 8, 8, 256, False, 16, -40, 8, 0)
    cond = np.zeros((2, 16, 8), np.float32)
    with pytest.raises(TypeError, match='generate_batch') as e:
        dec.generate_batch(cond, DeviceUniforms(3))
    assert 'generate_lockstep' in str(e.value)
    with pytest.raises(ValueError, match='generate_lockstep'):                      # the controls as before
        dec.generate_batch(cond, np.zeros((8, 2)), temperature=0.5)


def test_rng_is_an_argument_of_the_synthesis_calls_and_its_default_stands():
    import inspect
    for fn in (vqvae_amd.synthesize, vqvae_amd.synthesize_many):
        p = inspect.signature(fn).parameters
        assert p['rng'].default is None and p['latent_condition'].default is False
        assert 'DeviceUniforms' in fn.__doc__
    assert inspect.signature(vqvae_amd.generation.sample_logits).parameters['step'].default == 0


# ---- the runners around stubs -------------------------------------------------------------------------------------------
class _StubNet(object):
    class proj2(object):
        class W(object):
            shape = (8, 4)


def test_stubbed_runners_get_the_generator_with_the_groups_ids():
    tl = np.array([3, 1, 2, 3, 1, 2, 2, 1, 3, 1, 2, 1, 3])
    lc = LatentCondition(tl, 2, 1, 4)
    N, Cc, T = lc.shape
    ids = (np.arange(N)[::-1] * 1000 + 2 ** 40).astype(np.uint64)

    for given, want_ids in ((DeviceUniforms(11, ids), ids), (DeviceUniforms(11), np.arange(N, dtype=np.uint64))):
        calls = []

        def stub(idx, ug, fg, gsteps, sampling=None):
            calls.append((np.array(idx).tolist(), ug, fg, gsteps))
            return np.zeros((len(idx), T), np.int32), None
        run_lockstep(_StubNet(), lc, given, _lib.GEN_SOFTMAX, group=5, _run_group=stub)
        assert [c[0] for c in calls] == [[0, 3, 8, 12, 2], [5, 6, 10, 1, 4], [7, 9, 11, 11, 11]]
        for idx, ug, fg, gsteps in calls:
            assert isinstance(ug, DeviceUniforms) and not isinstance(ug, np.ndarray) and ug.seed == 11 and fg is None
            assert ug.stream_ids.dtype == np.uint64 and ug.stream_ids.tolist() == want_ids[idx].tolist()   # repeats included

        seen = []

        def stub_refill(steps, ug, fg, sampling):
            seen.append((np.array(steps).tolist(), ug, fg, sampling))
            return np.zeros((N, T), np.int32), None
        run_lockstep_refill(_StubNet(), lc, given, _lib.GEN_SOFTMAX, group=5, _run=stub_refill)
        (steps, ug, fg, sampling), = seen
        assert steps == (lc.lengths - 1).tolist() and fg is None and sampling is None
        assert isinstance(ug, DeviceUniforms) and ug.seed == 11 and ug.stream_ids.tolist() == want_ids.tolist()

    # the controls still travel with the group, and an array still arrives as an array
    calls = []

    def stub2(idx, ug, fg, gsteps, sampling=None):
        calls.append((ug, sampling))
        return np.zeros((len(idx), T), np.int32), None
    temp = (np.arange(N, dtype=np.float32) + 1, None, None)
    run_lockstep(_StubNet(), lc, DeviceUniforms(2), _lib.GEN_SOFTMAX, group=5, _run_group=stub2, sampling=temp)
    assert calls[0][1][0].tolist() == [1, 4, 9, 13, 3] and isinstance(calls[0][0], DeviceUniforms)
    calls = []
    run_lockstep(_StubNet(), lc, np.zeros((T, N)), _lib.GEN_SOFTMAX, group=5, _run_group=stub2)
    assert isinstance(calls[0][0], np.ndarray) and calls[0][0].shape == (11, 5, 1)


# ---- the header, the table, the library ---------------------------------------------------------------------------------
NAMES = {'vqvae_gen_rng_abi_version', 'vqvae_gen_rng_fill', 'vqvae_sample_logits_rng', 'vqvae_wavenet_gen_step_rng',
         'vqvae_wavenet_gen_step_slots_rng'}


def test_header_exports_are_the_bound_table_and_versions_stand():
    """The header, the library, the versions and vqvae_gen_rng's layout: tests/test_host_abi.py, for every header."""
    assert set(_lib.HEADERS['vqvae_gen_rng.h'].prototypes) == NAMES
    assert [f[0] for f in _lib.GenRng._fields_] == ['seed', 'ids'] and _lib.GenRng._fields_[0][1] is C.c_uint64
    assert 'gen_rng.hip' in open(os.path.join(ROOT, 'chainer-vq-vae_amd', 'csrc', 'Makefile')).read()


def test_c_side_validation_needs_no_device():
    lib = _lib.load()
    fake = 0x10000                                                      # never dereferenced: every call below is rejected first
    rng = _lib.GenRng()
    rng.seed, rng.ids = 5, None

    def rejected(what, rc):
        assert rc == -1, what
        assert what.encode() in lib.vqvae_last_error_string(), (what, lib.vqvae_last_error_string())

    fill = lib.vqvae_gen_rng_fill
    rejected('gen_rng_fill: null rng or out', fill(None, 0, 4, 3, 1, fake, None))
    rejected('gen_rng_fill: null rng or out', fill(C.byref(rng), 0, 4, 3, 1, None, None))
    rejected('gen_rng_fill: n must be at least 1', fill(C.byref(rng), 0, 4, 0, 1, fake, None))
    rejected('gen_rng_fill: n_uniform must be at least 1', fill(C.byref(rng), 0, 4, 3, 0, fake, None))
    rejected('gen_rng_fill: steps', fill(C.byref(rng), -1, 4, 3, 1, fake, None))
    rejected('gen_rng_fill: steps', fill(C.byref(rng), 0, -4, 3, 1, fake, None))
    rejected('gen_rng_fill: steps', fill(C.byref(rng), 2 ** 31 - 2, 4, 3, 1, fake, None))
    assert fill(C.byref(rng), 3, 0, 3, 1, fake, None) == 0                          # nothing to do, nothing launched

    smp = lib.vqvae_sample_logits_rng
    S, M = _lib.GEN_SOFTMAX, _lib.GEN_MOL
    rejected('sample_logits_rng: null logits, rng or out', smp(None, 6, 256, S, -40.0, C.byref(rng), 0, 1, None, fake, None, None))
    rejected('sample_logits_rng: null logits, rng or out', smp(fake, 6, 256, S, -40.0, None, 0, 1, None, fake, None, None))
    rejected('sample_logits_rng: null logits, rng or out', smp(fake, 6, 256, S, -40.0, C.byref(rng), 0, 1, None, None, None, None))
    rejected('sample_logits_rng: n must be', smp(fake, 0, 256, S, -40.0, C.byref(rng), 0, 1, None, fake, None, None))
    rejected('sample_logits_rng: step', smp(fake, 6, 256, S, -40.0, C.byref(rng), -1, 1, None, fake, None, None))
    rejected('sample_logits_rng: out_dim', smp(fake, 6, 1025, S, -40.0, C.byref(rng), 0, 1, None, fake, None, None))
    rejected('sample_logits_rng: mode', smp(fake, 6, 256, 0, -40.0, C.byref(rng), 0, 1, None, fake, None, None))
    rejected('sample_logits_rng: n_uniform', smp(fake, 6, 256, S, -40.0, C.byref(rng), 0, 0, None, fake, None, None))
    rejected('sample_logits_rng: mixture sampling', smp(fake, 6, 30, M, -40.0, C.byref(rng), 0, 9, None, fake, None, None))
    rejected('sample_logits_rng: mixture sampling', smp(fake, 6, 31, M, -40.0, C.byref(rng), 0, 10, None, fake, None, None))
    ctl = _lib.GenSampling()
    ctl.top_k = fake
    rejected('sample_logits_rng: the mixture of logistics', smp(fake, 6, 30, M, -40.0, C.byref(rng), 0, 10, C.byref(ctl), fake, None, None))
    rejected('sample_logits_rng: probs_out', smp(fake, 6, 30, M, -40.0, C.byref(rng), 0, 10, None, fake, fake, None))

    blocks = (_lib.GenBlock * 1)()
    d = _lib.GenDesc()
    d.n, d.n_blocks, d.blocks = 6, 1, blocks
    d.input_dim, d.residual, d.dilated, d.skip, d.cond_dim, d.out_dim = 16, 8, 16, 8, 0, 30
    for name in ('embed_W', 'embed_b', 'proj1_W', 'proj1_b', 'proj2_W', 'proj2_b', 'step', 'x_cur', 'x_prev', 'h0', 'h1', 'z',
                 'skip_acc', 's1', 'logits', 'out'):
        setattr(d, name, fake)
    d.sample_mode, d.n_uniform, d.uniforms, d.max_steps = M, 10, None, 4
    step = lib.vqvae_wavenet_gen_step_rng
    rejected('gen_step_rng: null rng', step(C.byref(d), None, None, None))
    rejected('gen_step: null descriptor', step(None, None, C.byref(rng), None))
    d.n_uniform = 9
    rejected('mixture sampling needs out_dim = 3*nr_mix and nr_mix uniforms', step(C.byref(d), None, C.byref(rng), None))
    d.n_uniform = 0
    rejected('sampling needs uniforms', step(C.byref(d), None, C.byref(rng), None))
    d.n_uniform = 10
    d.n = 4
    rejected('gen_step_rng: d->n must be 5..128', step(C.byref(d), None, C.byref(rng), None))
    d.n = 6
    d.sample_mode = _lib.GEN_NONE
    rejected('gen_step_rng: sample_mode VQVAE_GEN_NONE', step(C.byref(d), None, C.byref(rng), None))
    d.sample_mode = M
    rejected('gen_step_rng: the mixture of logistics', step(C.byref(d), C.byref(ctl), C.byref(rng), None))
    rejected('block 0 incomplete', step(C.byref(d), None, C.byref(rng), None))     # null uniforms were not the obstacle
    assert lib.vqvae_wavenet_gen_step(C.byref(d), None) == -1                       # ... and still are for the array form
    assert b'sampling needs uniforms' in lib.vqvae_last_error_string()

    t = _lib.GenSlots()
    t.n_seq, t.n_queue = 8, 8
    for name in ('steps', 'queue', 'next', 'slot_seq', 'slot_t', 'live'):
        setattr(t, name, fake)
    slots = lib.vqvae_wavenet_gen_step_slots_rng
    rejected('gen_step_slots_rng: null rng', slots(C.byref(d), C.byref(t), None, None, None))
    rejected('gen_step_slots_rng: null descriptor or slot table', slots(C.byref(d), None, None, C.byref(rng), None))
    rejected('gen_step_slots_rng: block 0 incomplete', slots(C.byref(d), C.byref(t), None, C.byref(rng), None))
    d.n_uniform = 9
    rejected('nr_mix uniforms', slots(C.byref(d), C.byref(t), None, C.byref(rng), None))
    d.n_uniform = 10
    d.sample_mode = _lib.GEN_NONE
    rejected('gen_step_slots_rng: sample_mode VQVAE_GEN_NONE', slots(C.byref(d), C.byref(t), None, C.byref(rng), None))
    d.sample_mode = M
    assert lib.vqvae_wavenet_gen_step_slots(C.byref(d), C.byref(t), None, None) == -1
    assert b'sampling needs uniforms' in lib.vqvae_last_error_string()


# ---- the compiled kernels -----------------------------------------------------------------------------------------------
def test_device_uniform_kernels_compile_without_scratch(tmp_path, record_property):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    src = os.path.join(ROOT, 'chainer-vq-vae_amd', 'csrc', 'gen_rng.hip')
    out = str(tmp_path / 'gen_rng.s')
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-S',
                           '--cuda-device-only', src, '-o', out], stderr=subprocess.DEVNULL)
    text = open(out).read()
    meta = {}
    for m in re.finditer(r'\.group_segment_fixed_size:\s*(\d+).*?\.name:\s*(\S+).*?\.private_segment_fixed_size:\s*(\d+)'
                         r'.*?\.vgpr_count:\s*(\d+).*?\.vgpr_spill_count:\s*(\d+)', text, re.S):
        meta[m.group(2)] = dict(lds=int(m.group(1)), scratch=int(m.group(3)), vgpr=int(m.group(4)), spill=int(m.group(5)))
    names = ('gen_rng_fill_kernel', 'gen_rng_lockstep_finish_kernel', 'gen_rng_sampled_finish_kernel',
             'gen_rng_slots_finish_kernel', 'gen_rng_slots_sampled_finish_kernel', 'gen_rng_advance_kernel')
    assert len(meta) == len(names), sorted(meta)
    for name in names:
        hits = [v for k, v in meta.items() if name in k]
        assert len(hits) == 1, '%s is not in the compiled module' % name
        record_property(name, '%(vgpr)d VGPRs, %(lds)d B LDS' % hits[0])
        assert (hits[0]['scratch'], hits[0]['spill']) == (0, 0), (name, hits[0])
