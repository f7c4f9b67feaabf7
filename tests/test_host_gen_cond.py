"""CPU checks of the latent-rate condition of lockstep generation (include/vqvae_gen_cond.h, csrc/generate_cond.hip,
vqvae_amd.generation.LatentCondition): the column rule restated in NumPy against the tables the dense up-sampling uses,
the header against the table Python binds, the object's bookkeeping, run_lockstep / run_lockstep_refill on stubs in place
of the device, the entry point's argument validation and the compiled kernel's resources."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import gen_cond_ref as R
from vqvae_amd import _lib
from vqvae_amd.functions import resize_tables_host
from vqvae_amd.generation import LatentCondition, run_lockstep, run_lockstep_refill

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the rule ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('upscale', [1, 3, 64])
def test_restated_positions_are_the_existing_tables(upscale):
    """t * ((H-1) / (T-1)) in float64 with the last element set to H-1 is np.linspace(0, H-1, T) as
    functions.resize_tables_host uses it: v0, v1, w0 and w1 agree exactly, vectorised and element by element."""
    for H in list(range(1, 41)) + [120, 2500]:
        T = upscale * H
        want = resize_tables_host(H, T)
        v0, v1, w0, w1 = R.tables(H, upscale)
        for got, name in ((v0, 'v0'), (v1, 'v1')):
            np.testing.assert_array_equal(got, want[name], '%s at H = %d' % (name, H))
        for got, name in ((w0, 'w0'), (w1, 'w1')):
            assert got.dtype == np.float32
            np.testing.assert_array_equal(_bits(got), _bits(want[name]), '%s at H = %d' % (name, H))
        ts = range(T) if T <= 200 else list(range(0, T, 997)) + [0, 1, upscale - 1, upscale, T - 2, T - 1]
        for t in ts:
            inside, a0, a1, b0, b1 = R.position(t, H, upscale)
            assert inside and (a0, a1) == (want['v0'][t], want['v1'][t]), (H, t)
            assert _bits(b0) == _bits(want['w0'][t]) and _bits(b1) == _bits(want['w1'][t]), (H, t)
        assert R.position(T, H, upscale)[0] is False and R.position(T + 5, H, upscale)[0] is False


def test_restated_column_is_a_column_of_the_restated_expansion():
    rs = np.random.RandomState(11)
    for tl, upscale in ((1, 64), (2, 64), (3, 64), (5, 64), (7, 3), (4, 1)):
        x = rs.standard_normal((20, tl)).astype(np.float32)
        g = rs.standard_normal(13).astype(np.float32)
        full = R.dense(x, g, upscale)
        assert full.shape == (33, upscale * tl) and full.dtype == np.float32
        for t in range(upscale * tl):
            np.testing.assert_array_equal(_bits(R.column(x, g, t, upscale)), _bits(full[:, t]), 'tl %d t %d' % (tl, t))
        past = R.column(x, g, upscale * tl, upscale)
        assert not past[:20].any()
        np.testing.assert_array_equal(past[20:], g)
        if tl == 1:                                                       # one frame: the frame itself at every step
            np.testing.assert_array_equal(full[:20], np.repeat(x, upscale, axis=1))


# ---- the header, the table, the library -------------------------------------------------------------------------------
def test_header_exports_are_the_bound_table_and_versions_stand():
    """The header, the library, the versions and vqvae_gen_latent_cond's layout: tests/test_host_abi.py, for every header."""
    assert set(_lib.HEADERS['vqvae_gen_cond.h'].prototypes) == {'vqvae_gen_cond_abi_version', 'vqvae_gen_cond_column'}
    assert 'generate_cond.hip' in open(os.path.join(ROOT, 'chainer-vq-vae_amd', 'csrc', 'Makefile')).read()


def test_c_side_validation_needs_no_device():
    lib = _lib.load()
    fake = 0x10000                                                      # never dereferenced: every call below is rejected first

    def latent(**kw):
        c = _lib.GenLatentCond()
        for name in ('local', 'local_off', 'tl', 'global_vec', 'column'):
            setattr(c, name, fake)
        c.n_seq, c.Cl, c.G, c.upscale = 8, 20, 13, 64
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def table(**kw):
        t = _lib.GenSlots()
        t.n_seq, t.n_queue = 8, 8
        for name in ('steps', 'queue', 'next', 'slot_seq', 'slot_t', 'live'):
            setattr(t, name, fake)
        for k, v in kw.items():
            setattr(t, k, v)
        return t

    d = _lib.GenDesc()
    d.n, d.step, d.cond_dim = 5, fake, 33
    fn = lib.vqvae_gen_cond_column

    def rejected(what, *args):
        assert fn(*args) == -1, what
        assert what.encode() in lib.vqvae_last_error_string(), (what, lib.vqvae_last_error_string())

    rejected('null latent condition or descriptor', None, C.byref(d), None, None)
    rejected('null latent condition or descriptor', C.byref(latent()), None, None, None)
    for member in ('local', 'local_off', 'tl', 'global_vec', 'column'):
        rejected('null latent condition member', C.byref(latent(**{member: None})), C.byref(d), None, None)
    rejected('cond_dim', C.byref(latent(Cl=21)), C.byref(d), None, None)
    rejected('cond_dim', C.byref(latent(G=12)), C.byref(d), None, None)
    rejected('upscale', C.byref(latent(upscale=0)), C.byref(d), None, None)
    for name in ('n_seq', 'Cl', 'G'):
        rejected('negative count', C.byref(latent(**{name: -1})), C.byref(d), None, None)
    for n in (0, 129):
        d.n = n
        rejected('1..128', C.byref(latent()), C.byref(d), None, None)
    d.n = 5
    d.step = None
    rejected('null step counter', C.byref(latent()), C.byref(d), None, None)
    d.step = fake
    for member in ('slot_seq', 'slot_t', 'live'):
        rejected('null slot table member', C.byref(latent()), C.byref(d), C.byref(table(**{member: None})), None)
    rejected('the slot table has 9 sequences', C.byref(latent()), C.byref(d), C.byref(table(n_seq=9, n_queue=9)), None)


# ---- LatentCondition on the host --------------------------------------------------------------------------------------
def test_latent_condition_bookkeeping_and_the_memory_formula():
    lc = LatentCondition([3, 1, 2, 5], 20, 13, 64)
    assert lc.shape == (4, 33, 320) and lc.ndim == 3
    np.testing.assert_array_equal(lc.lengths, [192, 64, 128, 320])
    np.testing.assert_array_equal(lc.local_off, [0, 60, 80, 120])
    assert lc.local_off.dtype == np.int64 and lc.tl.dtype == np.int32
    assert lc.nbytes == 4 * 20 * 11 + 4 * 13 * 4 and lc.dense_nbytes == 4 * 33 * 4 * 320
    with pytest.raises(RuntimeError, match='no device data'):
        lc.dense()
    # the default model: 300 utterances of 2 500 latent frames (10 s at 16 kHz)
    N, Tl = 300, 2500
    big = LatentCondition([Tl] * N, 512, 128, 64)
    assert big.dense_nbytes == 4 * 640 * N * (64 * Tl) == 122880000000
    assert big.nbytes == 4 * 512 * N * Tl + 4 * 128 * N == 1536153600
    assert 79.9 < big.dense_nbytes / big.nbytes < 80.0                  # 2 560 against 32 bytes per sample
    assert int(big.local_off[-1]) == 512 * Tl * (N - 1) > 2 ** 28       # the offsets are 64-bit for a reason
    ragged = LatentCondition([2500, 100, 100], 512, 128, 64)           # the dense form pads to the longest
    assert ragged.dense_nbytes == 4 * 640 * 3 * 160000 and ragged.nbytes == 4 * 512 * 2700 + 4 * 128 * 3
    for bad in (dict(tl=[]), dict(tl=[3, 0]), dict(tl=[[1, 2]]), dict(tl=[1.5]), dict(upscale=0), dict(Cl=-1), dict(Cl=0, G=0),
                dict(tl=[2 ** 26], upscale=64)):
        kw = dict(tl=[1, 2], Cl=4, G=2, upscale=64)
        kw.update(bad)
        with pytest.raises(ValueError):
            LatentCondition(**kw)


def test_from_latents_refuses_bad_shapes_before_it_needs_a_device():
    f32 = np.float32
    g = np.zeros((2, 13), f32)
    with pytest.raises(ValueError, match='different channel counts'):
        LatentCondition.from_latents([np.zeros((20, 3), f32), np.zeros((21, 3), f32)], g, 64)
    with pytest.raises(ValueError, match='0 frames'):
        LatentCondition.from_latents([np.zeros((20, 3), f32), np.zeros((20, 0), f32)], g, 64)
    with pytest.raises(ValueError, match='no sequences'):
        LatentCondition.from_latents([], g, 64)
    with pytest.raises(ValueError, match='Cl, Tl'):
        LatentCondition.from_latents([np.zeros((20, 3, 2), f32), np.zeros((20, 3), f32)], g, 64)
    for bad in (np.zeros((3, 13), f32), np.zeros((13,), f32), np.zeros((2, 13, 1), f32)):
        with pytest.raises(ValueError, match='global_vec'):
            LatentCondition.from_latents([np.zeros((20, 3), f32), np.zeros((20, 2), f32)], bad, 64)
    with pytest.raises(ValueError):                                     # host arrays cannot be computed on
        LatentCondition.from_latents([np.zeros((20, 3), f32), np.zeros((20, 2), f32)], g, 64)


def test_the_dense_paths_refuse_a_latent_condition_by_name():
    import vqvae_amd
    from vqvae_amd.wavenet import WaveNet
    assert vqvae_amd.LatentCondition is LatentCondition
    dec = WaveNet(1, 2, 2, 16, 8, 8, 8, 256, False, 16, -40, 8, 0)
    lc = LatentCondition([2, 2], 5, 3, 4)
    u = np.zeros((8, 2))
    for call in (lambda: dec.generate_sequence(lc, u), lambda: dec.generate_batch(lc, u),
                 lambda: dec.generate(np.zeros((2, 16, 1, 1), np.float32), lc)):
        with pytest.raises(TypeError, match=r'generate_lockstep') as e:
            call()
        assert '.dense()' in str(e.value)
    with pytest.raises(ValueError, match='generate_lockstep'):           # the controls are still checked first
        dec.generate_lockstep(lc, u, temperature=-1.0)


# ---- the runners around stubs -----------------------------------------------------------------------------------------
class _StubNet(object):
    class proj2(object):
        class W(object):
            shape = (8, 4)


def test_stubbed_runners_see_what_they_see_with_a_dense_array():
    tl = np.array([3, 1, 2, 3, 1, 2, 2, 1, 3, 1, 2, 1, 3])
    lc = LatentCondition(tl, 2, 1, 4)
    N, Cc, T = lc.shape
    assert (N, Cc, T) == (13, 3, 12)
    dense = np.zeros(lc.shape, np.float32)
    rs = np.random.RandomState(0)
    u = rs.random_sample((T, N))
    forced = rs.randint(0, 4, (T, N)).astype(np.int32)

    def grouped(cond, **kw):
        calls = []

        def stub(idx, ug, fg, gsteps):
            calls.append((np.array(idx).tolist(), gsteps, ug.copy(), fg.copy()))
            o = np.zeros((len(idx), T), np.int32)
            o[:, :gsteps] = 1000 * np.asarray(idx)[:, None] + np.arange(gsteps)[None, :] + 1
            return o, np.ones((gsteps, len(idx), 8), np.float32)
        res = run_lockstep(_StubNet(), cond, u, _lib.GEN_SOFTMAX, forced=forced, return_logits=True, group=5, _run_group=stub, **kw)
        return calls, res

    def refilled(cond, **kw):
        calls = []

        def stub(steps, ug, fg, sampling):
            calls.append((np.array(steps).tolist(), ug.copy(), fg.copy(), sampling))
            o = (1000 * np.arange(N)[:, None] + np.arange(T)[None, :] + 1).astype(np.int32)
            return o, np.ones((int(max(steps)), N, 8), np.float32)
        res = run_lockstep_refill(_StubNet(), cond, u, _lib.GEN_SOFTMAX, forced=forced, return_logits=True, group=5, _run=stub, **kw)
        return calls, res

    for runner in (grouped, refilled):
        for kw_lat, kw_dense in ((dict(), dict(lengths=lc.lengths)),                      # lengths default to the object's own
                                 (dict(n_steps=5), dict(lengths=lc.lengths, n_steps=5)),
                                 (dict(lengths=np.minimum(lc.lengths, 7)), dict(lengths=np.minimum(lc.lengths, 7)))):
            a, ra = runner(lc, **kw_lat)
            b, rb = runner(dense, **kw_dense)
            assert len(a) == len(b) > 0
            for x, y in zip(a, b):
                for p, q in zip(x, y):
                    np.testing.assert_array_equal(p, q)
            np.testing.assert_array_equal(ra[0], rb[0])
            np.testing.assert_array_equal(ra[1], rb[1])
    calls, (out, _) = grouped(lc)
    assert calls[0][0] == [0, 3, 8, 12, 2] and calls[0][1] == 11      # longest first: 12 samples, 11 steps
    assert calls[-1][0] == [7, 9, 11, 11, 11]                                          # filled up with repeats of the last member
    for i, L in enumerate(lc.lengths):
        assert (out[i, :L - 1] > 0).all() and not out[i, L - 1:].any()
    for cond in (lc, dense):
        for bad in (dict(uniforms=u[:5]), dict(uniforms=u[:, :5]), dict(lengths=lc.lengths[:-1]), dict(lengths=np.full(N, T + 1)),
                    dict(group=4), dict(group=129), dict(forced=forced[:3]), dict(n_steps=T + 1, lengths=None)):
            kw = dict(uniforms=u, lengths=lc.lengths, forced=forced)
            kw.update(bad)
            if cond is lc and 'n_steps' in bad:
                continue                                                # without lengths the object's own apply: no error to compare
            uu = kw.pop('uniforms')
            with pytest.raises(ValueError):
                run_lockstep(_StubNet(), cond, uu, _lib.GEN_SOFTMAX, _run_group=lambda *a: None, **kw)
            with pytest.raises(ValueError):
                run_lockstep_refill(_StubNet(), cond, uu, _lib.GEN_SOFTMAX, _run=lambda *a: None, **kw)


def test_latent_condition_is_an_argument_of_the_synthesis_calls():
    import inspect
    import vqvae_amd
    for fn in (vqvae_amd.synthesize, vqvae_amd.synthesize_many):
        assert inspect.signature(fn).parameters['latent_condition'].default is False


# ---- the compiled kernel ----------------------------------------------------------------------------------------------
def test_column_kernel_compiles_without_scratch(tmp_path, record_property):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    src = os.path.join(ROOT, 'chainer-vq-vae_amd', 'csrc', 'generate_cond.hip')
    out = str(tmp_path / 'generate_cond.s')
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-S',
                           '--cuda-device-only', src, '-o', out], stderr=subprocess.DEVNULL)
    text = open(out).read()
    meta = {}
    for m in re.finditer(r'\.group_segment_fixed_size:\s*(\d+).*?\.name:\s*(\S+).*?\.private_segment_fixed_size:\s*(\d+)'
                         r'.*?\.vgpr_count:\s*(\d+).*?\.vgpr_spill_count:\s*(\d+)', text, re.S):
        meta[m.group(2)] = dict(lds=int(m.group(1)), scratch=int(m.group(3)), vgpr=int(m.group(4)), spill=int(m.group(5)))
    hits = [v for k, v in meta.items() if 'gen_cond_column_kernel' in k]
    assert len(meta) == 1 and len(hits) == 1, sorted(meta)
    record_property('gen_cond_column_kernel', '%(vgpr)d VGPRs, %(lds)d B LDS' % hits[0])
    assert (hits[0]['scratch'], hits[0]['spill'], hits[0]['lds']) == (0, 0, 0), hits[0]
    assert 'atomic' not in text and 'v_fma_f32' not in text and 'v_fmac_f32' not in text, \
        'no atomics, and the two products and the sum are not contracted'
