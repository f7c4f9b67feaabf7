"""CPU checks of the optimizer hooks (include/vqvae_optim.h, vqvae_amd/optimizers.py): the work-item table, the
NumPy restatement of the summation order against the exact sum, the hook registry, and the compiled kernels'
resource budget."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import optim_hooks_ref as R
from vqvae_amd import _lib, optimizers as Op

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = _lib.OPTIM_CHUNK

# a 1-element parameter, a parameter whose offset is odd (everything behind the first), one element more than a chunk,
# an empty one, exactly a chunk, three chunks and a bit at an offset that is 1 mod 4, a short tail
AWKWARD = [1, 7, CHUNK + 1, 0, CHUNK, 3 * CHUNK + 1, 3]


def test_constants_mirror_the_header():
    """_lib's constants against the header's macros: tests/test_host_abi.py; the restatement mirrors _lib."""
    assert (R.CHUNK, R.THREADS) == (_lib.OPTIM_CHUNK, _lib.OPTIM_THREADS)


@pytest.mark.parametrize('sizes', [AWKWARD, [5], [CHUNK], [0, 0, 2], [2 * CHUNK, 1, 1, CHUNK - 1]])
def test_item_table_covers_every_element_exactly_once(sizes):
    items, params = Op.plan_items(sizes)
    n = sum(sizes)
    hits = np.zeros(n, np.int64)
    owner = np.full(n, -1, np.int64)
    assert params.shape == (len(sizes), 2)
    for p, (first, count) in enumerate(params):
        assert count == -(-sizes[p] // CHUNK)
        for s, ln in items[first:first + count]:
            assert 1 <= ln <= CHUNK and 0 <= s and s + ln <= n
            hits[s:s + ln] += 1
            owner[s:s + ln] = p
    assert (hits == 1).all()
    offs = np.concatenate([[0], np.cumsum(sizes)])
    for p, size in enumerate(sizes):
        assert (owner[offs[p]:offs[p + 1]] == p).all()
    assert int(params[:, 1].sum()) == len(items)
    # the restatement cuts the same chunks, and so does the library's host planner
    assert [(p, s, ln) for p, s, ln in R.chunks_of(sizes)] == \
        [(p, int(s), int(ln)) for p, (f, c) in enumerate(params) for s, ln in items[f:f + c]]
    lib = _lib.load()
    arr = (C.c_int64 * len(sizes))(*sizes)
    cnt = lib.vqvae_optim_plan_items(arr, len(sizes), None, None)
    assert cnt == len(items)
    it = (C.c_int32 * (2 * max(cnt, 1)))()
    pa = (C.c_int32 * (2 * len(sizes)))()
    assert lib.vqvae_optim_plan_items(arr, len(sizes), it, pa) == cnt
    assert (np.array(it)[:2 * cnt].reshape(-1, 2) == items).all() and (np.array(pa).reshape(-1, 2) == params).all()
    assert lib.vqvae_optim_workspace_bytes(cnt) == 8 * cnt
    assert lib.vqvae_optim_state_bytes(len(sizes), 3, 7) == 64 + 8 * len(sizes) + 12 + 7 * 5 * 4
    assert lib.vqvae_optim_state_bytes(len(sizes), 3, 0) == 0


def test_item_table_against_an_independent_construction():
    """Element by element: element i of the arena belongs to the parameter whose range holds it and to chunk
    (i - offset) // CHUNK of that parameter; the table's items are exactly the runs of equal (parameter, chunk)."""
    items, params = Op.plan_items(AWKWARD)
    offs = np.concatenate([[0], np.cumsum(AWKWARD)])
    i = np.arange(offs[-1])
    owner = np.searchsorted(offs, i, side='right') - 1
    chunk = (i - offs[owner]) // CHUNK
    cut = np.flatnonzero((np.diff(owner) != 0) | (np.diff(chunk) != 0)) + 1
    starts = np.concatenate([[0], cut])
    lengths = np.diff(np.concatenate([starts, [offs[-1]]]))
    assert (items[:, 0] == starts).all() and (items[:, 1] == lengths).all()
    counts = [len(set(chunk[owner == p])) for p in range(len(AWKWARD))]
    assert params[:, 1].tolist() == counts
    assert params[:, 0].tolist() == np.concatenate([[0], np.cumsum(counts)[:-1]]).tolist()
    with pytest.raises(ValueError):
        Op.plan_items([1 << 30, 1 << 30, 1])
    assert _lib.load().vqvae_optim_plan_items((C.c_int64 * 1)(-1), 1, None, None) == -1


def _exact_sumsq(g):
    return math.fsum((g.astype(np.float64) ** 2).tolist())      # each square is exact in float64; fsum rounds once


@pytest.mark.parametrize('seed,n', [(0, 5391000), (1, 5391003), (2, 12289)])
def test_restatement_against_the_exact_sum(seed, n):
    """float64 summation of n non-negative terms in ANY order is within n * 2^-53 (relative) of the exact sum."""
    rng = np.random.RandomState(seed)
    g = (10.0 ** rng.uniform(-12, 3, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    sizes, left = [], n
    while left:                                    # parameters of mixed sizes, odd offsets among them
        s = min(left, int(rng.choice([1, 3, 64, 513, CHUNK, CHUNK + 1, 70000, 524288])))
        sizes.append(s)
        left -= s
    sp = R.param_sumsq(g, sizes)
    S = R.total(sp)
    exact = _exact_sumsq(g)
    rel = abs(float(S) - exact) / exact
    print('n = %d: relative difference %.3e, bound %.3e' % (n, rel, n * 2.0 ** -53))
    assert rel <= n * 2.0 ** -53
    off = 0
    for p, s in enumerate(sizes[:40]):
        ex = _exact_sumsq(g[off:off + s])
        assert abs(float(sp[p]) - ex) <= s * 2.0 ** -53 * ex
        off += s


def test_restatement_finalise_fields():
    sp = np.array([4.0, 5.0, 16.0])
    f = R.finalise(sp, threshold=2.5, groups=[[0, 2], [1]])
    assert f['S'] == 25.0 and f['norm'] == 5.0 and f['rate'] == 0.5 and f['scale'] == np.float32(0.5)
    assert f['nonfinite'] == 0 and f['group_norms'].tolist() == [np.float32(np.sqrt(20.0)), np.float32(np.sqrt(5.0))]
    assert R.finalise(sp, threshold=10.0)['scale'] == np.float32(1.0)
    bad = R.finalise(np.array([1.0, np.inf]), threshold=1.0)
    assert bad['nonfinite'] == 1 and bad['rate'] == 0.0 and bad['scale'] == np.float32(0.0)
    nan = R.finalise(np.array([1.0, np.nan]), threshold=1.0)
    assert nan['nonfinite'] == 1 and np.isnan(nan['rate']) and nan['scale'] == np.float32(1.0)


# ---- the hook registry, on a host double of a set-up optimizer (no device: the tables are only uploaded when the
# arenas are device arrays) -----------------------------------------------------------------------------------------
class _Param(object):
    def __init__(self, size):
        self.size = size


class _Link(object):
    def __init__(self, name, params, children=()):
        self.name, self._p, self._c = name, params, list(children)

    def namedparams(self):
        for n, p in self._p:
            yield '/' + n, p
        for c in self._c:
            for n, p in c.namedparams():
                yield '/' + c.name + n, p

    def params(self):
        for _, p in self.namedparams():
            yield p

    def children(self):
        return iter(self._c)


def _host_optimizer():
    import collections
    enc = _Link('encoder', [('W', _Param(7)), ('b', _Param(1))])
    dec = _Link('decoder', [('W', _Param(CHUNK + 1))])
    bare = _Link('bare', [])
    model = _Link('main', [], [dec, enc, bare])
    opt = Op.Adam(2e-4)
    opt.target = model
    opt._hooks = collections.OrderedDict()        # what setup() does, without arenas on a device
    opt._layout, off = [], 0
    for n, p in model.namedparams():
        opt._layout.append((n, off, p.size))
        off += p.size
    opt.n_train = off
    opt.grads = None
    return opt, model


def test_add_hook_before_setup_raises():
    opt = Op.Adam()
    with pytest.raises(RuntimeError):
        opt.add_hook(Op.GradientClipping(1.0))
    with pytest.raises(RuntimeError):
        opt.remove_hook('GradientClipping')


def test_add_remove_hook_names_and_errors():
    opt, _ = _host_optimizer()
    opt.add_hook(Op.GradientClipping(1.0))
    opt.add_hook(Op.NonFiniteGuard(), name='guard')
    assert list(opt._hooks) == ['GradientClipping', 'guard']
    with pytest.raises(KeyError):
        opt.add_hook(Op.GradientNorms(), name='guard')                 # duplicate name
    with pytest.raises(KeyError):
        opt.remove_hook('NonFiniteGuard')                              # it was registered as 'guard'
    with pytest.raises(TypeError):
        opt.add_hook(lambda o: None)                                   # host callables cannot run inside the update
    opt.remove_hook('guard')
    opt.remove_hook('GradientClipping')
    assert not opt._hooks


def test_capture_key_follows_the_hook_configuration():
    opt, model = _host_optimizer()
    bare = opt.capture_key()
    assert bare == (0.9, 0.999, 1e-8)              # an optimizer without hooks keys as it always did
    clip = Op.GradientClipping(1.0)
    opt.add_hook(clip)
    k1 = opt.capture_key()
    clip.threshold = 2.0
    k2 = opt.capture_key()
    opt.add_hook(Op.NonFiniteGuard())
    k3 = opt.capture_key()
    opt.add_hook(Op.GradientNorms())
    k4 = opt.capture_key()
    opt.remove_hook('GradientNorms')
    opt.add_hook(Op.GradientNorms({'enc': list(model.children())[1]}))
    k5 = opt.capture_key()
    assert len({bare, k1, k2, k3, k4, k5}) == 6
    opt.remove_hook('GradientNorms')
    opt.add_hook(Op.GradientNorms(slots=8))
    assert opt.capture_key() not in {bare, k1, k2, k3, k4, k5}
    for name in list(opt._hooks):
        opt.remove_hook(name)
    assert opt.capture_key() == bare


def test_default_groups_are_the_children_that_own_parameters():
    opt, model = _host_optimizer()
    opt.add_hook(Op.GradientNorms())
    assert opt.hook_groups() == [('decoder', [0]), ('encoder', [1, 2])]        # 'bare' owns nothing
    opt.remove_hook('GradientNorms')
    enc = list(model.children())[1]
    opt.add_hook(Op.GradientNorms({'e': enc, 'all': model}))
    assert opt.hook_groups() == [('e', [1, 2]), ('all', [0, 1, 2])]


def test_hook_classes_are_exported():
    import vqvae_amd as V
    assert V.GradientClipping is Op.GradientClipping and V.NonFiniteGuard is Op.NonFiniteGuard
    assert V.GradientNorms is Op.GradientNorms


# ---- the compiled module -------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def optim_meta(tmp_path_factory):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    src = os.path.join(ROOT, 'chainer-vq-vae_amd', 'csrc', 'optim_hooks.hip')
    out = str(tmp_path_factory.mktemp('optim') / 'optim_hooks.s')
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-S',
                           '--cuda-device-only', src, '-o', out], stderr=subprocess.DEVNULL)
    text = open(out).read()
    meta = {}
    for m in re.finditer(r'\.agpr_count:\s*(\d+).*?\.group_segment_fixed_size:\s*(\d+).*?\.name:\s*(\S+)'
                         r'.*?\.private_segment_fixed_size:\s*(\d+).*?\.vgpr_count:\s*(\d+).*?\.vgpr_spill_count:\s*(\d+)',
                         text, re.S):
        meta[m.group(3)] = dict(lds=int(m.group(2)), scratch=int(m.group(4)), vgpr=int(m.group(5)), spill=int(m.group(6)))
    return meta, text


def test_kernels_compile_without_scratch(optim_meta, record_property):
    meta, text = optim_meta
    for kernel in ('optim_sumsq_kernel', 'optim_finalise_kernel', 'adam_hooked_kernel'):
        hits = [v for k, v in meta.items() if kernel in k]
        assert len(hits) == 1, '%s is not in the compiled module' % kernel
        record_property(kernel, '%(vgpr)d VGPRs, %(lds)d B LDS' % hits[0])
        assert (hits[0]['scratch'], hits[0]['spill']) == (0, 0), (kernel, hits[0])
    sumsq = [v for k, v in meta.items() if 'optim_sumsq_kernel' in k][0]
    assert sumsq['lds'] == 8 * _lib.OPTIM_THREADS
    assert sumsq['vgpr'] <= 64                     # eight waves a SIMD: the pass lives on loads in flight
    name = [k for k in meta if 'optim_sumsq_kernel' in k][0].replace('.kd', '')
    body = text[text.index('\n%s:' % name):]
    body = body[:body.index('s_endpgm')]           # the norm pass's own instructions (finalise's sqrt expands into FMAs)
    assert 'global_load_dwordx4' in body           # the 16-byte loads of whole quads
    assert 'v_mul_f64' in body and 'v_add_f64' in body
    assert 'v_fma_f64' not in body and 'v_fmac_f64' not in body      # a contracted g*g + acc would round once, NumPy twice
