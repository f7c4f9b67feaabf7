"""CPU checks of the device-resident corpus (include/vqvae_corpus.h, csrc/corpus.hip, csrc/corpus_rule.h,
vqvae_amd.corpus): the header's known answers on the independent restatement (tests/resident_corpus_ref.py), the
permutation's properties, the package's host replay against the restatement, the very functions the kernel runs compiled
for the host into a stand-alone program, the split, the iterator's bookkeeping, the header against the table Python binds,
the entry point's validation and the compiled kernel's resources.  Every comparison of the rule is an equality."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import resident_corpus_ref as R
import vqvae_amd
from vqvae_amd import _lib
from vqvae_amd import corpus as K
from vqvae_amd.corpus import CorpusView, ResidentCorpus, ResidentCorpusIterator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'vqvae_corpus.h')
CSRC = os.path.join(ROOT, 'chainer-vq-vae_amd', 'csrc')
BIG_SEED = 2 ** 40 + 3
PLAN_LENGTHS = [1, 129, 130, 131, 1000]
PLAN = [[(2, 0), (4, 6), (0, 0), (1, 0)],
        [(3, 0), (1, 0), (0, 0), (3, 0)],
        [(2, 0), (4, 857), (2, 0), (0, 0)]]


# ---- the rule -----------------------------------------------------------------------------------------------------------
def test_known_answers_on_the_restatement():
    assert [R.pi(71, 0, p, 5) for p in range(5)] == [2, 4, 0, 1, 3]
    assert [R.pi(71, 1, p, 5) for p in range(5)] == [1, 0, 3, 2, 4]
    assert [R.pi(71, 0, p, 2) for p in range(2)] == [1, 0]
    assert [R.pi(BIG_SEED, 7, p, 1000) for p in range(6)] == [923, 47, 656, 221, 117, 678]
    assert [R.start_of(71, d, 1000) for d in range(4)] == [555, 6, 920, 140]
    assert R.start_of(71, 2 ** 32 + 1, 2 ** 31 + 5) == 123133830
    for it, want in enumerate(PLAN):
        assert R.plan(71, it, 4, PLAN_LENGTHS, 130) == want
    assert R.draw(71, 5, PLAN_LENGTHS, 130) == PLAN[1][1] and divmod(5, 5) == (1, 0)     # draw 5: epoch 1, position 0
    assert R.pi(71, 1, 0, 5) == 1


def test_known_answers_are_recorded_in_the_header():
    text = ' '.join(open(HEADER).read().replace('*', ' ').split())
    for line in ('e = 0 gives [2, 4, 0, 1, 3]', 'e = 1 gives [1, 0, 3, 2, 4]', 'n = 2 gives [1, 0]',
                 'p = 0..5 gives [923, 47, 656, 221, 117, 678]', 'd = 0..3 gives [555, 6, 920, 140]', 'gives 123133830',
                 'iteration 0: (2,0) (4,6) (0,0) (1,0)', 'iteration 1: (3,0) (1,0) (0,0) (3,0)',
                 'iteration 2: (2,0) (4,857) (2,0) (0,0)', '0x50455231', '0x43524F31'):
        assert line in text, line


@pytest.mark.parametrize('n', [1, 2, 3, 5, 7, 64, 65, 1000])
def test_pi_is_a_bijection_and_its_walks_are_bounded(n):
    for e in range(3):
        got = [R.pi_walks(71, e, p, n) for p in range(n)]
        assert sorted(q for q, _ in got) == list(range(n))
        if n > 1:
            assert max(w for _, w in got) <= 2 ** R.width(n)
            assert R.width(n) % 2 == 0 and 2 ** R.width(n) >= n and R.width(n) >= 2
        # the package's vectorised form walks all rows together
        np.testing.assert_array_equal(K.shuffled_positions(71, [e] * n, range(n), n), [q for q, _ in got])


def test_two_epochs_are_two_orders():
    a = [R.pi(71, 0, p, 64) for p in range(64)]
    b = [R.pi(71, 1, p, 64) for p in range(64)]
    assert a != b and a != list(range(64)) and sorted(a) == sorted(b)
    assert [R.pi(72, 0, p, 64) for p in range(64)] != a


def test_draws_across_an_epoch_boundary_inside_one_batch():
    lengths = PLAN_LENGTHS
    n, B = 5, 4
    draws = [u for it in range(5) for u, _ in R.plan(71, it, B, lengths, 130)]         # 20 draws = 4 epochs
    for e in range(4):
        assert sorted(draws[e * n:(e + 1) * n]) == list(range(n))
        assert draws[e * n:(e + 1) * n] == [R.pi(71, e, p, n) for p in range(n)]
    second = R.plan(71, 1, B, lengths, 130)                                             # draws 4..7: epoch 0 ends inside it
    assert second[0][0] == R.pi(71, 0, 4, n) and [u for u, _ in second[1:]] == [R.pi(71, 1, p, n) for p in range(3)]
    # without the shuffle: the utterances in order, again and again
    assert [u for it in range(3) for u, _ in R.plan(71, it, B, lengths, 130, shuffle=False)] == [d % n for d in range(12)]


def test_shards_partition_the_global_batch():
    lengths = [300, 500, 131, 4099, 1000, 140, 700]
    c = ResidentCorpus.describe(lengths, range(7))
    for it in range(4):
        whole = R.plan(9, it, 5, lengths, 130)
        parts = [R.plan(9, it, 5, lengths, 130, rows=range(rank, 5, 2)) for rank in (0, 1)]
        assert [len(p) for p in parts] == [3, 2]
        assert parts[0] == whole[0::2] and parts[1] == whole[1::2]
        for rank in (0, 1):
            got = ResidentCorpusIterator(c, 5, 129, 9, rank=rank, size=2).plan(it)
            assert got.dtype == np.int64 and [tuple(r) for r in got.tolist()] == whole[rank::2]


@pytest.mark.parametrize('shuffle', [True, False])
def test_iterator_plan_is_the_restatement(shuffle):
    rng = np.random.RandomState(3)
    lengths = rng.randint(1, 3000, size=37).tolist()
    c = ResidentCorpus.describe(lengths, rng.randint(0, 9, size=37))
    train, valid = c.split(30, seed=11)
    for seed in (71, BIG_SEED, 2 ** 64 - 1):
        for view, utts in ((c, None), (train, train.utterances), (valid, valid.utterances)):
            it = ResidentCorpusIterator(view, 6, 511, seed, shuffle=shuffle)
            for i in (0, 1, 5, 2 ** 31):                               # the last: draws beyond 2^32, epochs below
                want = R.plan(seed, i, 6, lengths, 512, shuffle, utts)
                assert [tuple(r) for r in it.plan(i).tolist()] == want
    assert [tuple(r) for r in K.plan_rows(71, 1, 4, PLAN_LENGTHS, 130).tolist()] == PLAN[1]
    assert K.crop_start(71, 2 ** 32 + 1, 2 ** 31 + 5) == 123133830 and K.crop_start(71, 3, 0) == 0 and K.crop_start(71, 3, -5) == 0
    with pytest.raises(ValueError, match='epoch'):
        K.plan_rows(71, 2 ** 40, 4, PLAN_LENGTHS, 130)


def test_shuffle_quality_is_coarsely_uniform():
    """Seed 71, n = 64, 600 epochs.  A uniform position has mean 31.5 and variance (64^2 - 1) / 12, so the mean of 600 has
    standard error sqrt(341.25 / 600) = 0.754: every utterance within 5 of them.  'Who is first' is a multinomial over 64
    cells with 600 / 64 expected: chi-square with 63 degrees of freedom, mean 63, variance 126: at most 63 + 5 sqrt(126)."""
    n, E = 64, 600
    where = np.empty((E, n), np.int64)                          # where[e, u]: the position of utterance u in epoch e
    first = np.zeros(n, np.int64)
    for e in range(E):
        order = K.shuffled_positions(71, np.full(n, e), np.arange(n), n)
        if e < 3:
            assert order.tolist() == [R.pi(71, e, p, n) for p in range(n)]
        where[e, order] = np.arange(n)
        first[order[0]] += 1
    se = np.sqrt((n * n - 1) / 12.0 / E)
    worst = np.abs(where.mean(axis=0) - 31.5).max() / se
    chi2 = float(((first - E / 64.0) ** 2 / (E / 64.0)).sum())
    print('worst mean position: %.2f standard errors; chi-square of the first place: %.1f' % (worst, chi2))
    assert worst <= 5.0
    assert chi2 <= 63 + 5 * np.sqrt(126.0)


# ---- the kernel's own functions, compiled for the host ------------------------------------------------------------------
_PROGRAM = r'''
#include <stdint.h>
#include <stdio.h>
#define __host__
#define __device__
#define __forceinline__ inline
#include "corpus_rule.h"
int main() {
  const uint64_t seeds[3] = {71ull, (1ull << 40) + 3ull, ~0ull};
  const uint32_t ns[9] = {1, 2, 3, 5, 7, 64, 65, 1000, 0x7fffffffu};
  const uint32_t es[4] = {0, 1, 7, 0xffffffffu};
  for (int s = 0; s < 3; ++s)
    for (int k = 0; k < 9; ++k)
      for (int j = 0; j < 4; ++j) {
        const uint32_t n = ns[k], top = n < 70 ? n : 70;
        for (uint32_t p = 0; p < top; ++p) printf("pi %d %u %u %u %u\n", s, n, es[j], p, vq::corpus_pi(seeds[s], es[j], p, n));
        if (n > 70) printf("pi %d %u %u %u %u\n", s, n, es[j], n - 1, vq::corpus_pi(seeds[s], es[j], n - 1, n));
      }
  const uint64_t ds[6] = {0, 1, 2, 3, (1ull << 32) + 1ull, ~0ull};
  const int64_t counts[7] = {-5, 0, 1, 2, 1000, (1ll << 31) + 5, 0x7fffffffll};
  for (int s = 0; s < 3; ++s)
    for (int i = 0; i < 6; ++i)
      for (int c = 0; c < 7; ++c)
        printf("start %d %llu %lld %lld\n", s, (unsigned long long)ds[i], (long long)counts[c],
               (long long)vq::corpus_start(seeds[s], ds[i], counts[c]));
  return 0;
}
'''


def test_device_functions_compiled_for_the_host_equal_the_restatement(tmp_path):
    """csrc/corpus_rule.h is what the kernel runs; here the host compiler builds the same functions into a program of its
    own (with the undefined-behaviour sanitiser when the toolchain has it: shifts and conversions are the risk)."""
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    src, exe = str(tmp_path / 'corpus_rule_host.cc'), str(tmp_path / 'corpus_rule_host')
    open(src, 'w').write(_PROGRAM)
    base = [cxx, '-O1', '-std=c++17', '-I', CSRC, src, '-o', exe]
    if subprocess.call(base + ['-fsanitize=undefined', '-fno-sanitize-recover=undefined'], stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(base)
    out = subprocess.run([exe], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert out.stderr == b'', out.stderr
    seeds = [71, BIG_SEED, 2 ** 64 - 1]
    lines = out.stdout.decode().split('\n')[:-1]
    assert len(lines) == 3 * 4 * (1 + 2 + 3 + 5 + 7 + 64 + 65 + 71 + 71) + 3 * 6 * 7
    for line in lines:
        f = line.split()
        if f[0] == 'pi':
            s, n, e, p, got = (int(v) for v in f[1:])
            assert got == R.pi(seeds[s], e, p, n), line
        else:
            s, d, count, got = (int(v) for v in f[1:])
            assert got == R.start_of(seeds[s], d, count), line
            assert got == 0 if count <= 0 else 0 <= got < count


# ---- the host package ---------------------------------------------------------------------------------------------------
def test_split_is_randomstate_permutation():
    c = ResidentCorpus.describe(np.arange(1, 24), np.arange(23) % 4)
    for seed in (0, 5, 12345):
        a, b = c.split(17, seed)
        order = np.random.RandomState(seed).permutation(23)
        assert isinstance(a, CorpusView) and a.utterances.dtype == np.int32
        assert a.utterances.tolist() == order[:17].tolist() and b.utterances.tolist() == order[17:].tolist()
        assert len(a) == 17 and len(b) == 6 and a.corpus is c
        assert a.lengths.tolist() == (order[:17] + 1).tolist() and b.speakers.tolist() == (order[17:] % 4).tolist()
    aa, ab = a.split(3, 1)                                                        # a view of a view names corpus utterances
    assert aa.utterances.tolist() == a.utterances[np.random.RandomState(1).permutation(17)[:3]].tolist()
    assert c.subset([5, 5, 2]).utterances.tolist() == [5, 5, 2]
    for bad in ([], [23], [-1], [0.5], [[1, 2]]):
        with pytest.raises(ValueError, match='subset'):
            c.subset(bad)
    for bad in (0, 23, 40):
        with pytest.raises(ValueError, match='split'):
            c.split(bad, 0)
    assert len(c) == 23 and c.lengths.dtype == np.int32 and c.offsets.tolist() == np.concatenate(([0], np.cumsum(np.arange(1, 23)))).tolist()
    assert c.nbytes == 4 * 276 + 16 * 23 and abs(c.hours(16000) - 276 / 16000.0 / 3600.0) < 1e-15
    assert vqvae_amd.ResidentCorpus is ResidentCorpus and vqvae_amd.ResidentCorpusIterator is ResidentCorpusIterator


def test_ingest_errors_need_no_device():
    ok = np.array([0.5, -0.25], np.float32)
    cases = [([], [], 'no waves'),
             ([ok, np.zeros(0, np.float32)], [0, 1], 'wave 1 is empty'),
             ([ok, np.zeros(5, np.float32)], [0, 1], 'wave 1 is all zeros'),
             ([np.array([0.1, np.nan], np.float32), ok], [0, 1], 'wave 0 holds a non-finite'),
             ([ok, np.array([np.inf, 0.5], np.float32)], [0, 1], 'wave 1 holds a non-finite'),
             ([ok, ok], [0], '1 speakers for 2 waves'),
             ([ok, ok], [0, -1], 'speaker ids'),
             ([ok, ok], [0, 1.5], 'speakers must be integers'),
             ([ok, np.zeros((2, 2), np.float32)], [0, 1], 'wave 1 is not a one-dimensional')]
    for waves, speakers, what in cases:
        with pytest.raises(ValueError, match=what):
            ResidentCorpus(waves, speakers)
    with pytest.raises(ValueError, match='wave 0 is empty'):
        ResidentCorpus.describe([0, 4], [0, 1])


def test_iterator_bookkeeping_state_and_argument_errors():
    c = ResidentCorpus.describe([200] * 7, range(7))
    it = ResidentCorpusIterator(c, 3, 99, 71)
    assert it.yields_rank_shard is True and (it.iteration, it.epoch, it.epoch_detail, it.is_new_epoch) == (0, 0, 0.0, False)
    assert [it.epoch_of(i) for i in range(6)] == [0, 0, 0, 1, 1, 2]
    state = dict(it.state_dict(), iteration=3)
    assert set(state) == {'seed', 'iteration', 'batch_size', 'n_view'}
    it.load_state_dict(state)
    assert (it.iteration, it.epoch, it.is_new_epoch) == (3, 1, True) and abs(it.epoch_detail - 9 / 7.0) < 1e-15
    assert [tuple(r) for r in it.plan().tolist()] == R.plan(71, 3, 3, [200] * 7, 100)
    for key, other in (('seed', 72), ('batch_size', 4), ('n_view', 8)):
        with pytest.raises(ValueError, match='load_state_dict: %s' % key):
            it.load_state_dict(dict(state, **{key: other}))
    with pytest.raises(ValueError, match='load_state_dict: iteration'):
        it.load_state_dict(dict(state, iteration=-1))
    assert it.iteration == 3
    it.reset()
    assert (it.iteration, it.is_new_epoch) == (0, False)
    with pytest.raises(RuntimeError, match='description only'):                     # before anything touches a device
        it.next()
    # one pass: 3 + 3 + 1 rows, in order
    once = ResidentCorpusIterator(c, 3, 99, 71, shuffle=False, repeat=False)
    assert [once.plan(i)[:, 0].tolist() for i in range(4)] == [[0, 1, 2], [3, 4, 5], [6], []]
    assert [once.epoch_of(i) for i in range(5)] == [0, 0, 0, 1, 1]
    for kw, err in ((dict(seed=-1), ValueError), (dict(seed=2 ** 64), ValueError), (dict(seed=1.5), TypeError),
                    (dict(batch_size=0), ValueError), (dict(length=0), ValueError), (dict(rank=2, size=2), ValueError),
                    (dict(rank=0, size=4), ValueError)):
        args = dict(batch_size=3, length=99, seed=1)
        args.update(kw)
        with pytest.raises(err, match='ResidentCorpusIterator'):
            ResidentCorpusIterator(c, **args)
    with pytest.raises(TypeError, match='ResidentCorpusIterator'):
        ResidentCorpusIterator([np.zeros(4)], 3, 99, 1)


# ---- the header, the table, the library ---------------------------------------------------------------------------------
NAMES = {'vqvae_corpus_abi_version', 'vqvae_corpus_draw'}


def test_header_exports_are_the_bound_table_and_versions_stand():
    """The header, the library, the versions and vqvae_corpus' layout: tests/test_host_abi.py, for every header."""
    table = _lib.HEADERS['vqvae_corpus.h'].prototypes
    assert set(table) == NAMES and len(table['vqvae_corpus_draw'][1]) == 18
    assert [f[0] for f in _lib.Corpus._fields_] == ['samples', 'offset', 'length', 'speaker', 'view', 'n_view']
    assert _lib.Corpus._fields_[5][1] is C.c_int32
    assert 'corpus' not in open(os.path.join(ROOT, 'include', 'vqvae_hip.h')).read()
    assert 'corpus.hip' in open(os.path.join(CSRC, 'Makefile')).read()


def test_c_side_validation_needs_no_device():
    lib = _lib.load()
    fake = 0x10000                                                      # never dereferenced: every call below is rejected first
    draw = lib.vqvae_corpus_draw

    def corpus(**kw):
        d = _lib.Corpus()
        d.samples = d.offset = d.length = d.speaker = fake
        d.view, d.n_view = None, 7
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def call(d=None, seed=71, shuffle=1, iteration=0, gb=5, row0=0, stride=1, rows=5, L1=130, thr=fake, nthr=255, x_enc=fake,
             x_dec=fake, t=fake, spk=fake):
        return draw(C.byref(d) if d is not None else None, seed, shuffle, iteration, gb, row0, stride, rows, L1, thr, nthr,
                    x_enc, x_dec, t, spk, None, None, None)

    def rejected(what, rc):
        assert rc == -1, what
        assert what.encode() in lib.vqvae_last_error_string(), (what, lib.vqvae_last_error_string())

    rejected('corpus_draw: null corpus', call(None))
    for name in ('samples', 'offset', 'length', 'speaker'):
        rejected('corpus_draw: null samples, offset, length or speaker', call(corpus(**{name: None})))
    for name in ('thr', 'x_enc', 'x_dec', 't', 'spk'):
        rejected('corpus_draw: null thresholds, x_enc, x_dec, t or speaker_out', call(corpus(), **{name: None}))
    rejected('corpus_draw: rows must be at least 1', call(corpus(), rows=0))
    rejected('corpus_draw: at most 65535 rows', call(corpus(), rows=65536, gb=70000))
    rejected('corpus_draw: L1 must be 2..2^30', call(corpus(), L1=1))
    rejected('corpus_draw: L1 must be 2..2^30', call(corpus(), L1=2 ** 30 + 1))
    rejected('corpus_draw: n_view must be at least 1', call(corpus(n_view=0)))
    rejected('corpus_draw: global_batch >= 1, row0 >= 0, row_stride >= 1', call(corpus(), gb=0))
    rejected('corpus_draw: global_batch >= 1, row0 >= 0, row_stride >= 1', call(corpus(), row0=-1))
    rejected('corpus_draw: global_batch >= 1, row0 >= 0, row_stride >= 1', call(corpus(), stride=0))
    rejected('corpus_draw: row 5 is not a row of a global batch of 5', call(corpus(), rows=6))
    rejected('corpus_draw: row 5 is not a row of a global batch of 5', call(corpus(), row0=1, stride=2, rows=3))
    rejected('corpus_draw: row 6 is not a row of a global batch of 5', call(corpus(), row0=2, stride=1, rows=5))
    rejected('corpus_draw: n_thresholds must be 1..8192', call(corpus(), nthr=0))
    rejected('corpus_draw: n_thresholds must be 1..8192', call(corpus(), nthr=8193))
    rejected('do not fit 64 bits', call(corpus(), iteration=2 ** 64 - 1))
    rejected('does not fit 32 bits', call(corpus(), iteration=7 * 2 ** 32 // 5 + 1))        # epoch 2^32
    rejected('does not fit 32 bits', call(corpus(n_view=1), iteration=2 ** 32 // 5 + 1, rows=1))


# ---- the compiled kernel ------------------------------------------------------------------------------------------------
def test_draw_kernel_compiles_without_scratch(tmp_path, record_property):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    out = str(tmp_path / 'corpus.s')
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-S',
                           '--cuda-device-only', os.path.join(CSRC, 'corpus.hip'), '-o', out], stderr=subprocess.DEVNULL)
    text = open(out).read()
    meta = {}
    for m in re.finditer(r'\.group_segment_fixed_size:\s*(\d+).*?\.name:\s*(\S+).*?\.private_segment_fixed_size:\s*(\d+)'
                         r'.*?\.vgpr_count:\s*(\d+).*?\.vgpr_spill_count:\s*(\d+)', text, re.S):
        meta[m.group(2)] = dict(lds=int(m.group(1)), scratch=int(m.group(3)), vgpr=int(m.group(4)), spill=int(m.group(5)))
    hits = [v for k, v in meta.items() if 'corpus_draw_kernel' in k]
    assert len(meta) == 1 and len(hits) == 1, sorted(meta)
    record_property('corpus_draw_kernel', '%(vgpr)d VGPRs, %(lds)d B LDS' % hits[0])
    assert (hits[0]['scratch'], hits[0]['spill']) == (0, 0), hits[0]
