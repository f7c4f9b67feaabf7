"""CPU check of the alignment kernels' compiled resources (csrc/audio_align.hip).  The DP kernel runs one workgroup per
pair and a barrier per anti-diagonal; what it keeps per cell lives in LDS, so a spilled register would put a scratch
round trip inside every one of a pair's Fa * Fb cells and leave every bit-equality test green.
Bounds: the DP kernel's LDS is all dynamic, 48 bytes per cell of the shorter side, set at the launch and bounded there by
the 160 KiB of a CU (restated below); with the coefficient loop unrolled by eight it holds sixteen float64 operands in
flight, and 64 registers (eight waves per SIMD: 512 / 8) are asked for.  The path kernel folds 256 float64 partials in
LDS: 2048 bytes."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'chainer-vq-vae_amd', 'csrc', 'audio_align.hip')
HEADER = os.path.join(ROOT, 'include', 'vqvae_align.h')


@pytest.fixture(scope='module')
def align_asm(tmp_path_factory):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    out = str(tmp_path_factory.mktemp('align') / 'audio_align.s')
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-S',
                           '--cuda-device-only', SRC, '-o', out], stderr=subprocess.DEVNULL)
    return open(out).read()


@pytest.fixture(scope='module')
def align_meta(align_asm):
    meta = {}
    for m in re.finditer(r'\.agpr_count:\s*(\d+).*?\.group_segment_fixed_size:\s*(\d+).*?\.name:\s*(\S+)'
                         r'.*?\.private_segment_fixed_size:\s*(\d+).*?\.vgpr_count:\s*(\d+).*?\.vgpr_spill_count:\s*(\d+)',
                         align_asm, re.S):
        if 'align_' in m.group(3):
            meta[m.group(3)] = dict(agpr=int(m.group(1)), lds=int(m.group(2)), scratch=int(m.group(4)),
                                    vgpr=int(m.group(5)), spill=int(m.group(6)))
    return meta


def test_every_launched_kernel_is_compiled_without_scratch(align_meta, record_property):
    launched = set(re.findall(r'hipLaunchKernelGGL\(\(?(\w+)', open(SRC).read()))
    assert launched == {'align_cepstra_kernel', 'align_dtw_kernel', 'align_path_kernel'}
    for name, vgpr_max, lds in (('align_cepstra_kernel', 32, 0), ('align_dtw_kernel', 64, 0), ('align_path_kernel', 32, 256 * 8)):
        hits = [v for n, v in align_meta.items() if name in n]
        assert len(hits) == 1, '%s is not in the compiled module' % name
        m = hits[0]
        record_property(name, '%(vgpr)d registers (%(agpr)d accumulation), %(lds)d bytes of static LDS' % m)
        assert (m['scratch'], m['spill']) == (0, 0), (name, m)
        assert m['agpr'] == 0 and m['vgpr'] <= vgpr_max, (name, m)
        assert m['lds'] == lds, (name, m)


def test_the_dp_has_one_barrier_and_no_contracted_sum(align_asm):
    """One s_barrier in the whole DP kernel: the one per anti-diagonal.  The rule is float64 + - * with one rounding each:
    the only fused multiply-adds are those of the correctly rounded square root's refinement, which follow its
    v_rsq_f64; none stands before the first (the coefficient sum) and every square root brings the same number."""
    start = align_asm.index('align_dtw_kernel')
    body = align_asm[start:align_asm.index('s_endpgm', start)]
    assert len(re.findall(r'\bs_barrier\b', body)) == 1
    assert 'v_mul_f64' in body and 'v_add_f64' in body
    fused = r'v_(pk_)?fma_f64|v_fmac_f64|v_mad_f64'
    roots = body.split('v_rsq_f64')
    assert len(roots) >= 2 and not re.search(fused, roots[0])
    counts = [len(re.findall(fused, part)) for part in roots[1:]]
    assert len(set(counts)) == 1 and 1 <= counts[0] <= 8, counts


def test_dynamic_lds_is_within_a_cu_at_the_bound():
    """The launch's formula restated: 3 diagonals * (8 + 4 + 4) bytes * max_short."""
    text, header = open(SRC).read(), open(HEADER).read()
    assert 'AL_LDS_CAP = 160 * 1024' in text and 'AL_CELL_BYTES = 3 * (sizeof(double) + 2 * sizeof(int))' in text
    assert 'const size_t lds = AL_CELL_BYTES * (size_t)d->max_short;' in text
    bound = int(re.search(r'#define VQVAE_ALIGN_MAX_SHORT (\d+)', header).group(1))
    assert bound == 3072 >= 2048
    assert 48 * bound == 147456 <= 160 * 1024 and 48 * (bound + 1024) > 160 * 1024      # the largest multiple of 1024 that fits
    assert 48 * 220 == 10560                                                          # a typical pair: many workgroups share a CU
