"""CPU check of the ABX kernels' compiled resources (csrc/abx.hip), read from the code object's metadata and assembly.  The
one-wavefront DP keeps its diagonals and sixteen prefetched local costs in registers; an array that went to scratch instead
would leave every bit-equality test green and put a memory round trip into every diagonal of the one loop that cannot be
made parallel.

What was chosen, and the register bound it implies (registers are handed out eight at a time, 512 per lane of a SIMD):
  abx_local_kernel<metric, false>   one wavefront per 16 x 16 tile, 4096 bytes of LDS: eight waves per SIMD, at most 64.
  abx_local_kernel<metric, true>    the codebook's table, one call per snapshot: four waves, at most 128.
  abx_dtw_wave_kernel               one wavefront per pair; the launch is bound by its longest pair, so what matters is
                                    that many pairs are resident: five waves per SIMD, at most 96.
  abx_dtw_block_kernel              256 lanes; its occupancy is set by LDS (36 * max_short bytes), not registers: at most 64.
  abx_cell_kernel<0|1|2>, abx_norms_kernel   streaming; eight waves, at most 64.
Measured with the Makefile's flags: 56, 56; 88, 88; 67; 32; 24, 16, 17; 8 registers; no accumulation registers, no scratch,
no spills.  Static LDS: the local kernel's two float32 tiles [32][16], 2 * 2048 bytes; the 256-lane DP's is dynamic."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'chainer-vq-vae_amd', 'csrc', 'abx.hip')
HEADER = os.path.join(ROOT, 'chainer-vq-vae_amd', 'csrc', 'abx.h')
# kernel (as mangled): (register ceiling, bytes of static LDS)
BUDGET = {'abx_local_kernelILi0ELb0EE': (64, 4096), 'abx_local_kernelILi1ELb0EE': (64, 4096),
          'abx_local_kernelILi0ELb1EE': (128, 4096), 'abx_local_kernelILi1ELb1EE': (128, 4096),
          'abx_dtw_wave_kernel': (96, 0), 'abx_dtw_block_kernel': (64, 0),
          'abx_cell_kernelILi0EE': (64, 0), 'abx_cell_kernelILi1EE': (64, 0), 'abx_cell_kernelILi2EE': (64, 0),
          'abx_norms_kernel': (64, 0)}
FUSED = r'v_(pk_)?fma_f64|v_fmac_f64|v_mad_f64|v_mfma'


@pytest.fixture(scope='module')
def abx_asm(tmp_path_factory):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    out = str(tmp_path_factory.mktemp('abx') / 'abx.s')
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-S',
                           '--cuda-device-only', SRC, '-o', out], stderr=subprocess.DEVNULL)
    return open(out).read()


@pytest.fixture(scope='module')
def abx_meta(abx_asm):
    meta = {}
    for m in re.finditer(r'\.agpr_count:\s*(\d+).*?\.group_segment_fixed_size:\s*(\d+).*?\.name:\s*(\S+)'
                         r'.*?\.private_segment_fixed_size:\s*(\d+).*?\.vgpr_count:\s*(\d+).*?\.vgpr_spill_count:\s*(\d+)',
                         abx_asm, re.S):
        if 'abx_' in m.group(3):
            meta[m.group(3)] = dict(agpr=int(m.group(1)), lds=int(m.group(2)), scratch=int(m.group(4)),
                                    vgpr=int(m.group(5)), spill=int(m.group(6)))
    return meta


def _body(asm, name):
    label = re.search(r'^(_ZN2vq\d+%s\w*):' % name, asm, flags=re.M).group(1)
    start = asm.index(label + ':')
    return asm[start:asm.index('.Lfunc_end', start)]


def test_abx_hip_compiles_for_gfx950_and_every_launched_kernel_has_no_scratch(abx_meta, record_property):
    text = open(SRC).read()
    launched = set(re.findall(r'hipLaunchKernelGGL\(\(?(\w+)', text))
    assert launched == {'abx_norms_kernel', 'abx_local_kernel', 'abx_cell_kernel', 'abx_dtw_wave_kernel', 'abx_dtw_block_kernel'}
    assert len(abx_meta) == len(BUDGET)
    for name, (vgpr_max, lds) in BUDGET.items():
        hits = [v for n, v in abx_meta.items() if name in n]
        assert len(hits) == 1, '%s is not in the compiled module' % name
        m = hits[0]
        record_property(name, '%(vgpr)d registers (%(agpr)d accumulation), %(lds)d bytes of static LDS' % m)
        print('%s: %r' % (name, m))
        assert (m['scratch'], m['spill']) == (0, 0), (name, m)
        assert m['agpr'] == 0 and m['vgpr'] <= vgpr_max, (name, m)
        assert m['lds'] == lds, (name, m)


@pytest.mark.parametrize('name', [n for n in sorted(BUDGET) if 'local' in n])
def test_the_local_kernel_s_products_and_sums_are_not_contracted(abx_asm, name):
    """The sums of step 2 are float64 * + (and - for euclidean) with one rounding each: no fused multiply-add and no matrix
    instruction anywhere in the kernel's body.  The correctly rounded square root and division, whose refinements are
    fused by design, live in abx_cell_kernel, apart from the sums."""
    body = _body(abx_asm, name)
    assert not re.search(FUSED, body), re.findall(FUSED, body)[:3]
    assert body.count('v_mul_f64') >= 4 and body.count('v_add_f64') >= 4          # 2 x 2 cells a lane


def test_the_dp_kernels_add_and_compare_only(abx_asm):
    for name in ('abx_dtw_wave_kernel', 'abx_dtw_block_kernel'):
        body = _body(abx_asm, name)
        assert 'v_add_f64' in body and re.search(r'v_cmp_n?[lg][te]_f64', body), name
        assert 'v_mfma' not in body and 'v_mul_f64' not in body.split('v_rcp_f64')[0], name      # only distance = cost / K divides
    wave = _body(abx_asm, 'abx_dtw_wave_kernel')
    assert 's_barrier' not in wave and 'ds_' not in wave                 # no LDS and no barrier in the one-wavefront form
    assert 'wave_shr:1' in wave                                          # the neighbour's values arrive by a cross-lane move
    assert len(re.findall(r'\bs_barrier\b', _body(abx_asm, 'abx_dtw_block_kernel'))) == 1


def test_lds_is_within_a_cu():
    """The 256-lane form's dynamic LDS at MAX_SHORT and the local kernel's static LDS, restated."""
    text, header = open(SRC).read(), open(HEADER).read()
    assert 'AB_LDS_CAP = 160 * 1024' in text and 'AB_JT = 32' in text
    assert 'AB_CELL_BYTES = 3 * (sizeof(double) + sizeof(int))' in text
    assert 'const size_t lds = AB_CELL_BYTES * (size_t)d->max_short;' in text
    assert '__shared__ __attribute__((aligned(16))) float s_a[AB_JT][AB_TILE];' in text
    assert '__shared__ __attribute__((aligned(16))) float s_b[AB_JT][AB_TILE];' in text
    assert text.count('__shared__') == 3 and text.count('extern __shared__') == 1
    bound = int(re.search(r'#define VQVAE_ABX_MAX_SHORT (\d+)', header).group(1))
    tile = int(re.search(r'#define VQVAE_ABX_TILE (\d+)', header).group(1))
    assert bound == 1024 and 36 * bound == 36864 <= 64 * 1024 <= 160 * 1024       # 36 KB: four pairs to a CU, no opt-in
    assert 2 * 4 * 32 * tile == 4096 and 8 * 4 * 4096 <= 160 * 1024                # eight waves per SIMD keep their tiles
