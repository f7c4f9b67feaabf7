"""CPU check of the segmental kernels' compiled resources (csrc/segmental.hip), read from the code object's metadata and
assembly.  The DP kernels keep V of a lane's codes and the next frame's row of D in registers (2 * CPL float64); an array
that went to scratch instead would leave every bit-equality test green and put a memory round trip into every frame of
the one loop that cannot be made parallel.

What was chosen, and the register bound it implies (registers are handed out eight at a time, 512 per lane of a SIMD):
  seg_dist_kernel          four waves per SIMD (four workgroups of 256 to a compute unit, 4 * 16896 bytes of LDS): at most
                           128.  It is float64 vector work on 16 accumulators a lane; more waves would not add arithmetic.
  seg_dp_kernel<1|2|4, 1>  one wavefront per (utterance, penalty), k <= 256: eight waves per SIMD, at most 64; the launch
                           is bound by its longest utterance, so what matters is that every (utterance, penalty) is resident.
  seg_dp_kernel<8, 1>      k <= 512: five waves, at most 96.
  seg_dp_kernel<4, 4>      256 lanes, k <= 1024: eight waves, at most 64.
  seg_dp_kernel<8, 4>      k <= 2048: five waves, at most 96.
  seg_dp_kernel<16, 4>     k <= 4096: four waves, at most 128.
  seg_dp_kernel<32, 4>     k <= 8192: V and the next row are 128 registers; two waves (two workgroups to a compute unit), at
                           most 256.
Measured with the Makefile's flags: 64; 30, 36, 53; 85; 53; 78; 127; 245 registers; no accumulation registers, no scratch,
no spills.  LDS is static throughout and does not depend on k: the distance kernel's z tile [32][64] and transposed W tile
[32][68] of float32, 8192 + 8704 bytes; the 256-lane DP kernels' double-buffered reduce slots, 2 * 4 * (8 + 4) = 96 bytes;
the one-wavefront DP kernels use none.  No launch asks for dynamic LDS."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'chainer-vq-vae_amd', 'csrc', 'segmental.hip')
# kernel (as mangled): (register ceiling, bytes of static LDS)
BUDGET = {'seg_dist_kernel': (128, 32 * 64 * 4 + 32 * 68 * 4),
          'seg_dp_kernelILi1ELi1EE': (64, 0), 'seg_dp_kernelILi2ELi1EE': (64, 0), 'seg_dp_kernelILi4ELi1EE': (64, 0),
          'seg_dp_kernelILi8ELi1EE': (96, 0), 'seg_dp_kernelILi4ELi4EE': (64, 96), 'seg_dp_kernelILi8ELi4EE': (96, 96),
          'seg_dp_kernelILi16ELi4EE': (128, 96), 'seg_dp_kernelILi32ELi4EE': (256, 96)}
FUSED = r'v_(pk_)?fma_f64|v_fmac_f64|v_mad_f64|v_mfma'


@pytest.fixture(scope='module')
def seg_asm(tmp_path_factory):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    out = str(tmp_path_factory.mktemp('seg') / 'segmental.s')
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-S',
                           '--cuda-device-only', SRC, '-o', out], stderr=subprocess.DEVNULL)
    return open(out).read()


@pytest.fixture(scope='module')
def seg_meta(seg_asm):
    meta = {}
    for m in re.finditer(r'\.agpr_count:\s*(\d+).*?\.group_segment_fixed_size:\s*(\d+).*?\.name:\s*(\S+)'
                         r'.*?\.private_segment_fixed_size:\s*(\d+).*?\.vgpr_count:\s*(\d+).*?\.vgpr_spill_count:\s*(\d+)',
                         seg_asm, re.S):
        if 'seg_' in m.group(3):
            meta[m.group(3)] = dict(agpr=int(m.group(1)), lds=int(m.group(2)), scratch=int(m.group(4)),
                                    vgpr=int(m.group(5)), spill=int(m.group(6)))
    return meta


def _body(asm, name):
    label = re.search(r'^(_ZN2vq\d+%s\w*):' % name, asm, flags=re.M).group(1)
    start = asm.index(label + ':')
    return asm[start:asm.index('.Lfunc_end', start)]


def test_every_launched_kernel_is_compiled_without_scratch(seg_meta, record_property):
    text = open(SRC).read()
    launched = set(re.findall(r'hipLaunchKernelGGL\(\(?(\w+)', text))
    assert launched == {'seg_dist_kernel', 'seg_dp_kernel'}
    instances = sorted((int(c), int(w)) for c, w in re.findall(r'sg_launch_dp<(\d+), (\d+)>\(a, P, s\)', text))
    assert instances == [(1, 1), (2, 1), (4, 1), (4, 4), (8, 1), (8, 4), (16, 4), (32, 4)]
    assert len(seg_meta) == len(BUDGET) == 1 + len(instances)
    for name, (vgpr_max, lds) in BUDGET.items():
        hits = [v for n, v in seg_meta.items() if name in n]
        assert len(hits) == 1, '%s is not in the compiled module' % name
        m = hits[0]
        record_property(name, '%(vgpr)d registers (%(agpr)d accumulation), %(lds)d bytes of static LDS' % m)
        print('%s: %r' % (name, m))
        assert (m['scratch'], m['spill']) == (0, 0), (name, m)
        assert m['agpr'] == 0 and m['vgpr'] <= vgpr_max, (name, m)
        assert m['lds'] == lds, (name, m)


@pytest.mark.parametrize('name', sorted(BUDGET))
def test_the_arithmetic_is_not_contracted(seg_asm, name):
    """The rule is float64 - * + with one rounding each: no fused multiply-add and no matrix instruction in any kernel.
    The table's terms are a product and an addition, so the distance kernel holds both instructions; steps 2 and 3 have no
    product at all (sw = m + lam, V = D + ...), so the DP kernels hold the addition and, having nothing to fuse, no
    multiplication either."""
    body = _body(seg_asm, name)
    assert not re.search(FUSED, body), re.findall(FUSED, body)[:3]
    assert 'v_add_f64' in body
    if 'dist' in name:
        assert body.count('v_mul_f64') >= 16 and body.count('v_add_f64') >= 32      # 16 cells: a subtraction and an addition each
    else:
        assert 'v_mul_f64' not in body and 'v_cmp_le_f64' in body                   # b = (V <= sw)


def test_the_module_multiplies_and_adds_in_float64(seg_asm):
    bodies = ''.join(_body(seg_asm, name) for name in BUDGET)
    assert 'v_add_f64' in bodies and 'v_mul_f64' in bodies and not re.search(FUSED, bodies)


def test_lds_is_within_a_cu_at_the_largest_codebook():
    """Static LDS restated; nothing is dynamic (every launch passes 0), so k = 8192 takes what k = 1 takes."""
    text = open(SRC).read()
    assert 'SG_LDS_CAP = 160 * 1024' in text and 'SG_JT = 32' in text and 'SG_WPAD = SG_TILE + 4' in text
    assert '__shared__ __attribute__((aligned(16))) float s_z[SG_JT][SG_TILE];' in text
    assert '__shared__ __attribute__((aligned(16))) float s_w[SG_JT][SG_WPAD];' in text
    assert '__shared__ double s_v[2][WAVES];' in text and '__shared__ int s_i[2][WAVES];' in text
    assert text.count('__shared__') == 4 and 'extern __shared__' not in text
    launches = re.findall(r'hipLaunchKernelGGL\((.*?)\);', text, flags=re.S)
    assert len(launches) == 2 and all(re.search(r'dim3\([^()]*(\([^()]*\))*[^()]*\),\s*0,\s*stream', ' '.join(l.split()))
                                      for l in launches), launches
    cap = 160 * 1024
    dist = 4 * 32 * (64 + 68)
    dp = 2 * 4 * 8 + 2 * 4 * 4
    assert dist == 16896 and dp == 96 and 4 * dist <= cap and 2 * dp <= cap
    assert 32 * 256 == 8192                                              # CPL 32 on 256 lanes reaches the largest k
