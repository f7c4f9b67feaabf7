"""CPU check of the speaker-identity kernels' compiled resources (csrc/speaker_id.hip), read from the code object's
metadata and assembly.  The score kernel keeps a frame's x and z = x - mu in registers and unrolls the whole triangle so
that every operand index is a constant; an array that went to scratch instead would leave every bit-equality test green
and put a memory round trip into each of the D (D + 1) / 2 products of every (frame, model).

What was chosen, and the register bound it implies (registers are handed out eight at a time, 512 per lane of a SIMD):
  spk_score_kernel<48>   two waves per SIMD, asked for with __launch_bounds__(256, 2): at most 256 registers.  x and z
                         are 96 registers each at D = 48, so nothing above two waves is to be had; the kernel is float64
                         vector work, and two workgroups' worth of waves per SIMD is what covers the LDS broadcasts.
  spk_score_kernel<32>   D <= 32 (the default 26): three waves, at most 168.
  spk_score_kernel<16>   D <= 16: five waves, at most 96.
  spk_features_kernel, spk_stats_kernel   eight waves, at most 64: they wait on memory, not on arithmetic.
Measured with the Makefile's flags: 28, 50, 88, 159 and 220 registers; no accumulation registers, no scratch, no spills.
LDS: the features kernel's fold and per-utterance maxima, 2 * 256 * 8 bytes; the statistics kernel's lane partials of
ACC_TILE = 8 accumulators and its count, 8 * 256 * 8 + 256 * 8; the score kernel's count statically, 256 * 8, and
dynamically MODEL_TILE * 8 * (D + D (D + 1) / 2 + 256) bytes (restated below): 40512 at D = 26, three workgroups to a
compute unit; 94720 at D = 48, one."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'chainer-vq-vae_amd', 'csrc', 'speaker_id.hip')
# kernel (as mangled): (register ceiling, bytes of static LDS)
BUDGET = {'spk_features_kernel': (64, 2 * 256 * 8), 'spk_stats_kernel': (64, 8 * 256 * 8 + 256 * 8),
          'spk_score_kernelILi16E': (96, 256 * 8), 'spk_score_kernelILi32E': (168, 256 * 8), 'spk_score_kernelILi48E': (256, 256 * 8)}


@pytest.fixture(scope='module')
def spk_asm(tmp_path_factory):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    out = str(tmp_path_factory.mktemp('spk') / 'speaker_id.s')
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-S',
                           '--cuda-device-only', SRC, '-o', out], stderr=subprocess.DEVNULL)
    return open(out).read()


@pytest.fixture(scope='module')
def spk_meta(spk_asm):
    meta = {}
    for m in re.finditer(r'\.agpr_count:\s*(\d+).*?\.group_segment_fixed_size:\s*(\d+).*?\.name:\s*(\S+)'
                         r'.*?\.private_segment_fixed_size:\s*(\d+).*?\.vgpr_count:\s*(\d+).*?\.vgpr_spill_count:\s*(\d+)',
                         spk_asm, re.S):
        if 'spk_' in m.group(3):
            meta[m.group(3)] = dict(agpr=int(m.group(1)), lds=int(m.group(2)), scratch=int(m.group(4)),
                                    vgpr=int(m.group(5)), spill=int(m.group(6)))
    return meta


def test_every_launched_kernel_is_compiled_without_scratch(spk_meta, record_property):
    launched = set(re.findall(r'hipLaunchKernelGGL\(\(?(\w+)', open(SRC).read()))
    assert launched == {'spk_features_kernel', 'spk_stats_kernel', 'spk_score_kernel'}
    assert len(spk_meta) == len(BUDGET)
    for name, (vgpr_max, lds) in BUDGET.items():
        hits = [v for n, v in spk_meta.items() if name in n]
        assert len(hits) == 1, '%s is not in the compiled module' % name
        m = hits[0]
        record_property(name, '%(vgpr)d registers (%(agpr)d accumulation), %(lds)d bytes of static LDS' % m)
        print('%s: %r' % (name, m))
        assert (m['scratch'], m['spill']) == (0, 0), (name, m)
        assert m['agpr'] == 0 and m['vgpr'] <= vgpr_max, (name, m)
        assert m['lds'] == lds, (name, m)
    text = open(SRC).read()
    assert '__launch_bounds__(SP_LANES, 2) void spk_score_kernel' in text


@pytest.mark.parametrize('name', ['spk_features_kernel', 'spk_stats_kernel', 'spk_score_kernelILi16E', 'spk_score_kernelILi32E',
                                  'spk_score_kernelILi48E'])
def test_the_sums_are_not_contracted(spk_asm, name):
    """The rule is float64 + - * with one rounding each, and one division per (utterance, model).  The only fused
    multiply-adds are those of that correctly rounded division (between its v_rcp_f64 and its v_div_fixup_f64); no matrix
    instruction anywhere."""
    label = re.search(r'^(_ZN2vq\d+%s\w*):' % name, spk_asm, flags=re.M).group(1)
    start = spk_asm.index(label + ':')
    body = spk_asm[start:spk_asm.index('.Lfunc_end', start)]            # the kernel returns in more than one place
    assert 'v_mul_f64' in body and 'v_add_f64' in body and 'v_mfma' not in body
    dividing, divisions, outside = 0, 0, []
    for line in body.splitlines():
        if 'v_rcp_f64' in line:
            dividing += 1
            divisions += 1
        if re.search(r'v_(pk_)?fma_f64|v_fmac_f64|v_mad_f64', line) and dividing <= 0:
            outside.append(line.strip())
        if 'v_div_fixup_f64' in line:
            dividing -= 1
    assert not outside and dividing == 0, (outside, dividing)
    assert divisions == (1 if 'score' in name else 0), divisions
    if 'score' in name:                                                 # the unrolled triangle: D (D + 1) / 2 products at the least
        dmax = int(re.search(r'ILi(\d+)E', name).group(1))
        assert body.count('v_mul_f64') >= dmax * (dmax + 1) // 2 + dmax, body.count('v_mul_f64')


def test_lds_is_within_a_cu_for_every_dimension():
    """The score launch's formula restated, with the kernel's static count array; the statistics kernel's LDS is static
    and does not depend on D."""
    text = open(SRC).read()
    assert 'SP_LDS_CAP = 160 * 1024' in text
    assert 'return sizeof(double) * (size_t)SP_TILE * ((size_t)D + (size_t)D * (D + 1) / 2 + SP_LANES);' in text
    assert 'const size_t lds = sp_score_lds(a.dim);' in text and 'lds_opt_in<spk_score_kernel<DMAX>>(lds)' in text
    assert '__shared__ double s_p[SP_ACC][SP_LANES];' in text
    cap, tile, lanes = 160 * 1024, 8, 256
    for D in range(1, 49):
        lds = 8 * tile * (D + D * (D + 1) // 2 + lanes) + 8 * lanes
        assert lds <= cap, D
    assert 8 * tile * (26 + 351 + lanes) == 40512 and 3 * (40512 + 2048) <= cap
    assert 8 * tile * (48 + 1176 + lanes) == 94720 and 94720 + 2048 <= cap < 2 * 94720
    assert 8 * 256 * 8 + 256 * 8 == 18432 <= cap
