"""CPU check of the pitch kernels' compiled resources (csrc/audio_pitch.hip).  The tracker's inner loop keeps four float64
accumulators and the terms of four samples in registers; a difference sum moved to scratch would leave every bit-equality
test green and the launch several times slower.
Bounds: the tracker takes 33 KB of LDS at the default configuration, so several workgroups share a CU and it is the
register file that limits them: 64 registers allow eight waves per SIMD (512 / 8), and are asked for.  All of its LDS is
dynamic, set at the launch and bounded there by the 160 KB of a CU (restated below from the launch's own formula).  The
pair kernel holds three float64 and five integer partials per thread in LDS: 256 * (3 * 8 + 5 * 4) bytes."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'chainer-vq-vae_amd', 'csrc', 'audio_pitch.hip')


@pytest.fixture(scope='module')
def pitch_asm(tmp_path_factory):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    out = str(tmp_path_factory.mktemp('pitch') / 'audio_pitch.s')
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-S',
                           '--cuda-device-only', SRC, '-o', out], stderr=subprocess.DEVNULL)
    return open(out).read()


@pytest.fixture(scope='module')
def pitch_meta(pitch_asm):
    meta = {}
    for m in re.finditer(r'\.agpr_count:\s*(\d+).*?\.group_segment_fixed_size:\s*(\d+).*?\.name:\s*(\S+)'
                         r'.*?\.private_segment_fixed_size:\s*(\d+).*?\.vgpr_count:\s*(\d+).*?\.vgpr_spill_count:\s*(\d+)',
                         pitch_asm, re.S):
        if 'pitch_' in m.group(3):
            meta[m.group(3)] = dict(agpr=int(m.group(1)), lds=int(m.group(2)), scratch=int(m.group(4)),
                                    vgpr=int(m.group(5)), spill=int(m.group(6)))
    return meta


def test_every_launched_kernel_is_compiled_without_scratch(pitch_meta, record_property):
    launched = set(re.findall(r'hipLaunchKernelGGL\(\(?(\w+)', open(SRC).read()))
    assert launched == {'pitch_yin_kernel', 'pitch_compare_kernel'}
    for name, vgpr_max, lds in (('pitch_yin_kernel', 64, 0), ('pitch_compare_kernel', 64, 256 * (3 * 8 + 5 * 4))):
        hits = [v for n, v in pitch_meta.items() if name in n]
        assert len(hits) == 1, '%s is not in the compiled module' % name
        m = hits[0]
        record_property(name, '%(vgpr)d registers (%(agpr)d accumulation), %(lds)d bytes of static LDS' % m)
        assert (m['scratch'], m['spill']) == (0, 0), (name, m)
        assert m['agpr'] == 0 and m['vgpr'] <= vgpr_max, (name, m)
        assert m['lds'] == lds, (name, m)


def test_the_difference_sums_are_not_contracted(pitch_asm):
    """The rule is float64 + - * / with one rounding each.  The only fused multiply-adds of the tracker are those of the
    correctly rounded division itself (between its v_rcp_f64 and its v_div_fixup_f64); none may stand anywhere else.  (The
    pair kernel calls the device library's log and log2, which use them inside.)"""
    start = pitch_asm.index('pitch_yin_kernel')
    body = pitch_asm[start:pitch_asm.index('s_endpgm', start)]
    assert 'v_mul_f64' in body and 'v_add_f64' in body
    dividing, divisions, outside = 0, 0, []
    for line in body.splitlines():
        if 'v_rcp_f64' in line:
            dividing += 1
            divisions += 1
        if re.search(r'v_(pk_)?fma_f64|v_fmac_f64|v_mad_f64', line) and dividing <= 0:
            outside.append(line.strip())
        if 'v_div_fixup_f64' in line:
            dividing -= 1
    assert not outside and dividing == 0 and divisions >= 3, (outside, dividing, divisions)


def test_dynamic_lds_is_within_a_cu_for_every_configuration():
    """The launch's formula restated: 64 + tile * (16 (tau_max + 1) + 4 frame) bytes with tile = min(4, what fits 160 KB)."""
    text = open(SRC).read()
    assert 'PT_LDS_CAP = 160 * 1024' in text and 'PT_LDS_FIXED = PT_MAX_TILE * (sizeof(long long) + sizeof(double))' in text
    assert 'return 2 * sizeof(double) * ((size_t)tau_max + 1) + sizeof(float) * (size_t)frame' in text
    cap, fixed = 160 * 1024, 4 * 16
    worst = 0
    for frame in range(4, 2049):
        tau_max = frame - 2                                          # the largest the entry point takes: W = 2
        per = 16 * (tau_max + 1) + 4 * frame
        tile = min(4, (cap - fixed) // per)
        assert tile >= 1 and fixed + tile * per <= cap, frame
        worst = max(worst, fixed + tile * per)
    assert worst == 163840 == cap                                    # frame 2048, tau_max 2046, four frames: exactly a CU's
    assert fixed + 4 * (16 * 268 + 4 * 1024) == 33600                # the default configuration
