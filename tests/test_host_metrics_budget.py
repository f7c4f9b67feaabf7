"""CPU check of the audio-metrics kernels' compiled resources (csrc/audio_metrics.hip).  The STFT kernel keeps the next
block of the DFT table in registers while the matrix pipe works on this one's (16 staged words beside 32 accumulators):
an array moved to scratch would leave every parity test green and the launch several times slower.
Bounds: the STFT kernel takes up to 103 KB of LDS at the default configuration, so one workgroup (one wave per SIMD)
lives on a CU and the register file is not what limits it; 128 registers would still allow four waves per SIMD (512 / 4)
for the small configurations, and is asked for.  All of its LDS is dynamic, set at the launch and bounded there by the
160 KB of a CU (restated below from the launch's own formula).  The distance kernel holds four float64 partials per
thread in LDS: 4 * 256 * 8 bytes."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'chainer-vq-vae_amd', 'csrc', 'audio_metrics.hip')


@pytest.fixture(scope='module')
def metrics_meta(tmp_path_factory):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    out = str(tmp_path_factory.mktemp('metrics') / 'audio_metrics.s')
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-S',
                           '--cuda-device-only', SRC, '-o', out], stderr=subprocess.DEVNULL)
    meta = {}
    for m in re.finditer(r'\.agpr_count:\s*(\d+).*?\.group_segment_fixed_size:\s*(\d+).*?\.name:\s*(\S+)'
                         r'.*?\.private_segment_fixed_size:\s*(\d+).*?\.vgpr_count:\s*(\d+).*?\.vgpr_spill_count:\s*(\d+)',
                         open(out).read(), re.S):
        if 'metrics_' in m.group(3):
            meta[m.group(3)] = dict(agpr=int(m.group(1)), lds=int(m.group(2)), scratch=int(m.group(4)),
                                    vgpr=int(m.group(5)), spill=int(m.group(6)))
    return meta


def test_every_launched_kernel_is_compiled_without_scratch(metrics_meta, record_property):
    launched = set(re.findall(r'hipLaunchKernelGGL\(\(?(\w+)', open(SRC).read()))
    assert launched == {'metrics_stft_mel_kernel', 'metrics_distances_kernel'}
    for name, vgpr_max, lds in (('metrics_stft_mel_kernel', 128, 0), ('metrics_distances_kernel', 64, 4 * 256 * 8)):
        hits = [v for n, v in metrics_meta.items() if name in n]
        assert len(hits) == 1, '%s is not in the compiled module' % name
        m = hits[0]
        record_property(name, '%(vgpr)d registers (%(agpr)d accumulation), %(lds)d bytes of static LDS' % m)
        assert (m['scratch'], m['spill']) == (0, 0), (name, m)
        assert m['agpr'] <= m['vgpr'] <= vgpr_max, (name, m)
        assert m['lds'] == lds, (name, m)


def _skew(s):
    return s + (s >> 5) + (s >> 10)


def test_dynamic_lds_is_within_a_cu_for_every_configuration():
    """The launch's formula restated: 384 + 128 nb bytes, + 4 (skew(n_fft + 31 hop - 1) + 1) when the samples are staged;
    staged only when that fits 160 KB, and the direct form fits for every n_fft the entry point takes."""
    text = open(SRC).read()
    assert 'MT_LDS_CAP = 160 * 1024' in text and 'return s + (s >> 5) + (s >> 10)' in text
    cap = 160 * 1024
    for n_fft in range(32, 2049, 32):
        nb = n_fft // 2 + 1
        direct = 32 * 12 + nb * 32 * 4
        assert direct <= cap, n_fft
    nb = 513
    assert 32 * 12 + nb * 128 + 4 * (_skew(1024 + 31 * 256 - 1) + 1) == 103036 <= cap      # the default: staged
    # the skew sends the 32 lanes of an operand read (hop samples apart) to 32 different banks for every power-of-two hop
    for hop in (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024):
        for k in (0, 5, 37, 1000):
            assert len({_skew(lane * hop + k) % 32 for lane in range(32)}) >= 16, (hop, k)
        assert len({_skew(lane * hop) % 32 for lane in range(32)}) == 32, hop
