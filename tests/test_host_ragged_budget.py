"""CPU check of the ragged conv kernels' compiled resources (csrc/ragged_front.hip).  The kernels keep the next channel
group's operands in registers while the matrix pipe works (up to 64 staged words per thread beside up to 64
accumulators): an array moved to scratch would leave every parity test green and the launch several times slower.
Bounds, from the register file alone (512 registers per SIMD lane, accumulation registers included in vgpr_count):
the 64 x 64-tile kernels keep three waves per SIMD (512 / 3, allocated in eights: 168), the 128 x 128-tile kernels, whose
four waves are one per SIMD, must fit one wave (512)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def ragged_meta(tmp_path_factory):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    src = os.path.join(ROOT, 'chainer-vq-vae_amd', 'csrc', 'ragged_front.hip')
    out = str(tmp_path_factory.mktemp('ragged') / 'ragged_front.s')
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-S',
                           '--cuda-device-only', src, '-o', out], stderr=subprocess.DEVNULL)
    meta = {}
    for m in re.finditer(r'\.agpr_count:\s*(\d+).*?\.group_segment_fixed_size:\s*(\d+).*?\.name:\s*(\S+)'
                         r'.*?\.private_segment_fixed_size:\s*(\d+).*?\.vgpr_count:\s*(\d+).*?\.vgpr_spill_count:\s*(\d+)',
                         open(out).read(), re.S):
        if 'ragged_' in m.group(3):
            meta[m.group(3)] = dict(agpr=int(m.group(1)), lds=int(m.group(2)), scratch=int(m.group(4)),
                                    vgpr=int(m.group(5)), spill=int(m.group(6)))
    return meta


def test_every_launched_instantiation_is_compiled_without_scratch(ragged_meta, record_property):
    for mode in (0, 3):
        for t2 in (1, 2):
            for k in (3, 4):
                hits = [v for n, v in ragged_meta.items() if 'ragged_conv_kernelILi%dELi%dELi%dEE' % (mode, t2, k) in n]
                assert len(hits) == 1, 'ragged_conv_kernel<%d, %d, %d> is not in the compiled module' % (mode, t2, k)
                m = hits[0]
                record_property('ragged_conv_kernel_%d_%d_%d' % (mode, t2, k), '%(vgpr)d registers (%(agpr)d accumulation)' % m)
                assert (m['scratch'], m['spill']) == (0, 0), (mode, t2, k, m)
                assert m['agpr'] <= m['vgpr'] <= (168 if t2 == 1 else 512), (mode, t2, k, m)
                assert m['lds'] == 0, (mode, t2, k, m)                         # all of it dynamic: 34.3 / 68.3 KB, set at the launch
    for name in ('ragged_conv1_kernel', 'ragged_code_gather_kernel', 'ragged_speaker_gather_kernel'):
        hits = [v for n, v in ragged_meta.items() if name in n]
        assert len(hits) == 1 and (hits[0]['scratch'], hits[0]['spill']) == (0, 0), (name, hits)
        assert hits[0]['vgpr'] <= 128 and hits[0]['lds'] <= 2048, (name, hits)
