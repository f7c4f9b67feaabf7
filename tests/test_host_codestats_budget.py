"""CPU check of the code-statistics kernels' compiled resources (csrc/code_stats.hip), read from the code object's
metadata.  The edit-distance kernel runs one workgroup per pair and a barrier per anti-diagonal; what it keeps per cell
lives in LDS, so a spilled register would put a scratch round trip inside every one of a pair's La * Lb cells and leave
every bit-equality test green.

Measured with the Makefile's flags: codes_runs_kernel 33 registers and 2048 bytes of static LDS (the two scan arrays),
codes_hist_kernel 14 and none, codes_agree_kernel 19 and 1024 (the fold), codes_edit_kernel 19 and none (its LDS is all
dynamic, 24 bytes per cell of the shorter side, set at the launch and restated below); no accumulation registers, no
scratch.  Registers are allocated eight at a time: a kernel's ceiling here is its measured count rounded up to its
granule, plus one granule more."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'chainer-vq-vae_amd', 'csrc', 'code_stats.hip')
HEADER = os.path.join(ROOT, 'include', 'vqvae_codes.h')
GRANULE = 8
MEASURED = {'codes_runs_kernel': (33, 2 * 256 * 4), 'codes_hist_kernel': (14, 0), 'codes_agree_kernel': (19, 256 * 4),
            'codes_edit_kernel': (19, 0)}                    # registers, bytes of static LDS


@pytest.fixture(scope='module')
def codes_meta(tmp_path_factory):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    out = str(tmp_path_factory.mktemp('codes') / 'code_stats.s')
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-S',
                           '--cuda-device-only', SRC, '-o', out], stderr=subprocess.DEVNULL)
    meta = {}
    for m in re.finditer(r'\.agpr_count:\s*(\d+).*?\.group_segment_fixed_size:\s*(\d+).*?\.name:\s*(\S+)'
                         r'.*?\.private_segment_fixed_size:\s*(\d+).*?\.vgpr_count:\s*(\d+).*?\.vgpr_spill_count:\s*(\d+)',
                         open(out).read(), re.S):
        if 'codes_' in m.group(3):
            meta[m.group(3)] = dict(agpr=int(m.group(1)), lds=int(m.group(2)), scratch=int(m.group(4)),
                                    vgpr=int(m.group(5)), spill=int(m.group(6)))
    return meta


def test_every_launched_kernel_is_compiled_without_scratch(codes_meta, record_property):
    launched = set(re.findall(r'hipLaunchKernelGGL\(\(?(\w+)', open(SRC).read()))
    assert launched == set(MEASURED)
    for name, (vgpr, lds) in MEASURED.items():
        hits = [v for n, v in codes_meta.items() if name in n]
        assert len(hits) == 1, '%s is not in the compiled module' % name
        m = hits[0]
        record_property(name, '%(vgpr)d registers (%(agpr)d accumulation), %(lds)d bytes of static LDS' % m)
        print('%s: %r' % (name, m))
        assert (m['scratch'], m['spill']) == (0, 0), (name, m)
        assert m['agpr'] == 0 and m['vgpr'] <= -(-vgpr // GRANULE) * GRANULE + GRANULE, (name, m)
        assert m['lds'] == lds, (name, m)


def test_dynamic_lds_is_within_a_cu_at_the_bound():
    """The launch's formula restated: 3 diagonals * (4 + 4) bytes * max_short, under the 144 KiB the alignment's DP asks
    for, which the 160 KiB of a compute unit allow."""
    text, header = open(SRC).read(), open(HEADER).read()
    assert 'CS_LDS_CAP = 160 * 1024' in text and 'CS_CELL_BYTES = 3 * 2 * sizeof(int)' in text
    assert 'const size_t lds = CS_CELL_BYTES * (size_t)d->max_short;' in text
    bound = int(re.search(r'#define VQVAE_CODES_MAX_SHORT (\d+)', header).group(1))
    assert bound == 6143
    assert 24 * bound == 147432 <= 144 * 1024 <= 160 * 1024 and 24 * (bound + 2) > 144 * 1024
    assert 24 * 400 == 9600                                  # a typical pair: many workgroups share a compute unit
