"""CPU check of the mixture-of-logistics scoring kernels' compiled resources (csrc/ragged_mol.hip), read from the code object's
metadata as tests/test_host_ragged_decoder_budget.py does.  Both kernels are memory-bound VALU: they should keep four waves
per SIMD of the 512-register file (128 registers), use no scratch and next to no LDS.  rdmol_nll_kernel's component arrays
are indexed by a fully unrolled loop of 16; an array left in scratch would leave every parity test green."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ('rdmol_embed_kernel', 'rdmol_nll_kernel')


@pytest.fixture(scope='module')
def meta(tmp_path_factory):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    src = os.path.join(ROOT, 'chainer-vq-vae_amd', 'csrc', 'ragged_mol.hip')
    out = str(tmp_path_factory.mktemp('rdmol') / 'ragged_mol.s')
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-S',
                           '--cuda-device-only', src, '-o', out], stderr=subprocess.DEVNULL)
    found = {}
    for m in re.finditer(r'\.agpr_count:\s*(\d+).*?\.group_segment_fixed_size:\s*(\d+).*?\.name:\s*(\S+)'
                         r'.*?\.private_segment_fixed_size:\s*(\d+).*?\.vgpr_count:\s*(\d+).*?\.vgpr_spill_count:\s*(\d+)',
                         open(out).read(), re.S):
        found[m.group(3)] = dict(agpr=int(m.group(1)), lds=int(m.group(2)), scratch=int(m.group(4)),
                                 vgpr=int(m.group(5)), spill=int(m.group(6)))
    return found


def test_both_kernels_are_compiled_without_scratch_within_four_waves(meta, record_property):
    assert len(meta) == len(KERNELS), sorted(meta)
    for name in KERNELS:
        hits = [v for n, v in meta.items() if name in n]
        assert len(hits) == 1, '%s is not in the compiled module' % name
        m = hits[0]
        record_property(name, '%(vgpr)d registers (%(agpr)d accumulation), %(lds)d bytes of static LDS' % m)
        print(name, m)
        assert (m['scratch'], m['spill']) == (0, 0), (name, m)
        assert m['lds'] <= 4096, (name, m)
        assert m['agpr'] <= m['vgpr'] <= 128, (name, m)
