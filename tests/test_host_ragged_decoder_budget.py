"""CPU check of the ragged decoder kernels' compiled resources (csrc/ragged_decoder.hip), read from the code object's
metadata as tests/test_host_ragged_budget.py does.  The GEMM kernels keep the next channel group's operands in registers
while the matrix pipe works; an array moved to scratch would leave every parity test green and the launch several times
slower.  Bounds, from the register file alone (512 registers per SIMD lane, accumulation registers included in vgpr_count):
the 64 x 64-tile kernels keep three waves per SIMD (512 / 3, allocated in eights: 168), the 128 x 128-tile kernels two
(256).  All LDS is dynamic, sized at the launch."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN, GATE, RESSKIP, HEAD = range(4)
# (mode, T2, epilogue) of every instantiation the entry points launch
LAUNCHED = [(m, t2, e) for m in (0, 3) for t2, e in ((1, PLAIN), (2, PLAIN), (2, GATE), (1, RESSKIP), (2, RESSKIP), (1, HEAD))]


@pytest.fixture(scope='module')
def meta(tmp_path_factory):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    src = os.path.join(ROOT, 'chainer-vq-vae_amd', 'csrc', 'ragged_decoder.hip')
    out = str(tmp_path_factory.mktemp('rdec') / 'ragged_decoder.s')
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-S',
                           '--cuda-device-only', src, '-o', out], stderr=subprocess.DEVNULL)
    found = {}
    for m in re.finditer(r'\.agpr_count:\s*(\d+).*?\.group_segment_fixed_size:\s*(\d+).*?\.name:\s*(\S+)'
                         r'.*?\.private_segment_fixed_size:\s*(\d+).*?\.vgpr_count:\s*(\d+).*?\.vgpr_spill_count:\s*(\d+)',
                         open(out).read(), re.S):
        if 'rd_' in m.group(3):
            found[m.group(3)] = dict(agpr=int(m.group(1)), lds=int(m.group(2)), scratch=int(m.group(4)),
                                     vgpr=int(m.group(5)), spill=int(m.group(6)))
    return found


def test_every_launched_instantiation_is_compiled_without_scratch(meta, record_property):
    gemms = [n for n in meta if 'rd_gemm_kernel' in n]
    assert len(gemms) == len(LAUNCHED), sorted(gemms)
    for mode, t2, epi in LAUNCHED:
        hits = [v for n, v in meta.items() if 'rd_gemm_kernelILi%dELi%dELi%dEE' % (mode, t2, epi) in n]
        assert len(hits) == 1, 'rd_gemm_kernel<%d, %d, %d> is not in the compiled module' % (mode, t2, epi)
        m = hits[0]
        record_property('rd_gemm_kernel_%d_%d_%d' % (mode, t2, epi), '%(vgpr)d registers (%(agpr)d accumulation)' % m)
        assert (m['scratch'], m['spill']) == (0, 0), (mode, t2, epi, m)
        assert m['agpr'] <= m['vgpr'] <= (168 if t2 == 1 else 256), (mode, t2, epi, m)
        assert m['lds'] == 0, (mode, t2, epi, m)
    for name in ('rd_embed_kernel', 'rd_gvec_kernel', 'rd_reduce_kernel'):
        hits = [v for n, v in meta.items() if name in n]
        assert len(hits) == 1 and (hits[0]['scratch'], hits[0]['spill']) == (0, 0), (name, hits)
        assert hits[0]['vgpr'] <= 64 and hits[0]['lds'] <= 4096, (name, hits)
