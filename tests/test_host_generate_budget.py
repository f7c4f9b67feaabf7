"""CPU check of the persistent generation kernel's compiled resource budget (csrc/generate.hip).  The chain wave's
instruction count is its latency: a private array moved to scratch would multiply a step's time with every parity
test still green, so the metadata of each launched instantiation of gen_mega_kernel is part of the contract."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def mega_meta(tmp_path_factory):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    src = os.path.join(ROOT, 'chainer-vq-vae_amd', 'csrc', 'generate.hip')
    out = str(tmp_path_factory.mktemp('gen') / 'generate.s')
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-S',
                           '--cuda-device-only', src, '-o', out], stderr=subprocess.DEVNULL)
    meta = {}
    for m in re.finditer(r'\.agpr_count:\s*(\d+).*?\.group_segment_fixed_size:\s*(\d+).*?\.name:\s*(\S+)'
                         r'.*?\.private_segment_fixed_size:\s*(\d+).*?\.vgpr_count:\s*(\d+).*?\.vgpr_spill_count:\s*(\d+)',
                         open(out).read(), re.S):
        if 'gen_mega_kernel' in m.group(3):
            meta[m.group(3)] = dict(agpr=int(m.group(1)), lds=int(m.group(2)), scratch=int(m.group(4)),
                                    vgpr=int(m.group(5)), spill=int(m.group(6)))
    return meta


def _inst(meta, cls, nb, exact):
    hits = [v for k, v in meta.items() if cls in k and 'Li%dELb%dE' % (nb, exact) in k]
    assert len(hits) == 1, 'gen_mega_kernel<%s, %d, %d> is not in the compiled module' % (cls, nb, exact)
    return hits[0]


def test_narrow_class_keeps_its_register_and_lds_budget(mega_meta):
    """The 256-channel class is what it was before the kernel grew a width parameter: VGPRs and LDS bytes of
    its four instantiations as compiled from the un-templated source, no accumulation registers, no scratch."""
    want = {(1, 1): (164, 2048), (2, 1): (184, 3584), (4, 1): (244, 6656), (4, 0): (254, 6656)}
    for (nb, exact), (vgpr, lds) in want.items():
        m = _inst(mega_meta, 'MegaNarrow', nb, exact)
        assert (m['vgpr'], m['lds'], m['agpr'], m['scratch'], m['spill']) == (vgpr, lds, 0, 0, 0), (nb, exact, m)


def test_wide_class_runs_without_scratch(mega_meta, record_property):
    """The 512-channel class: no scratch and no spilled VGPR in any instantiation (a scratch reload on the chain
    wave would sit on every dependency edge), at most one wave's 512 registers, and a workgroup's LDS far below
    what two workgroups per CU may take.  The counts are recorded with the test."""
    for nb, exact in ((1, 1), (2, 1), (4, 1), (4, 0)):
        m = _inst(mega_meta, 'MegaWide', nb, exact)
        record_property('MegaWide_%d_%d' % (nb, exact), '%(vgpr)d VGPRs (%(agpr)d accumulation), %(lds)d B LDS' % m)
        assert (m['scratch'], m['spill']) == (0, 0), (nb, exact, m)
        assert m['vgpr'] <= 512 and m['lds'] <= 16 * 1024, (nb, exact, m)
