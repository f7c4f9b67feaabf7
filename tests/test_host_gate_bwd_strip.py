"""CPU check of the column-strip gate-derivative kernel's compiled resource budget (csrc/gate_bwd_strip.hip).  The kernel
is faster than the 128 x 128-tile form because SIXTEEN of its waves share a CU: that needs at most 128 registers per
lane, and one spilled accumulator would put scratch traffic into a kernel that is bound by memory -- with every parity
test still green.  So the metadata of the compiled kernel is part of the contract; the tiled instantiations it stands
beside keep theirs (tests/test_host.py)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'chainer-vq-vae_amd', 'csrc')


@pytest.fixture(scope='module')
def strip_asm(tmp_path_factory):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    out = str(tmp_path_factory.mktemp('strip') / 'gate_bwd_strip.s')
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-S',
                           '--cuda-device-only', os.path.join(CSRC, 'gate_bwd_strip.hip'), '-o', out],
                          stderr=subprocess.DEVNULL)
    return open(out).read()


def _meta(asm):
    hits = [m for m in re.finditer(r'\.agpr_count:\s*(\d+).*?\.group_segment_fixed_size:\s*(\d+).*?\.max_flat_workgroup_size:\s*(\d+)'
                                   r'.*?\.name:\s*(\S+).*?\.private_segment_fixed_size:\s*(\d+).*?\.vgpr_count:\s*(\d+)'
                                   r'.*?\.vgpr_spill_count:\s*(\d+)', asm, re.S) if 'gate_bwd_strip_kernel' in m.group(4)]
    assert len(hits) == 1, 'gate_bwd_strip_kernel is not in the compiled module exactly once'
    m = hits[0]
    return dict(agpr=int(m.group(1)), lds=int(m.group(2)), threads=int(m.group(3)), name=m.group(4), scratch=int(m.group(5)),
                vgpr=int(m.group(6)), spill=int(m.group(7)))


def test_strip_kernel_fits_sixteen_waves_per_cu(strip_asm, record_property):
    m = _meta(strip_asm)
    record_property('gate_bwd_strip_kernel', '%(vgpr)d VGPRs (%(agpr)d accumulation), %(lds)d B LDS, %(threads)d threads' % m)
    assert m['threads'] == 1024, m
    assert m['vgpr'] + m['agpr'] <= 128, m               # 16 waves per CU = 4 per SIMD of 512 registers
    assert (m['spill'], m['scratch']) == (0, 0), m
    assert m['lds'] <= 64 * 1024, m
    # the name tests/test_host.py pins the tiled kernels by must not match this one
    for other in ('conv_gemm_x3_kernel', 'wgrad3_kernel', 'wgrad3_dma_kernel'):
        assert other not in m['name']


def test_strip_kernel_loop_is_matrix_products_and_counted_waits(strip_asm):
    """The K loop (the one backward branch around MFMAs) holds two steps -- g_res and g_skip of a channel group: 24 MFMAs
    (4 row blocks x 3 products of the float32x2 split, twice), two barriers, no scratch access, and no wait that drains
    the memory counter: the loads of the following steps stay in flight."""
    body = strip_asm[strip_asm.index('gate_bwd_strip_kernel'):]
    assert 'scratch_' not in body
    lines = body.splitlines()
    label = {l.split(':')[0].strip(): i for i, l in enumerate(lines) if re.match(r'\.LBB\d+_\d+:', l.strip())}
    loops = []
    for i, l in enumerate(lines):
        m = re.match(r'\s*s_cbranch_\w+\s+(\.LBB\d+_\d+)', l)
        if m and label.get(m.group(1), i) < i:
            span = lines[label[m.group(1)]:i]
            if any('v_mfma' in x for x in span):
                loops.append(span)
    assert len(loops) == 1
    loop = loops[0]
    assert sum('v_mfma_f32_32x32x16_f16' in l for l in loop) == 24
    assert sum(l.strip().startswith('s_barrier') for l in loop) == 2
    assert not any(re.search(r's_waitcnt\s+vmcnt\(0\)', l) for l in loop)


def test_launch_gemm_asks_the_strip_kernel_first():
    """launch_gemm<EPI_GATE_BWD> hands the fused pull-back launch to the strip kernel when its shape test passes and keeps
    the tiled instantiation compiled for every other launch."""
    src = open(os.path.join(CSRC, 'conv_gemm_x3.hip')).read()
    i, j = src.index('gate_bwd_strip_shape(g)'), src.index('conv_gemm_x3_kernel<EPI_GATE_BWD, 2, 1, 2, true, 0, OUTv>')
    assert i < j
    # ... inside select_gemm's ordered list of forms: the strip form is asked before the tiled OUT form is named
    select = src[src.index('static int select_gemm('):src.index('using GemmKernel')]
    assert select.index('gate_bwd_strip_shape(g)') < select.index('f = tiled_form(2, 1, 2, tap2, 0, out, grid)')
    assert 'case GEMM_GATE_STRIP: return launch_gate_bwd_strip(g, tag, st);' in src
    assert 'gate_bwd_strip.hip' in open(os.path.join(CSRC, 'Makefile')).read()
