"""The 'wide' shape class of the float32x2 pre-split chain (the reference's default decoder: 512 residual / dilated
channels) as far as it can be checked without a GPU: the capability query's domain, and the register / LDS budget of the
kernel built for it, from the compiled code object's metadata."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_BITS = 32 | 64 | 128 | 256     # VQVAE_STORE_GH_F16X2 | X_F16X2 | RES_F16X2 | GATES_SIG


def _desc(_lib, B=4, T=7680, Cr=512, Cd=512, Cs=256, Cc=640, K=2, dil=512):
    return _lib.ResblockDesc(B, T, Cr, Cd, Cs, Cc, K, dil, 0)


def test_wide_blocks_are_offered_every_presplit_bit():
    """vqvae_resblock_f16x2_storage for the params.py decoder block (Cr = Cd = 512, Cs = 256, K = 2, B = 4, T = 7680):
    all four bits in matmul mode 3; none with vqvae_set_presplit(0), in modes 0 / 1 / 2, for T % 128 != 0, for other
    channel counts, for a dilation beyond the sequence or a batch beyond the 32-bit offsets.  Cs = 512 is in the class;
    the 256-channel answer is what it was.  check_rb accepts what the query offers (a workspace query goes through it)."""
    from vqvae_amd import _lib
    lib = _lib.load()
    q = lambda d: lib.vqvae_resblock_f16x2_storage(C.byref(d))
    mode0 = lib.vqvae_get_matmul_dtype()
    try:
        assert lib.vqvae_set_matmul_dtype(3) == 0
        assert q(_desc(_lib)) == ALL_BITS
        assert q(_desc(_lib, Cs=512)) == ALL_BITS
        assert q(_desc(_lib, dil=1)) == ALL_BITS
        for mask in range(8):
            assert lib.vqvae_set_presplit(mask) == 0
            want = (32 if mask & 1 else 0) | (192 if mask & 2 else 0) | (256 if mask & 4 else 0)
            assert q(_desc(_lib)) == want, mask
            assert q(_desc(_lib, 16, 7680, 256, 256, 256, 192)) == want, mask
        lib.vqvae_set_presplit(7)
        assert q(_desc(_lib, T=7680 + 64)) == 0
        assert q(_desc(_lib, Cr=384)) == 0
        assert q(_desc(_lib, Cd=384)) == 0
        assert q(_desc(_lib, Cs=128)) == 0
        assert q(_desc(_lib, K=3)) == 0
        assert q(_desc(_lib, T=256, dil=256)) == 0
        assert q(_desc(_lib, B=140)) == 0                   # 140 * 512 * 7680 * 4 bytes >= 2^31
        d = _desc(_lib)
        d.storage = ALL_BITS
        assert lib.vqvae_resblock_workspace_bytes(C.byref(d)) > 0
        assert lib.vqvae_get_fused_pullback(C.byref(_desc(_lib))) == 0
        assert lib.vqvae_get_fused_pullback(C.byref(_desc(_lib, 16, 7680, 256, 256, 256, 192))) == 1
        for mode in (0, 1, 2):
            assert lib.vqvae_set_matmul_dtype(mode) == 0
            assert q(_desc(_lib)) == 0, mode
            assert lib.vqvae_get_fused_pullback(C.byref(_desc(_lib, 16, 7680, 256, 256, 256, 192))) == 0
    finally:
        lib.vqvae_set_presplit(7)
        lib.vqvae_set_matmul_dtype(mode0)


def test_wide_streaming_kernel_budget(tmp_path):
    """lin256_stream_kernel keeps a wave's 32 x 256 slice of Wr in registers (128 VGPRs of A fragments): both
    instantiations fit the 256 VGPRs of two waves per SIMD without a spill or scratch, with two 32 KB z images + 1 KB of
    biases in LDS, and every buffer access keeps its row offset in SGPRs (no waterfall loop around a load)."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    src = os.path.join(ROOT, 'chainer-vq-vae_amd', 'csrc', 'lin_stream_wide.hip')
    out = str(tmp_path / 'lin_stream_wide.s')
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off',
                           '-S', '--cuda-device-only', src, '-o', out], stderr=subprocess.DEVNULL)
    text = open(out).read()
    hits = {}
    for m in re.finditer(r'\.group_segment_fixed_size:\s*(\d+).*?\.name:\s*(\S+).*?\.private_segment_fixed_size:\s*(\d+)'
                         r'.*?\.vgpr_count:\s*(\d+).*?\.vgpr_spill_count:\s*(\d+)', text, re.S):
        if 'lin256_stream_kernel' in m.group(2):
            hits[m.group(2)] = tuple(int(m.group(i)) for i in (1, 3, 4, 5))
    assert len(hits) == 2, hits                            # x_l fp32 (the stack's first block) / pre-split
    for name, (lds, scratch, vgpr, spills) in hits.items():
        assert (scratch, spills) == (0, 0), (name, scratch, spills)
        assert 128 < vgpr <= 232, (name, vgpr)
        assert lds in (2 * 32768 + 1024, 2 * 32768 + 1024 + 64), (name, lds)      # (+ 64 B: amax_commit's reduction)
    assert 's_cbranch_execnz' not in text
    assert text.count('v_mfma_f32_32x32x16_f16') == 2 * 2 * 16 * 3      # two instantiations x two unrolled tiles x 16 steps x 3 products
