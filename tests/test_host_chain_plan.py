"""The storage plan of ResidualNet's chain (vqvae_amd.wavenet._plan_storage) over the shapes its predicates split, as far
as it can be checked without a GPU: vqvae_resblock_bf16_storage / vqvae_resblock_f16x2_storage are host-only queries, so
the real planner runs on real descriptors and the plan is held to what the library can execute.

The invariants: a block is never handed a bit the library does not offer ITS descriptor (check_rb would reject the
launch); what block l writes its residual output as is what block l + 1 reads its input as, likewise the gradient stream
gx_{l+1} = g_res_l; the ends of the chain have no stream bit; a block that reads a stored x stores its residual output
(rb_formats: that pair of formats is not built); gh_l is stored only where a pull-back to the latent rate reads it stored
(fused into the gate-derivative launch, or inside the segmented kernel's domain); the backward bits contain the forward
bits."""
import ctypes as C
import itertools

import pytest

X16, RES16, GX16, GRES16, GH16 = 2, 4, 8, 16, 1             # VQVAE_STORE_*_BF16
GHX2, XX2, RESX2, GSIG = 32, 64, 128, 256                   # VQVAE_STORE_*_F16X2, VQVAE_STORE_GATES_SIG

CHANNELS = [(256, 256, 128), (256, 256, 256), (256, 256, 512), (512, 512, 256), (512, 512, 512), (64, 64, 64)]   # Cr, Cd, Cs
TS = [64, 128, 192, 256, 384, 512, 1000, 1024, 2048]
DILS = [[1], [1, 2], [2 ** (i % 10) for i in range(20)], [512, 1], [1, 512, 1]]
# (matmul mode, presplit mask, wavenet.BF16_STORAGE): the mask matters in mode 3 only, the switch in mode 1 only
VARIANTS = [(0, 7, True), (2, 7, True), (1, 7, True), (1, 7, False)] + [(3, m, True) for m in range(8)]


def _x_fmt(bits):
    return 'bf16' if bits & X16 else ('pre-split' if bits & XX2 else 'none')


def _res_fmt(bits):
    return 'bf16' if bits & RES16 else ('pre-split' if bits & RESX2 else 'none')


def _accepted(lib, d):
    """Does check_rb accept d.storage?  A weight-gradient call over zero blocks stops at its argument check, behind check_rb
    and in front of anything that touches a device: the error text says which of the two refused it."""
    rc = lib.vqvae_resstack_dil_wgrad(C.byref(d), 0, None, None, None, None, None, 0, None, 0, None, None, None)
    assert rc != 0
    return b'desc.storage' not in lib.vqvae_last_error_string()


def _latents(T):
    """Latent lengths per T: the configs' up-sampling (64) and a ratio below the segmented pull-back's 8."""
    return [max(2, T // 64), max(2, T // 4)]


def check_plan(lib, _lib, descs, fwd, bwd, Tl, bf16_on=True):
    """The invariants of one plan; raises AssertionError naming the block."""
    nb, d0 = len(descs), descs[0]
    fused = lib.vqvae_get_matmul_dtype() == 3 and d0.Cd == 256 and d0.T % 128 == 0 and d0.T >= 64 * Tl
    segmented = Tl >= 3 and d0.T >= 8 * Tl and d0.T % 4 == 0 and d0.T // 4 <= 2048
    assert fused or segmented or not any(b & (GH16 | GHX2) for b in bwd), \
        'a stored gh with T = %d over Tl = %d: no pull-back reads it (%s)' % (d0.T, Tl, bwd)
    assert len(fwd) == len(bwd) == nb
    for name, plan in (('forward', fwd), ('backward', bwd)):
        for l, (d, bits) in enumerate(zip(descs, plan)):
            off = lib.vqvae_resblock_bf16_storage(C.byref(d)) | lib.vqvae_resblock_f16x2_storage(C.byref(d))
            assert bits & ~off == 0, '%s: block %d (dil %d) is handed %d, offered %d' % (name, l, d.dil, bits, off)
            if not bf16_on:
                assert bits & (X16 | RES16 | GX16 | GRES16 | GH16) == 0, (name, l, bits)
            probe = _lib.ResblockDesc.from_buffer_copy(d)
            probe.storage = bits
            assert lib.vqvae_resblock_workspace_bytes(C.byref(probe)) > 0
            assert _accepted(lib, probe), '%s: check_rb rejects block %d (dil %d) with storage %d' % (name, l, d.dil, bits)
            assert not (bits & X16 and bits & XX2) and not (bits & RES16 and bits & RESX2), (name, l, bits)
        for l in range(nb - 1):
            assert _res_fmt(plan[l]) == _x_fmt(plan[l + 1]), \
                '%s: block %d writes its residual output as %s, block %d reads its input as %s (dils %s)' % (
                    name, l, _res_fmt(plan[l]), l + 1, _x_fmt(plan[l + 1]), [d.dil for d in descs])
            assert _x_fmt(plan[l]) == 'none' or _res_fmt(plan[l]) == _x_fmt(plan[l]), \
                '%s: block %d reads a stored x and writes an fp32 residual output: no kernel does' % (name, l)
        assert _x_fmt(plan[0]) == 'none' and _res_fmt(plan[-1]) == 'none', (name, plan[0], plan[-1])
    for l in range(nb - 1):
        assert bool(bwd[l] & GRES16) == bool(bwd[l + 1] & GX16), 'g_res of block %d / gx of block %d' % (l, l + 1)
    assert not bwd[0] & GX16 and not bwd[-1] & GRES16
    assert all(f & ~(GX16 | GRES16 | GH16 | GHX2) == f for f in fwd), fwd          # no gradient tensor in the forward bits
    assert all(b & f == f for f, b in zip(fwd, bwd)), (fwd, bwd)


@pytest.mark.parametrize('variant', VARIANTS, ids=lambda v: 'mode%d-mask%d-%s' % (v[0], v[1], 'bf16' if v[2] else 'nobf16'))
def test_plan_is_executable_and_consistent_over_the_grid(variant):
    """Every (channels, T, dilation list) of the grid in one matmul mode / presplit mask / BF16_STORAGE setting."""
    from vqvae_amd import _lib, wavenet
    lib = _lib.load()
    mode, mask, bf16_on = variant
    mode0, sw0 = lib.vqvae_get_matmul_dtype(), wavenet.BF16_STORAGE
    stored = 0
    try:
        assert lib.vqvae_set_matmul_dtype(mode) == 0 and lib.vqvae_set_presplit(mask) == 0
        wavenet.BF16_STORAGE = bf16_on
        for (Cr, Cd, Cs), T, dils in itertools.product(CHANNELS, TS, DILS):
            for Tl in _latents(T):
                descs = [_lib.ResblockDesc(2, T, Cr, Cd, Cs, 192, 2, dil, 0) for dil in dils]
                fwd, bwd = wavenet._plan_storage(descs, True, mode == 3, Tl)
                try:
                    check_plan(lib, _lib, descs, fwd, bwd, Tl, bf16_on)
                except AssertionError as e:
                    raise AssertionError('mode %d mask %d bf16 %s, Cr %d Cd %d Cs %d, T %d, Tl %d, dils %s: %s'
                                         % (mode, mask, bf16_on, Cr, Cd, Cs, T, Tl, dils, e))
                assert all(d.storage == 0 for d in descs)                    # the planner only reads the descriptors
                stored += sum(1 for b in bwd if b)
                assert wavenet._plan_storage(descs, False, False) == ([0] * len(dils), [0] * len(dils))    # pack per call: nothing stored
        # the grid is not vacuous: the modes that store anything do so somewhere on it
        assert (stored > 0) == ((mode == 3 and mask != 0) or (mode == 1 and bf16_on)), (variant, stored)
    finally:
        wavenet.BF16_STORAGE = sw0
        lib.vqvae_set_presplit(7)
        lib.vqvae_set_matmul_dtype(mode0)


def test_plan_around_a_block_refused_presplit_storage():
    """'float32x2', 256 channels, T = 384, dilations 1 .. 512, 1, 2 (block 9: dil 512 >= T, offered nothing): the blocks in
    front of it keep an fp32 stream (a stored x with an fp32 output is not built, so the fp32 boundary 8 | 9 reaches back
    to block 0), block 9 stores nothing at all, the stream is pre-split again from 10 | 11 on, and every other block keeps
    its own gh pre-split and its gates as sigmoid + z.  With every dilation inside the sequence (T = 1024) the plan is the
    uniform one: RES on all but the last block, X on all but the first, GH and GATES_SIG everywhere."""
    from vqvae_amd import _lib, wavenet
    lib = _lib.load()
    mode0 = lib.vqvae_get_matmul_dtype()
    dils = [2 ** (i % 10) for i in range(12)]
    try:
        assert lib.vqvae_set_matmul_dtype(3) == 0 and lib.vqvae_set_presplit(7) == 0
        descs = [_lib.ResblockDesc(2, 384, 256, 256, 256, 192, 2, dil, 0) for dil in dils]
        fwd, bwd = wavenet._plan_storage(descs, True, True, descs[0].T // 64)
        assert fwd == [GSIG] * 9 + [0, GSIG | RESX2, GSIG | XX2], fwd
        assert bwd == [GSIG | GHX2] * 9 + [0, GSIG | GHX2 | RESX2, GSIG | GHX2 | XX2], bwd
        descs = [_lib.ResblockDesc(2, 1024, 256, 256, 256, 192, 2, dil, 0) for dil in dils]
        fwd, bwd = wavenet._plan_storage(descs, True, True, descs[0].T // 64)
        assert fwd == [GSIG | RESX2] + [GSIG | RESX2 | XX2] * 10 + [GSIG | XX2], fwd
        assert bwd == [f | GHX2 for f in fwd], bwd
        # the unsupported block first / in the middle of three
        for dl, want in (([512, 1], [0, GSIG]), ([1, 512, 1], [GSIG, 0, GSIG]), ([512, 1, 2], [0, GSIG | RESX2, GSIG | XX2])):
            descs = [_lib.ResblockDesc(2, 256, 256, 256, 256, 192, 2, dil, 0) for dil in dl]
            fwd, bwd = wavenet._plan_storage(descs, True, True, descs[0].T // 64)
            assert fwd == want and bwd == [f | GHX2 if f else 0 for f in fwd], (dl, fwd, bwd)
    finally:
        lib.vqvae_set_presplit(7)
        lib.vqvae_set_matmul_dtype(mode0)


def test_bf16_plan_follows_the_three_predicates():
    """'bfloat16': no bf16 predicate depends on the dilation, so the plan is uniform along a chain and decided by the
    shape: T % 128 == 0 and Cs == Cr: everything; Cs = 512: X / RES / GH without GX / GRES; T % 64 == 0 only: GH alone;
    Cs = 128 (z_bf16 false), T % 64 != 0, 512 channels: nothing.  wavenet.BF16_STORAGE = False: nothing anywhere."""
    from vqvae_amd import _lib, wavenet
    lib = _lib.load()
    mode0, sw0 = lib.vqvae_get_matmul_dtype(), wavenet.BF16_STORAGE

    def plan(T, Cs, Cr=256):
        descs = [_lib.ResblockDesc(2, T, Cr, Cr, Cs, 192, 2, dil, 0) for dil in (256, 512, 1)]
        return wavenet._plan_storage(descs, True, False, T // 64)
    try:
        assert lib.vqvae_set_matmul_dtype(1) == 0
        wavenet.BF16_STORAGE = True
        assert plan(384, 256) == ([RES16, RES16 | X16, X16], [RES16 | GH16 | GRES16, RES16 | X16 | GH16 | GX16 | GRES16, X16 | GH16 | GX16])
        assert plan(512, 512) == ([RES16, RES16 | X16, X16], [RES16 | GH16, RES16 | X16 | GH16, X16 | GH16])
        assert plan(192, 256) == ([0, 0, 0], [GH16] * 3)
        for T, Cs, Cr in ((512, 128, 256), (1000, 256, 256), (512, 256, 512)):
            assert plan(T, Cs, Cr) == ([0, 0, 0], [0, 0, 0]), (T, Cs, Cr)
        wavenet.BF16_STORAGE = False
        assert plan(384, 256) == ([0, 0, 0], [0, 0, 0])
    finally:
        wavenet.BF16_STORAGE = sw0
        lib.vqvae_set_matmul_dtype(mode0)
