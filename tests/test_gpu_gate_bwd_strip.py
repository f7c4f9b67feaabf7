"""The column-strip gate-derivative kernel (csrc/gate_bwd_strip.hip) against the 128 x 128-tile kernel it replaces in
ResidualNet's 'float32x2' chain.

wavenet.FUSE_PULLBACK selects the launch: True (the default) asks for the pull-back inside the gate-derivative launch,
which the strip kernel serves for every block that has a g_res; False asks for gh alone, which stays on
conv_gemm_x3_kernel.  Both store gh pre-split under the same bound, so everything that is a function of gh and its
maxima alone -- the input gradient and the dilated-conv / res / skip parameter gradients of every block -- must not
differ in a single bit, whatever the number of tiles (a multiple of a workgroup's four, or not).  What runs through the
pull-back (condition gradients) is summed in another order by the unfused launches and holds the bar of
test_presplit_storage_changes_only_the_rounding_point."""
import numpy as np
import pytest

from helpers import assert_close_scaled, to4
from test_gpu_kernels import _rb_params

pytestmark = pytest.mark.gpu


def _dev(gpu, a):
    return gpu.to_device(np.ascontiguousarray(a))


@pytest.mark.parametrize('B,T', [(16, 7680), (3, 7808), (1, 128 * 64)])
def test_strip_kernel_equals_tiled_kernel(gpu, B, T):
    import vqvae_amd.wavenet as wn
    from vqvae_amd import functions as F
    from vqvae_amd.core import Variable
    gpu.set_matmul_dtype('float32x2')
    dils = [1, 4, 512]
    Tl, Cl, G, nspk = T // 64, 64, 128, 7
    rs = np.random.RandomState(5)
    blocks = [_rb_params(rs, 256, 256, 256, Cl + G, 2) for _ in dils]
    x = rs.standard_normal((B, 256, T)).astype(np.float32)
    local = rs.standard_normal((B, Cl, Tl)).astype(np.float32)
    E = rs.standard_normal((nspk, G)).astype(np.float32)
    ids = rs.randint(0, nspk, B).astype(np.int32)
    gy = rs.standard_normal((B, 256, T)).astype(np.float32)
    order = ['conv', 'condition_proj', 'res', 'skip']

    def run(fuse):
        wn.FUSE_PULLBACK = fuse
        vx = Variable(_dev(gpu, to4(x)))
        vlocal, vE = Variable(_dev(gpu, to4(local))), Variable(_dev(gpu, E))
        vcond = F.condition_assemble(vlocal, vE, _dev(gpu, ids), 64)
        pv = []
        for blk in blocks:
            for n in order:
                pv += [Variable(_dev(gpu, to4(blk[n][0]))), Variable(_dev(gpu, blk[n][1]))]
        fn = wn.ResidualStackFunction(dils)
        skip = fn.apply([vx, vcond] + pv)[0]
        skip.grad = _dev(gpu, to4(gy))
        skip.backward()
        assert all(d.storage & 32 for d in fn.descs), [d.storage for d in fn.descs]      # VQVAE_STORE_GH_F16X2: gh is stored pre-split
        out = {'gx': vx.grad.get(), 'glocal': vlocal.grad.get(), 'gE': vE.grad.get()}
        for i, v in enumerate(pv):
            if v.grad is not None:
                out['block %d %s %s' % (i // 8, order[(i % 8) // 2], 'gb' if i % 2 else 'gW')] = v.grad.get()
        return out
    try:
        strip, tiled = run(True), run(False)
        again = run(True)
    finally:
        wn.FUSE_PULLBACK = True
        gpu.set_matmul_dtype(gpu.default_matmul_dtype())
    assert set(strip) == set(tiled)
    for k in strip:
        assert strip[k].tobytes() == again[k].tobytes(), 'run to run: %s' % k
        if k in ('glocal', 'gE') or 'condition_proj' in k:
            assert_close_scaled(strip[k], tiled[k], 2e-6, k)
        else:
            assert strip[k].tobytes() == tiled[k].tobytes(), '%s differs by %g' % (k, np.abs(strip[k] - tiled[k]).max())
