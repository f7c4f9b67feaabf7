"""Callers hold workspaces across calls and the recorded step bakes their sizes in: every *_workspace_bytes /
*_packed_bytes export keeps returning the byte count recorded in tests/golden/workspace_bytes.json, for every shape of
the grid below.  The queries are host arithmetic (no device), so the numbers are the same on every machine; the one
query whose answer consults the device (vqvae_wavenet_gen_run_workspace_bytes) is left out.

    python tests/test_host_workspace_bytes.py        re-records the file from the built library
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'workspace_bytes.json')


def _rb(B, T, C_, Cs, Cc, K=2, storage=0):
    return [B, T, C_, C_, Cs, Cc, K, 1, storage]          # ResblockDesc: B T Cr Cd Cs Cc K dil storage


def _grid():
    """[(export, matmul mode, [int arguments; a desc's fields come first])]"""
    g = []
    # (B, T, d, k, decoder channels, skip channels, condition channels, blocks): BASELINE configs[0], [1] / [2] per GPU,
    # [4] (mixture of logistics, 40 blocks), the default model, the small model of the tests
    models = [(1, 7680, 64, 512, 256, 256, 192, 20), (16, 7680, 64, 512, 256, 256, 192, 20),
              (16, 7680, 64, 512, 256, 256, 192, 40), (4, 7680, 512, 128, 512, 512, 640, 30),
              (2, 512, 32, 64, 64, 64, 48, 6)]
    for B, T, d, k, Cr, Cs, Cc, nb in models:
        Tl = T // 64
        g.append(('vqvae_vq_workspace_bytes', 2, [B, d, Tl, k]))
        g.append(('vqvae_vq_ema_workspace_bytes', 2, [B, d, Tl, k]))
        g.append(('vqvae_embed_onehot_workspace_bytes', 2, [B, Cr, 256, 2, T]))
        g.append(('vqvae_softmax_xent_workspace_bytes', 2, [B, 256, T]))
        g.append(('vqvae_convstack_workspace_bytes', 2, [5, B, d]))
        g.append(('vqvae_conv_s2_bwd_workspace_bytes', 2, [B, d, T // 2]))
        for storage in (0, 1):
            g.append(('vqvae_resblock_workspace_bytes', 2, _rb(B, T, Cr, Cs, Cc, 2, storage)))
            g.append(('vqvae_resstack_packed_bytes', 2, _rb(B, T, Cr, Cs, Cc, 2, storage)))
        for n in (1, 2, 3, 4, 6, 8, 12, 13):
            g.append(('vqvae_resstack_dil_wgrad_workspace_bytes', 2, _rb(B, T, Cr, Cs, Cc) + [n]))
        for mode in (0, 1, 2, 3):
            # the encoder's first and later stages, the decoder's output projections, the stacked condition projection
            for Cin, Cout, Tin, K, stride in ((1, d, T, 4, 2), (d, d, T // 2, 4, 2), (Cs, Cs, T, 1, 1), (Cs, 256, T, 1, 1),
                                              (Cc, nb * Cr, Tl, 1, 1)):
                pad = 1 if stride == 2 else 0
                desc = [B, Cin, Tin, Cout, (Tin + 2 * pad - K) // stride + 1, K, stride, pad, 1, 0]
                g.append(('vqvae_conv1d_workspace_bytes', mode, desc))
                for backward in (0, 1):
                    g.append(('vqvae_conv1d_packed_bytes', mode, desc + [backward]))
    for n in range(1, 26):                                  # every group size, and one beyond the 24 supported
        g.append(('vqvae_resstack_workspace_bytes', 2, _rb(16, 7680, 256, 256, 192) + [n]))
        g.append(('vqvae_resstack_workspace_bytes', 2, _rb(4, 7680, 512, 512, 640) + [n]))
    for n in (1, 5, 24):
        g.append(('vqvae_resstack_workspace_bytes', 2, _rb(3, 1001, 96, 80, 40) + [n]))
    # the VQ stress shape (configs[3]), odd T, odd d, both sides of the large-N gradient's threshold
    for B, d, T, k in ((16, 128, 65535, 8192), (1, 128, 1920, 8192), (3, 7, 121, 33), (1, 1, 1, 1), (5, 255, 333, 512),
                       (2, 64, 4097, 512), (16, 64, 8191, 4096)):
        g.append(('vqvae_vq_workspace_bytes', 2, [B, d, T, k]))
        g.append(('vqvae_vq_ema_workspace_bytes', 2, [B, d, T, k]))
    # generic conv: K 1..4, stride 1 and 2, odd lengths and channel counts, every matmul mode
    for mode in (0, 1, 2, 3):
        for K in (1, 2, 3, 4):
            for stride in (1, 2):
                for B, Cin, Cout, Tin in ((2, 48, 80, 1001), (16, 256, 256, 7680), (1, 3, 130, 64)):
                    Tout = (Tin + 2 - K) // stride + 1
                    desc = [B, Cin, Tin, Cout, Tout, K, stride, 1, 1, 0]
                    g.append(('vqvae_conv1d_workspace_bytes', mode, desc))
                    g.append(('vqvae_conv1d_packed_bytes', mode, desc + [K % 2]))
    for B, Cout, q, K, T in ((3, 48, 256, 2, 1001), (1, 64, 10, 1, 7), (16, 512, 256, 2, 7680), (2, 64, 256, 3, 512)):
        g.append(('vqvae_embed_onehot_workspace_bytes', 2, [B, Cout, q, K, T]))
    for L, B, Cc in ((1, 1, 64), (3, 7, 64), (5, 128, 128), (5, 4, 512)):
        g.append(('vqvae_convstack_workspace_bytes', 2, [L, B, Cc]))
        g.append(('vqvae_conv_s2_bwd_workspace_bytes', 2, [B, Cc, 1001]))
    seen, out = set(), []
    for e in g:
        key = json.dumps(e)
        if key not in seen:
            seen.add(key)
            out.append(e)
    return out


def _query(lib, _lib, fn, mode, args):
    assert lib.vqvae_set_matmul_dtype(mode) == 0
    proto = getattr(lib, fn).argtypes
    if proto and proto[0] in (C.POINTER(_lib.Conv1dDesc), C.POINTER(_lib.ResblockDesc)):
        desc = proto[0]._type_
        nf = len(desc._fields_)
        return int(getattr(lib, fn)(C.byref(desc(*args[:nf])), *args[nf:]))
    return int(getattr(lib, fn)(*args))


def _replay():
    from vqvae_amd import _lib
    lib = _lib.load()
    before = lib.vqvae_get_matmul_dtype()
    try:
        return [[fn, mode, args, _query(lib, _lib, fn, mode, args)] for fn, mode, args in _grid()]
    finally:
        lib.vqvae_set_matmul_dtype(before)


def test_workspace_queries_return_the_recorded_sizes():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = _replay()
    assert [e[:3] for e in got] == [e[:3] for e in want], 'the grid and the recorded file list different queries'
    assert len(want) >= 300 and any(e[3] > 0 for e in want)
    bad = [(g, w[3]) for g, w in zip(got, want) if g[3] != w[3]]
    assert not bad, 'workspace sizes moved (query, recorded): %r' % bad[:10]


if __name__ == '__main__':
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'chainer-vq-vae_amd'))
    with open(GOLDEN, 'w') as f:
        f.write('[\n' + ',\n'.join(json.dumps(e) for e in _replay()) + '\n]\n')
