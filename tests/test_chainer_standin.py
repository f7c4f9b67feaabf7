"""Self-check of tests/golden/chainer_standin.py, the Chainer stand-in the reference-model fixtures were
computed on.  Dev container only: needs torch, and for the VQ check the reference checkout;
the tests skip where either is missing.  torch is imported when a test runs, not at collection (see
test_oracle_torch.py for why)."""
import os
import sys

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
REF = '/root/reference'


@pytest.fixture
def standin():
    """The stand-in installed in sys.modules for one test, and everything it brought removed afterwards."""
    pytest.importorskip('torch')
    before_modules, before_path = set(sys.modules), list(sys.path)
    sys.path.insert(0, GOLD)
    import chainer_standin as S
    S.install()
    S.set_dtype(np.float64)
    yield S
    S.set_dtype(np.float64)
    for name in set(sys.modules) - before_modules:
        if name == 'chainer' or name.startswith('chainer.') or name in ('chainer_standin', 'six', 'librosa', 'utils'):
            del sys.modules[name]
    sys.path[:] = before_path


@pytest.mark.parametrize('name', ['vq_train.npz', 'vq_3d.npz', 'vq_ties.npz'])
def test_reference_vq_through_function_node_apply_is_bit_exact(standin, name):
    """utils.VQ / straight_through run through FunctionNode.apply inside the autograd graph, in float32, on the
    inputs of the committed VQ fixtures (which make_golden.py computed by calling forward / backward directly):
    idx, e and gW come out bit for bit."""
    if not os.path.isfile(os.path.join(REF, 'utils.py')):
        pytest.skip('the reference checkout is not on this machine')
    import types
    sys.modules.setdefault('librosa', types.ModuleType('librosa'))
    sys.path.insert(0, REF)
    import utils
    S = standin
    S.set_dtype(np.float32)
    g = np.load(os.path.join(GOLD, name))
    vq = utils.VQ(g['W'].shape[0], g['W'].shape[1])
    assert [n for n, _ in vq.namedparams()] == ['/W'] and vq.W.shape == g['W'].shape
    vq.W.array = g['W']
    z = S.Variable(g['z'])
    e = vq(z)
    assert e.dtype == np.float32
    np.testing.assert_array_equal(e.data, g['e'])
    np.testing.assert_array_equal(g['W'][g['idx']].reshape(-1, g['W'].shape[1]),
                                  np.moveaxis(g['e'].reshape(g['e'].shape[:3]), 1, 2).reshape(-1, g['W'].shape[1]))
    loss = (e * S.Variable(g['gy'], requires_grad=False))
    loss.backward()                                       # seeds ones: d/de = gy
    np.testing.assert_array_equal(vq.W.grad, g['gW'])
    np.testing.assert_array_equal(z.grad, g['gy'])        # straight through: gx is gy
    node = utils.StraightThrough()
    node.apply((S.Variable(g['z']), vq.W))
    np.testing.assert_array_equal(node.indexes, g['idx'])


def test_variable_semantics(standin):
    """backward() seeds 1 and accumulates; ``+=`` rebinds; a Variable made from .data is a detached leaf."""
    S = standin
    x = S.Variable(np.array([1.0, 2.0, 3.0]))
    y = (x * x * 2.0)
    y.backward()
    np.testing.assert_array_equal(x.grad, [4.0, 8.0, 12.0])
    (x * 3.0).backward()
    np.testing.assert_array_equal(x.grad, [7.0, 11.0, 15.0])          # accumulated
    x.cleargrad()
    assert x.grad is None
    h = keep = x * 1.0
    h += S.Variable(np.ones(3))
    assert h is not keep and (keep.data == [1, 2, 3]).all() and (h.data == [2, 3, 4]).all()
    cut = S.Variable(keep.data)
    (cut * x).backward()
    np.testing.assert_array_equal(x.grad, [1.0, 2.0, 3.0])           # nothing flowed through ``cut``
    assert (np.ones(3, np.float32) * x).dtype == np.float64 and (2.0 - x).shape == (3,)
    assert x.reshape((3, 1)).shape == (3, 1) and x.reshape(1, 3).transpose((1, 0)).shape == (3, 1)


def test_link_names_order_lazy_shapes_pad_and_deepcopy(standin):
    import copy
    import chainer
    import chainer.links as L

    class Block(chainer.Chain):
        def __init__(self):
            super(Block, self).__init__()
            with self.init_scope():
                self.conv = L.DilatedConvolution2D(None, 4, ksize=(2, 1), pad=(2, 0), dilate=(2, 1))
                self.alpha = L.Convolution2D(4, 4, 1)

    class Net(chainer.Chain):
        def __init__(self):
            super(Net, self).__init__()
            with self.init_scope():
                self.zeta = L.EmbedID(3, 2)
                self.resnet = chainer.ChainList()
                self.after = L.Convolution2D(1, 2, (4, 1), (2, 1), (1, 0))
            self.resnet.add_link(Block())
            self.resnet.add_link(Block())
    net = Net()
    names = [n for n, _ in net.namedparams()]
    assert names == ['/zeta/W', '/resnet/0/conv/W', '/resnet/0/conv/b', '/resnet/0/alpha/W', '/resnet/0/alpha/b',
                     '/resnet/1/conv/W', '/resnet/1/conv/b', '/resnet/1/alpha/W', '/resnet/1/alpha/b',
                     '/after/W', '/after/b']                          # registration order, not sorted
    conv = net.resnet[0].conv
    assert conv.W.data is None                                        # lazy
    x = chainer.Variable(np.arange(2 * 3 * 5, dtype=np.float64).reshape(2, 3, 5, 1))
    assert conv(x).shape == (2, 4, 7, 1) and conv.W.shape == (4, 3, 2, 1)
    conv.pad = (0, 0)                                                 # read at call time
    assert conv(x).shape == (2, 4, 3, 1)
    assert net.after.W.shape == (2, 1, 4, 1) and net.after(x[:, :1]).shape == (2, 2, 2, 1)
    twin = copy.deepcopy(net)
    twin.after.W.array = np.ones((2, 1, 4, 1))
    assert not net.after.W.data.any() and [n for n, _ in twin.namedparams()] == names
    net.after(x[:, :1]).backward()
    assert net.after.W.grad is not None and twin.after.W.grad is None
    net.cleargrads()
    assert net.after.W.grad is None


def test_resize_images_is_appendix_b(standin):
    """F.resize_images along the time axis equals the oracle's align-corners tables (both written from SURVEY
    Appendix B), and a length-1 axis is a broadcast."""
    sys.path.insert(0, os.path.join(os.path.dirname(GOLD), os.pardir, 'oracle'))
    import chainer.functions as F
    import vqvae_oracle as O
    rs = np.random.RandomState(3)
    x = rs.standard_normal((2, 3, 8))
    y = F.resize_images(standin.Variable(x[..., None]), (512, 1))
    np.testing.assert_allclose(y.data[..., 0], O.upsample_fwd(x, 512), rtol=0, atol=1e-14)
    g = F.resize_images(standin.Variable(x[:, :, :1, None]), (9, 1))
    np.testing.assert_array_equal(g.data[..., 0], np.broadcast_to(x[:, :, :1], (2, 3, 9)))
