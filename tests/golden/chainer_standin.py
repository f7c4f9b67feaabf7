"""A stand-in for the ~25 Chainer names the reference touches, on torch-CPU autograd.

Dev-container tooling, our own code: ``install()`` puts ``chainer`` and its
sub-modules (and ``six`` if absent) into ``sys.modules`` so that the reference's ``net.py``,
``WaveNet/modules.py``, ``updaters.py`` and the ``VQ`` / ``ExponentialMovingAverage`` / ``StraightThrough``
parts of ``utils.py`` run UNMODIFIED.  This file never opens the reference's files and holds none of its
lines; only ``make_golden_model.py`` (and the stand-in's self-check) import them, through ``sys.path``.

What running the reference on this pins is its COMPOSITION (which tensor goes where, in which order,
detached or not, cropped at which end).  Every ``F.*`` / ``L.*`` rests on ONE torch operator of published
semantics (table in SURVEY Appendix A); Chainer's own primitives, initialisers and ``Adam`` are not here
and stay [chainer-recalled].

Only what the reference calls exists.  An unused name is an AttributeError, not a guess.
"""
import contextlib
import sys
import types

import numpy as np
import torch

_DTYPE = [torch.float64]


def set_dtype(dtype):
    """The float type every Variable made from an array gets (the fixtures: float64)."""
    _DTYPE[0] = {np.dtype('float32'): torch.float32, np.dtype('float64'): torch.float64}[np.dtype(dtype)]


def _tensor(a):
    """ndarray / scalar / Variable -> torch tensor; floating arrays take the configured dtype."""
    if isinstance(a, Variable):
        return a._t
    if isinstance(a, torch.Tensor):
        return a
    a = np.array(a)                                   # a copy: never aliases the caller's array
    t = torch.from_numpy(a)
    return t.to(_DTYPE[0]) if a.dtype.kind == 'f' else t


# --------------------------------------------------------------------------- #
# Variable / Parameter
# --------------------------------------------------------------------------- #
class Variable(object):
    """Wraps a torch tensor.  A Variable made from an array is a leaf that wants a gradient (Chainer's
    default); one made by a function carries the autograd graph.  No ``__iadd__``: ``h += x`` rebinds
    (SURVEY 9 item 9)."""
    __array_priority__ = 200
    __array_ufunc__ = None                            # ndarray <op> Variable defers to the reflected method

    def __init__(self, data=None, requires_grad=True, name=None):
        self.name = name
        self.requires_grad = requires_grad
        self._t = None
        if data is not None:
            self._set(data)

    def _set(self, data):
        t = _tensor(data).detach().clone()
        if self.requires_grad and t.is_floating_point():
            t.requires_grad_(True)
        self._t = t

    @classmethod
    def _wrap(cls, t):
        v = cls.__new__(cls)
        v.name = None
        v.requires_grad = t.requires_grad
        v._t = t
        return v

    # ---- array access ---- #
    def _get_array(self):
        return None if self._t is None else self._t.detach().numpy()

    def _set_array(self, a):
        self._set(a)
    data = property(_get_array, _set_array)
    array = property(_get_array, _set_array)

    def _get_grad(self):
        return None if self._t is None or self._t.grad is None else self._t.grad.numpy()

    def _set_grad(self, g):
        self._t.grad = None if g is None else _tensor(g)
    grad = property(_get_grad, _set_grad)

    shape = property(lambda s: tuple(s._t.shape))
    ndim = property(lambda s: s._t.dim())
    size = property(lambda s: s._t.numel())
    dtype = property(lambda s: s._get_array().dtype)

    def __len__(self):
        return self._t.shape[0]

    def cleargrad(self):
        if self._t is not None:
            self._t.grad = None
    cleargrads = cleargrad

    def backward(self, retain_grad=False):
        """Seeds 1 and ACCUMULATES into the leaves' existing grads (torch's leaf semantics); the graph is
        kept, because the reference calls backward() on three losses that share a part of it."""
        self._t.backward(torch.ones_like(self._t), retain_graph=True)

    # ---- shape ---- #
    def reshape(self, *shape):
        if len(shape) == 1 and isinstance(shape[0], (tuple, list)):
            shape = tuple(shape[0])
        return Variable._wrap(self._t.reshape(shape))

    def transpose(self, *axes):
        if len(axes) == 1 and isinstance(axes[0], (tuple, list)):
            axes = tuple(axes[0])
        return Variable._wrap(self._t.permute(*axes))

    def __getitem__(self, idx):
        return Variable._wrap(self._t[idx])

    # ---- arithmetic (out of place only) ---- #
    def __neg__(self):
        return Variable._wrap(-self._t)

    def __add__(self, o):
        return Variable._wrap(self._t + _tensor(o))
    __radd__ = __add__

    def __sub__(self, o):
        return Variable._wrap(self._t - _tensor(o))

    def __rsub__(self, o):
        return Variable._wrap(_tensor(o) - self._t)

    def __mul__(self, o):
        return Variable._wrap(self._t * _tensor(o))
    __rmul__ = __mul__

    def __truediv__(self, o):
        return Variable._wrap(self._t / _tensor(o))

    def __rtruediv__(self, o):
        return Variable._wrap(_tensor(o) / self._t)

    def __pow__(self, o):
        return Variable._wrap(self._t ** o)


class Parameter(Variable):
    """``Parameter(initializer)`` is uninitialised (``.data is None``) until ``initialize(shape)`` or an
    array is assigned.  The initialiser's values are NOT Chainer's: the generator loads every parameter
    by name, so they are zeros."""

    def __init__(self, initializer=None, shape=None, name=None):
        Variable.__init__(self, None, True, name)
        if isinstance(initializer, np.ndarray):
            self._set(initializer)
        elif shape is not None:
            self.initialize(shape)

    def initialize(self, shape):
        self._set(np.zeros(shape, np.float64))


# --------------------------------------------------------------------------- #
# FunctionNode: the reference's NumPy forward / backward inside the autograd graph
# --------------------------------------------------------------------------- #
class FunctionNode(object):
    def retain_inputs(self, indexes):
        self._retained = tuple(indexes)

    def get_retained_inputs(self):
        return tuple(Variable(self._in_arrays[i], requires_grad=False) for i in self._retained)

    def apply(self, inputs):
        node = self

        class _Apply(torch.autograd.Function):
            @staticmethod
            def forward(ctx, *ts):
                node._in_arrays = tuple(t.detach().numpy() for t in ts)
                ctx.n_in = len(ts)
                outs = node.forward(node._in_arrays)
                return tuple(torch.from_numpy(np.ascontiguousarray(o)) for o in outs)

            @staticmethod
            def backward(ctx, *gs):
                wanted = tuple(i for i in range(ctx.n_in) if ctx.needs_input_grad[i])
                rets = node.backward(wanted, tuple(Variable._wrap(g.detach()) for g in gs))
                out = [None] * ctx.n_in
                for i, r in zip(wanted, rets):
                    out[i] = _tensor(r).detach().to(torch.from_numpy(node._in_arrays[i]).dtype)
                return tuple(out)
        return tuple(Variable._wrap(t) for t in _Apply.apply(*[_tensor(x) for x in inputs]))


# --------------------------------------------------------------------------- #
# links
# --------------------------------------------------------------------------- #
class Link(object):
    """Parameters and children are remembered in REGISTRATION order; namedparams() yields the link's own
    parameters first, then its children's, with Chainer's '/child/param' paths."""
    xp = np

    def __init__(self):
        self.__dict__['_params'] = []
        self.__dict__['_children'] = []
        self.__dict__['_within_init_scope'] = False
        self.name = None

    @contextlib.contextmanager
    def init_scope(self):
        old = self._within_init_scope
        self.__dict__['_within_init_scope'] = True
        try:
            yield
        finally:
            self.__dict__['_within_init_scope'] = old

    def __setattr__(self, name, value):
        if self.__dict__.get('_within_init_scope'):
            if isinstance(value, Parameter):
                value.name = name
                if name not in self._params:
                    self._params.append(name)
            elif isinstance(value, Link) and isinstance(self, Chain):
                value.name = name
                if name not in self._children:
                    self._children.append(name)
        object.__setattr__(self, name, value)

    def _child_links(self):
        return []

    def children(self):
        for _, c in self._child_links():
            yield c

    def namedparams(self, include_uninit=True):
        for name in self._params:
            p = self.__dict__[name]
            if include_uninit or p.data is not None:
                yield '/' + name, p
        for cname, child in self._child_links():
            for path, p in child.namedparams(include_uninit):
                yield '/' + cname + path, p

    def params(self, include_uninit=True):
        for _, p in self.namedparams(include_uninit):
            yield p

    def cleargrads(self):
        for p in self.params():
            p.cleargrad()


class Chain(Link):
    def _child_links(self):
        return [(n, self.__dict__[n]) for n in self._children]


class ChainList(Link):
    def __init__(self, *links):
        Link.__init__(self)
        self.__dict__['_list'] = []
        for l in links:
            self.add_link(l)

    def add_link(self, link):
        link.name = str(len(self._list))
        self._list.append(link)

    def _child_links(self):
        return [(str(i), l) for i, l in enumerate(self._list)]

    def __getitem__(self, i):
        return self._list[i]

    def __len__(self):
        return len(self._list)


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


class Convolution2D(Link):
    """L.Convolution2D(in, out, ksize, stride=1, pad=0): torch.nn.functional.conv2d (cross-correlation,
    zero padding on both sides).  ``pad`` is read at call time; in_channels=None is lazy."""
    _dilate = 1

    def __init__(self, in_channels, out_channels, ksize=None, stride=1, pad=0, nobias=False):
        Link.__init__(self)
        self.ksize, self.stride, self.pad, self.out_channels = ksize, stride, pad, out_channels
        with self.init_scope():
            self.W = Parameter()
            self.b = None if nobias else Parameter(shape=(out_channels,))
        if in_channels is not None:
            self._initialize_params(in_channels)

    def _initialize_params(self, in_channels):
        self.W.initialize((self.out_channels, in_channels) + _pair(self.ksize))

    def __call__(self, x):
        x = _tensor(x)
        if self.W.data is None:
            self._initialize_params(x.shape[1])
        b = None if self.b is None else self.b._t
        return Variable._wrap(torch.nn.functional.conv2d(
            x, self.W._t, b, stride=_pair(self.stride), padding=_pair(self.pad), dilation=_pair(self._dilate)))


class DilatedConvolution2D(Convolution2D):
    """L.DilatedConvolution2D(in, out, ksize, stride=1, pad=0, dilate=1): conv2d with ``dilation``."""

    def __init__(self, in_channels, out_channels, ksize=None, stride=1, pad=0, dilate=1, nobias=False):
        self.__dict__['_dilate'] = dilate
        Convolution2D.__init__(self, in_channels, out_channels, ksize, stride, pad, nobias)
        self.dilate = dilate


class EmbedID(Link):
    """L.EmbedID(n, d): torch.nn.functional.embedding (row lookup, scatter-add backward)."""

    def __init__(self, in_size, out_size):
        Link.__init__(self)
        with self.init_scope():
            self.W = Parameter(shape=(in_size, out_size))

    def __call__(self, ids):
        return Variable._wrap(torch.nn.functional.embedding(_tensor(ids).long(), self.W._t))


# --------------------------------------------------------------------------- #
# functions
# --------------------------------------------------------------------------- #
def _unary(op):
    return lambda x: Variable._wrap(op(_tensor(x)))


def _split_axis(x, indices_or_sections, axis):
    x = _tensor(x)
    if not isinstance(indices_or_sections, int):
        raise NotImplementedError('split_axis: the reference splits into equal sections only')
    if x.shape[axis] % indices_or_sections:
        raise ValueError('split_axis: not divisible')
    return tuple(Variable._wrap(t) for t in torch.split(x, x.shape[axis] // indices_or_sections, dim=axis))


def _concat(xs, axis=1):
    return Variable._wrap(torch.cat([_tensor(x) for x in xs], dim=axis))


def _resize_tables(n, out_n, dtype):
    # u = linspace(0, n-1, out_n); u0 = floor(u).clip(0, n-2); u1 = u0 + 1; weights
    # (u1 - u), (u - u0) computed in float64 and cast.  With n == 1 NumPy's clip(0, -1) gives -1, which
    # wraps to the only element with weight 0 while u1 = 0 gets weight 1.
    u = np.linspace(0, n - 1, num=out_n)
    u0 = np.floor(u).astype(np.int64).clip(0, n - 2)
    u1 = u0 + 1
    w0 = torch.from_numpy(u1 - u).to(dtype)
    w1 = torch.from_numpy(u - u0).to(dtype)
    return torch.from_numpy(u0 % n), torch.from_numpy(u1 % n), w0, w1


def _resize_images(x, output_shape):
    """F.resize_images: align-corners bilinear, written from SURVEY Appendix B's formula (four gathers)."""
    x = _tensor(x)
    out_h, out_w = output_shape
    v0, v1, wv0, wv1 = _resize_tables(x.shape[2], out_h, x.dtype)
    u0, u1, wu0, wu1 = _resize_tables(x.shape[3], out_w, x.dtype)
    wv0, wv1 = wv0[:, None], wv1[:, None]
    y = (wv0 * wu0) * x[:, :, v0][:, :, :, u0] + (wv0 * wu1) * x[:, :, v0][:, :, :, u1] \
        + (wv1 * wu0) * x[:, :, v1][:, :, :, u0] + (wv1 * wu1) * x[:, :, v1][:, :, :, u1]
    return Variable._wrap(y)


def _softmax_cross_entropy(x, t):
    """F.softmax_cross_entropy with its defaults, SURVEY Appendix B's reading: axis 1 holds the classes,
    every other axis positions, the mean is over the positions, ignore_label = -1.
    torch.nn.functional.cross_entropy (reduction 'mean') is that operator."""
    return Variable._wrap(torch.nn.functional.cross_entropy(_tensor(x), _tensor(t).long(), ignore_index=-1))


def _maximum(x1, x2):
    # the gradient goes to x1 where x1 >= x2 and to x2 elsewhere (torch.maximum would halve it at a tie)
    a, b = _tensor(x1), _tensor(x2)
    return Variable._wrap(torch.where(a >= b, a, b))


def _where(cond, x, y):
    return Variable._wrap(torch.where(_tensor(cond).bool(), _tensor(x), _tensor(y)))


def _mean(x, axis=None):
    x = _tensor(x)
    return Variable._wrap(torch.mean(x) if axis is None else torch.mean(x, dim=axis))


def _dropout(x, ratio=.5):
    raise NotImplementedError('dropout_zero_rate > 0 is outside the fixtures (SURVEY Appendix B)')


# --------------------------------------------------------------------------- #
# training scaffolding: what updaters.py needs around update_core
# --------------------------------------------------------------------------- #
def concat_examples(batch, device=None):
    """The default converter: a list of example tuples -> a tuple of stacked ARRAYS (not Variables)."""
    out = []
    for field in zip(*batch):
        a = np.stack([np.asarray(f) for f in field])
        out.append(_tensor(a).numpy() if a.dtype.kind == 'f' else a)
    return tuple(out)


class StandardUpdater(object):
    def __init__(self, iterator, optimizer, converter=concat_examples, device=None, loss_func=None):
        self._iterators = {'main': iterator}
        self._optimizers = {'main': optimizer}
        self.converter = converter
        self.device = device
        self.loss_func = loss_func
        self.iteration = 0

    def get_optimizer(self, name):
        return self._optimizers[name]

    def get_iterator(self, name):
        return self._iterators[name]

    def update(self):
        self.update_core()
        self.iteration += 1


class ParallelUpdater(StandardUpdater):
    """Exists because updaters.py subclasses it at import time; never instantiated (out of scope)."""


class ListIterator(object):
    """``next()`` hands out the same list of example tuples every time."""

    def __init__(self, batch):
        self.batch = batch

    def next(self):
        return self.batch
    __next__ = next


class SnapshotOptimizer(object):
    """An optimizer whose update() changes nothing: it records every parameter's gradient (a copy, or None
    where the step left ``grad is None``).  Chainer's Adam is not restated here."""

    def setup(self, link):
        self.target = link
        self.grads = None
        return self

    def update(self):
        self.grads = [(n, None if p.grad is None else p.grad.copy()) for n, p in self.target.namedparams()]


class _Config(object):
    train = True


config = _Config()


@contextlib.contextmanager
def using_config(name, value):
    old = getattr(config, name)
    setattr(config, name, value)
    try:
        yield
    finally:
        setattr(config, name, old)


class _Reporter(object):
    last = None

    def report(self, values, observer=None):
        self.last = dict(values)


def _same_types(*arrays):
    return all(isinstance(a, np.ndarray) for a in arrays)


def _module(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def install():
    """Puts the stand-in into sys.modules and returns the ``chainer`` module."""
    F = torch.nn.functional
    functions = _module(
        'chainer.functions',
        relu=_unary(torch.relu), tanh=_unary(torch.tanh), sigmoid=_unary(torch.sigmoid),
        exp=_unary(torch.exp), log=_unary(torch.log),
        softplus=_unary(lambda x: -F.logsigmoid(-x)),               # log(1 + e^x), exact for every x
        log_softmax=lambda x, axis=1: Variable._wrap(torch.log_softmax(_tensor(x), dim=axis)),
        softmax=lambda x, axis=1: Variable._wrap(torch.softmax(_tensor(x), dim=axis)),
        logsumexp=lambda x, axis=None: Variable._wrap(torch.logsumexp(_tensor(x), dim=axis)),
        broadcast_to=lambda x, shape: Variable._wrap(torch.broadcast_to(_tensor(x), tuple(shape))),
        split_axis=_split_axis, concat=_concat, resize_images=_resize_images, mean=_mean,
        maximum=_maximum, where=_where, dropout=_dropout, softmax_cross_entropy=_softmax_cross_entropy)
    links = _module('chainer.links', Convolution2D=Convolution2D, DilatedConvolution2D=DilatedConvolution2D,
                    EmbedID=EmbedID)
    link = _module('chainer.link', Link=Link, Chain=Chain, ChainList=ChainList)
    variable = _module('chainer.variable', Variable=Variable, Parameter=Parameter)
    initializers = _module('chainer.initializers', _get_initializer=lambda initializer: initializer)
    function_node = _module('chainer.function_node', FunctionNode=FunctionNode)
    cuda = _module('chainer.cuda', get_array_module=lambda *a: np)
    type_check = _module('chainer.utils.type_check', expect=lambda *a: None, same_types=_same_types)
    utils = _module('chainer.utils', type_check=type_check)
    configuration = _module('chainer.configuration', config=config, using_config=using_config)
    reporter = _Reporter()
    reporter_mod = _module('chainer.reporter', report=reporter.report, state=reporter)
    training = _module('chainer.training', StandardUpdater=StandardUpdater, ParallelUpdater=ParallelUpdater)
    ch = _module('chainer', functions=functions, links=links, link=link, variable=variable,
                 initializers=initializers, function_node=function_node, cuda=cuda, utils=utils,
                 configuration=configuration, reporter=reporter_mod, training=training,
                 Variable=Variable, Parameter=Parameter, Link=Link, Chain=Chain, ChainList=ChainList,
                 FunctionNode=FunctionNode, config=config, using_config=using_config)
    if 'six' not in sys.modules:
        try:
            import six  # noqa: F401
        except ImportError:
            _module('six', iterkeys=lambda d: iter(d.keys()), itervalues=lambda d: iter(d.values()),
                    iteritems=lambda d: iter(d.items()))
    return ch
