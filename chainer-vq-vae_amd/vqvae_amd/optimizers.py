"""chainer.optimizers.Adam for this path (train.py:101-102), over flat arenas.

``setup(model)`` moves every parameter into one contiguous fp32 arena (in
namedparams order; EMA shadow copies last) and gives each trainable parameter a
slot in one contiguous gradient arena.  ``update()`` is then a single fused Adam
kernel, ``cleargrads()`` a single memset, and the data-parallel exchange a single
RCCL all-reduce of the gradient arena (updaters.py:71-77 replaced).

Lazily shaped parameters.  The reference builds ``ConditionEmbed`` with
``DilatedConvolution2D(None, ...)`` (net.py:34-43) and calls ``optimizer.setup``
before the first forward (train.py:76-102), so five conv weights do not exist at
setup time; Chainer creates them at the first call and trains them like any other
parameter.  Here ``adopt_new_params()`` -- run by the updaters between backward and
the gradient exchange, and by ``update()`` -- notices parameters created since the
last layout (core.param_epoch('init')), rebuilds the arenas with them in
namedparams order and carries over every value, gradient and Adam moment, so the
first step already updates (and all-reduces) them.

Parameters whose gradient is None at update time (the EMA copies; the last
block's ``res`` conv, modules.py:89-96) are skipped by Chainer's update rule;
here their gradient slots are zero and their Adam moments stay exactly zero, so
the update is the identity on them -- the same result.

Hooks (``add_hook`` / ``remove_hook``, Chainer's names).  A hook here is not a Python callable run
over the parameters: the gradients live in one arena, ``update()`` may be one node of a replayed
hipGraph, and nothing the host computes per step may enter it.  The three hooks below configure a
device-side pass in front of the update instead (include/vqvae_optim.h): the sum of squares of every
parameter's gradient in float64 in a fixed order, a small state block (norm, rate, scale, non-finite
flag, group norms) and an Adam kernel that reads its gradient scale and its skip decision from that
block.  An optimizer without hooks launches exactly what it launched before.
"""
import collections

import numpy as np

from . import _lib, backend, core
from .backend import DeviceArray


def plan_items(sizes, chunk=_lib.OPTIM_CHUNK):
    """The (parameter, chunk) work-item table of include/vqvae_optim.h from the parameters' sizes in layout order:
    ``items`` int32 (n_items, 2) = (start, length), ``params`` int32 (n_params, 2) = (first_item, item_count).  Parameter
    p is cut into chunks of ``chunk`` elements counted from its own offset; nothing but the sizes enters."""
    items, params, off = [], [], 0
    for size in sizes:
        size = int(size)
        if size < 0:
            raise ValueError('plan_items: negative size')
        first = len(items)
        for s in range(0, size, chunk):
            items.append((off + s, min(chunk, size - s)))
        params.append((first, len(items) - first))
        off += size
    if off > 0x7fffffff:
        raise ValueError('plan_items: %d elements do not fit the int32 table' % off)
    return (np.asarray(items, np.int32).reshape(-1, 2), np.asarray(params, np.int32).reshape(-1, 2))


class GradientClipping(object):
    """chainer.optimizer.GradientClipping(threshold) [chainer-recalled]: one L2 norm over all parameters' gradients,
    ``rate = threshold / norm``, every gradient multiplied by ``rate`` if ``rate < 1``.  NumPy multiplies a float32 array
    by the scalar in float32, so the factor applied is the float32 rounding of the float64 rate.  After ``update()`` the
    gradient arena holds the clipped gradients, as ``p.grad`` does after Chainer's hook.  A non-finite norm behaves as in
    Chainer: a NaN rate clips nothing, a zero rate makes NaNs where the gradient is infinite."""
    name = 'GradientClipping'

    def __init__(self, threshold):
        self.threshold = float(threshold)

    def key(self):
        return (self.name, float(self.threshold))


class NonFiniteGuard(object):
    """No counterpart in Chainer.  A step whose gradient norm is not finite becomes a no-op on the parameters, both Adam
    moments and the gradients; ``optimizer.skipped_steps()`` counts such steps.  ``optimizer.t`` and the device-side step
    counter of a recorded step advance all the same (the host's and the device's schedules must not diverge), so the
    step after a skipped one uses the bias correction of its own number.  Covers the optimizer update only: an
    EMA-decoder blend or an attached EMACodebook still run."""
    name = 'NonFiniteGuard'

    def key(self):
        return (self.name,)


class GradientNorms(object):
    """Reports ``grad_norm`` (all parameters, before clipping), ``grad_norm/<group>`` and, beside a GradientClipping hook,
    ``clip_rate`` through ``core.report`` as device scalars (read back when a LogReport interval closes, never per step).
    ``groups``: {name: link}; default: the direct children of ``optimizer.target`` that own trainable parameters.

    Every step reports device scalars of ITS OWN: the finalise launch writes the step's values into the next row of a
    ring of ``slots`` rows inside the state block, and the optimizer, which counts its launches, reports views of that
    row -- after an eager ``update()`` and after every replay of a recorded step (``Adam.replayed``).  A LogReport
    interval therefore averages the steps of the interval, like the losses of eager steps; it must close within
    ``slots`` steps (default 4096), after which a row is written again."""
    name = 'GradientNorms'

    def __init__(self, groups=None, slots=4096):
        self.groups = None if groups is None else collections.OrderedDict(groups)
        self.slots = int(slots)
        if self.slots < 1:
            raise ValueError('GradientNorms: slots must be at least 1')

    def key(self):
        return (self.name, self.slots,
                None if self.groups is None else tuple((n, id(l)) for n, l in self.groups.items()))

    def resolve(self, target):
        """[(name, link)]"""
        if self.groups is not None:
            return list(self.groups.items())
        return [(c.name, c) for c in target.children()]


_HOOK_TYPES = (GradientClipping, NonFiniteGuard, GradientNorms)


class Adam(object):
    _hooks = None
    _hook_dev = None
    _hook_epoch = 0
    _skipped_base = 0

    def __init__(self, alpha=0.001, beta1=0.9, beta2=0.999, eps=1e-8):
        self.alpha = alpha
        self.beta1 = beta1
        self.beta2 = beta2
        self.eps = eps
        self.t = 0
        self.target = None
        self._layout = []
        self._epoch = -1

    @property
    def lr(self):
        fix1 = 1.0 - self.beta1 ** self.t
        fix2 = 1.0 - self.beta2 ** self.t
        return self.alpha * np.sqrt(fix2) / fix1

    def setup(self, link):
        self.target = link
        self._layout = []
        self.params = self.grads = self.m = self.v = None
        self._hooks = collections.OrderedDict()
        self._prepare_hooks()                   # (a second setup: the previous target's tables and state block go)
        self._skipped_base = 0
        self._build()
        return self

    # ---- hooks -------------------------------------------------------------------------------------
    def add_hook(self, hook, name=None):
        """chainer.Optimizer.add_hook: registers ``hook`` under ``name`` (default ``hook.name``).  RuntimeError before
        ``setup``, KeyError for a name already taken.  Only this module's hook classes run on the device path."""
        if not isinstance(hook, _HOOK_TYPES):
            raise TypeError('add_hook: the update runs on the device; hooks are GradientClipping, NonFiniteGuard and '
                            'GradientNorms of vqvae_amd.optimizers, got %s' % type(hook).__name__)
        if self._hooks is None:
            raise RuntimeError('call `setup` method before `add_hook` method')
        if name is None:
            name = hook.name
        if name in self._hooks:
            raise KeyError('hook %s already exists' % name)
        for other in self._hooks.values():
            if type(other) is type(hook):
                raise ValueError('a %s hook already exists: the update has one norm pass' % type(hook).__name__)
        self._hooks[name] = hook
        self._prepare_hooks()

    def remove_hook(self, name):
        """chainer.Optimizer.remove_hook (KeyError for an unknown name)."""
        if self._hooks is None:
            raise RuntimeError('call `setup` method before `remove_hook` method')
        del self._hooks[name]
        self._prepare_hooks()

    def _hook(self, cls):
        for h in (self._hooks or {}).values():
            if isinstance(h, cls):
                return h
        return None

    def hook_groups(self):
        """[(name, [index into the trainable part of layout()])] of the GradientNorms hook ([] without one)."""
        h = self._hook(GradientNorms)
        if h is None:
            return []
        by_name = dict(self.target.namedparams())
        index = {id(by_name[n]): i for i, (n, off, size) in enumerate(self._layout) if off + size <= self.n_train}
        out = []
        for gname, link in h.resolve(self.target):
            members = sorted(index[id(p)] for p in link.params() if id(p) in index)
            if members or h.groups is not None:
                out.append((gname, members))
        return out

    def _prepare_hooks(self):
        """(Re)builds what the hooked update reads from fixed addresses: the work-item table of the current layout, the
        group table, the state block and the partials' workspace -- uploaded once, here, never from inside a recording.
        A no-op for an optimizer whose arenas are not on a device (nothing to launch on)."""
        self._hook_epoch += 1
        if self._hook_dev is not None:
            self._skipped_base += self._read_state()['skipped']
            self._hook_dev = None
        if not self._hooks or not isinstance(self.grads, DeviceArray):
            return
        if backend._state.get('arena') is not None:
            raise RuntimeError('optimizer hooks cannot be (re)configured while a step is being recorded')
        sizes = [size for _, off, size in self._layout if off + size <= self.n_train]
        items, params = plan_items(sizes)
        groups = self.hook_groups()
        goff = np.zeros(len(groups) + 1, np.int32)
        goff[1:] = np.cumsum([len(m) for _, m in groups])
        gmem = np.asarray([i for _, m in groups for i in m] + [0], np.int32)     # (never empty: a buffer needs a byte)
        lib = _lib.load()
        norms = self._hook(GradientNorms)
        slots = norms.slots if norms is not None else 1
        nbytes = lib.vqvae_optim_state_bytes(len(sizes), len(groups), slots)
        d = {'n_items': len(items), 'n_params': len(sizes), 'groups': [g for g, _ in groups], 'slots': slots,
             'launches': 0}        # launches: the host's count of finalise launches, the state block's `steps` word
        if not len(items):
            return                                    # nothing trainable: update() has nothing to do either
        d['items'] = backend.to_device(items.reshape(-1))
        d['params'] = backend.to_device(params.reshape(-1))
        d['goff'] = backend.to_device(goff)
        d['gmem'] = backend.to_device(gmem)
        d['state'] = backend.zeros(((nbytes + 7) // 8,), np.float64)
        d['ws'] = backend.empty((len(items),), np.float64)
        st = d['state']
        f32 = lambda byte: DeviceArray((), np.float32, _block=st._block, _ptr=st.ptr + byte)
        d['f32'] = f32
        d['ring'] = _lib.OPTIM_STATE_HEADER + 8 * len(sizes) + 4 * len(groups)      # byte offset of the report ring
        self._hook_dev = d

    def _read_state(self):
        """Host copy of the state block (synchronises): the fields of include/vqvae_optim.h by name."""
        d = self._hook_dev
        raw = d['state'].get().view(np.uint8)
        n_p, n_g = d['n_params'], len(d['groups'])
        h = _lib.OPTIM_STATE_HEADER
        return {'S': float(raw[0:8].view(np.float64)[0]), 'norm': float(raw[8:16].view(np.float64)[0]),
                'rate': float(raw[16:24].view(np.float64)[0]), 'scale': raw[24:28].view(np.float32)[0],
                'nonfinite': int(raw[28:32].view(np.int32)[0]), 'skipped': int(raw[32:36].view(np.int32)[0]),
                'steps': int(raw[36:40].view(np.int32)[0]),
                'norm_f32': raw[40:44].view(np.float32)[0], 'rate_f32': raw[44:48].view(np.float32)[0],
                'param_sumsq': raw[h:h + 8 * n_p].view(np.float64).copy(),
                'group_norms': raw[h + 8 * n_p:h + 8 * n_p + 4 * n_g].view(np.float32).copy()}

    def hook_state(self):
        """The device state block of the last hooked ``update()`` as a dict (a host read on demand)."""
        if self._hook_dev is None:
            raise RuntimeError('no hook is attached (or nothing is trainable): there is no norm pass to read')
        return self._read_state()

    def grad_norms(self):
        """{'grad_norm', 'grad_norm/<group>'..., 'clip_rate' with a clipping hook} of the last ``update()``, as floats (a
        host read on demand; the GradientNorms hook reports the same values as device scalars)."""
        st = self.hook_state()
        out = {'grad_norm': st['norm']}
        for g, v in zip(self._hook_dev['groups'], st['group_norms']):
            out['grad_norm/' + g] = float(v)
        if self._hook(GradientClipping) is not None:
            out['clip_rate'] = st['rate']
        return out

    def skipped_steps(self):
        """How many updates the NonFiniteGuard has turned into a no-op since ``setup`` (a host read on demand)."""
        return self._skipped_base + (self._read_state()['skipped'] if self._hook_dev is not None else 0)

    def _update_hooked(self, lr, lr_table, step):
        d = self._hook_dev
        if d is None:
            self._prepare_hooks()
            d = self._hook_dev
            if d is None:
                return
        clip = self._hook(GradientClipping)
        flags = _lib.OPTIM_GUARD if self._hook(NonFiniteGuard) is not None else 0
        st = backend.stream()
        _lib.call('vqvae_optim_sumsq', self.grads.ptr, self.n_train, d['items'].ptr, d['n_items'], d['params'].ptr,
                  d['n_params'], d['goff'].ptr, d['gmem'].ptr, len(d['groups']), d['slots'],
                  float('inf') if clip is None else float(clip.threshold), flags, d['state'].ptr, d['ws'].ptr,
                  d['ws'].nbytes, st)
        _lib.call('vqvae_optim_adam_step_hooked', self.params.ptr, self.grads.ptr, self.m.ptr, self.v.ptr, self.n_train,
                  lr, lr_table, step, float(self.beta1), float(self.beta2), float(self.eps), d['state'].ptr, flags, st)
        if not self._recording:         # (a recorded launch has not run yet: Adam.replayed publishes it when it has)
            self._publish()

    def _publish(self):
        """Host-side bookkeeping of one executed norm pass: counts it (the row of the report ring it wrote follows from
        the count alone) and, with a GradientNorms hook, reports that row's device scalars -- this step's own."""
        d = self._hook_dev
        if d is None:
            return
        row = d['ring'] + 4 * (2 + len(d['groups'])) * (d['launches'] % d['slots'])
        d['launches'] += 1
        if self._hook(GradientNorms) is None:
            return
        values = {'grad_norm': d['f32'](row)}
        for j, g in enumerate(d['groups']):
            values['grad_norm/' + g] = d['f32'](row + 8 + 4 * j)
        if self._hook(GradientClipping) is not None:
            values['clip_rate'] = d['f32'](row + 4)
        core.report(values, self.target)

    # ------------------------------------------------------------------ #
    def _build(self):
        """(Re)builds the flat arenas over every parameter that has storage now."""
        self._epoch = core.param_epoch('init')
        named = [(n, p) for n, p in self.target.namedparams() if p.data is not None]
        for n, p in named:
            if not isinstance(p.data, DeviceArray):
                raise ValueError('optimizer.setup: parameter %s is on the host; call '
                                 'model.to_gpu() first (there is no CPU update path)' % n)
            # (checked BEFORE any p.data is re-pointed at an arena view: backend.copy_many refuses other dtypes, and a refusal
            #  half-way through the adoption would leave parameters pointing at views nothing was copied into)
            g = p.grad.data if isinstance(p.grad, core.Variable) else p.grad
            if p.data.dtype != np.float32 or (isinstance(g, DeviceArray) and g.dtype != np.float32):
                raise ValueError('optimizer.setup: parameter %s is %s; the arenas are float32' % (n, p.data.dtype))
        train = [(n, p) for n, p in named if not p._shadow]
        shadow = [(n, p) for n, p in named if p._shadow]
        old = {n: (off, size) for n, off, size in self._layout}
        old_m, old_v, old_n_train = self.m, self.v, getattr(self, 'n_train', 0)
        n_train = sum(p.size for _, p in train)
        n_all = n_train + sum(p.size for _, p in shadow)
        params = backend.empty((n_all,), np.float32)
        grads = backend.zeros((n_train,), np.float32)
        m = backend.zeros((n_train,), np.float32)
        v = backend.zeros((n_train,), np.float32)
        layout = []
        off = 0
        copies = []                           # (dst, src): issued together below (backend.copy_many)
        for n, p in train + shadow:
            view = params.flat_view(off, p.size, p.data.shape)
            copies.append((view, p.data))     # from the old arena or from the parameter's own buffer
            p.data = view
            if not p._shadow:
                slot = grads.flat_view(off, p.size, view.shape)
                if p.grad is not None:        # gradient accumulated before adoption / re-layout
                    copies.append((slot, p.grad.reshape(view.shape) if isinstance(p.grad, DeviceArray)
                                   else p.grad.data.reshape(view.shape)))
                    p.grad = slot
                p._grad_slot = slot
                if n in old and old[n][0] + old[n][1] <= old_n_train:
                    o, sz = old[n]
                    copies.append((m.flat_view(off, sz), old_m.flat_view(o, sz)))
                    copies.append((v.flat_view(off, sz), old_v.flat_view(o, sz)))
            p._owner_step = self._step_count        # lets caches notice parameter updates
            layout.append((n, off, p.size))
            off += p.size
        backend.copy_many(copies)
        self.params, self.grads, self.m, self.v = params, grads, m, v
        self._layout = layout
        self.n_train = n_train
        core.bump_param_epoch('layout')
        if self._hooks:
            self._prepare_hooks()               # the work-item table follows the layout

    def adopt_new_params(self):
        """Re-lays the arenas when parameters were created since the last layout (lazily
        shaped links at their first forward).  Cheap when nothing changed: one integer compare."""
        if self._epoch == core.param_epoch('init'):
            return False
        known = {n for n, _, _ in self._layout}
        fresh = [n for n, p in self.target.namedparams() if p.data is not None and n not in known]
        if not fresh:
            self._epoch = core.param_epoch('init')
            return False
        for n, p in self.target.namedparams():
            if n in fresh:
                p.to_gpu()
        self._build()
        return True

    def uninitialized_params(self):
        return [n for n, p in self.target.namedparams() if p.data is None]

    def _step_count(self):
        return self.t

    def update(self):
        """One Adam step on every trainable parameter (chainer Adam update rule)."""
        if self._recording:
            # inside a hipGraph capture (updaters.GraphedStep): the step size comes from the device-side schedule,
            # nothing host-dependent goes into the recorded launch
            if self._hooks:
                return self._update_hooked(0.0, self._lr_table.ptr, self._step_dev.ptr)
            _lib.call('vqvae_adam_step_dev', self.params.ptr, self.grads.ptr, self.m.ptr, self.v.ptr, self.n_train,
                      self._lr_table.ptr, self._step_dev.ptr, float(self.beta1), float(self.beta2), float(self.eps),
                      backend.stream())
            return
        self.adopt_new_params()
        self.t += 1
        if self._hooks:
            return self._update_hooked(float(self.lr), None, None)
        _lib.call('vqvae_adam_step', self.params.ptr, self.grads.ptr, self.m.ptr, self.v.ptr,
                  self.n_train, float(self.lr), float(self.beta1), float(self.beta2),
                  float(self.eps), backend.stream())

    # ---- device-side schedule for a captured step ------------------------------------------------
    _recording = False
    _lr_table = None
    SCHEDULE_HORIZON = 4096

    def sync_schedule(self):
        """Makes lr_table[*step] the step size of update number ``self.t + 1`` (what the next replayed step must
        use): a no-op while the device counter is where the host's ``t`` says; otherwise -- first use, the horizon
        reached, eager steps in between -- the table is refilled from ``t`` (one small synchronous upload)."""
        hyper = (float(self.alpha), float(self.beta1), float(self.beta2))
        if (self._lr_table is not None and self._sched_next == self.t + 1
                and self.t + 1 - self._sched_base <= self.SCHEDULE_HORIZON
                and self._sched_hyper == hyper):        # (a changed alpha / beta -- a decay extension, a manual edit -- refills the table: ADVICE r4)
            return
        base, t_save = self.t, self.t
        tbl = np.empty(self.SCHEDULE_HORIZON, np.float32)
        for i in range(self.SCHEDULE_HORIZON):
            self.t = base + 1 + i
            tbl[i] = np.float32(self.lr)             # the same double -> float32 rounding as vqvae_adam_step's cast
        self.t = t_save
        if self._lr_table is None:
            self._lr_table = backend.empty((self.SCHEDULE_HORIZON,), np.float32)
            self._step_dev = backend.empty((1,), np.int32)
        self._lr_table.set(tbl)
        self._step_dev.set(np.zeros(1, np.int32))
        self._sched_base, self._sched_next = base, base + 1
        self._sched_hyper = hyper

    def capture_key(self):
        """What a recorded step bakes into its Adam launch as kernel arguments: a change re-records (updaters._step_key)."""
        key = (float(self.beta1), float(self.beta2), float(self.eps))
        if self._hooks:     # which hooks, the threshold and the tables' identity are baked in too
            key += (tuple((n, h.key()) for n, h in self._hooks.items()), self._hook_epoch)
        return key

    def replayed(self):
        """Host-side bookkeeping of one replayed (or just captured and launched) step."""
        self.t += 1
        self._sched_next = self.t + 1
        if self._hooks:
            self._publish()

    def layout(self):
        """[(name, offset, size)] of the flat arena (trainable first)."""
        return list(self._layout)
