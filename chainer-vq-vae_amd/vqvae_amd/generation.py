"""Incremental WaveNet generation -- the queue machinery of WaveNet/modules.py:58-74, 98-110,
232-255 and the sampling loop of generate.py:101-145, on the device.

``WaveNet.initialize(n)`` / ``WaveNet.generate(x, condition)`` keep the reference's step-by-step
call surface (the host supplies the input vector and the condition column, gets the logits).
``WaveNet.generate_sequence`` is the MI355X-native form of generate.py's ``for i in range(...)``:
the whole loop -- network step, sampler, feedback of the sample, step counter -- lives in device
memory, one step's ~45 kernel launches are captured once into a hipGraph and the graph is
replayed, so the host does nothing per sample.
"""
import ctypes as C

import numpy as np

from . import _lib, backend, core
from .backend import DeviceArray

_S = backend.stream
_INT_MAX = 2 ** 31 - 1


def sampling_controls(n, temperature=None, top_k=None, top_p=None, use_logistic=False, who='generate_sequence'):
    """The sampling controls of include/vqvae_sampling.h as host arrays, validated: each of ``temperature`` (>= 0 and
    finite; 0 = greedy), ``top_k`` (integers >= 0; 0 or >= out_dim = off) and ``top_p`` (in (0, 1]; 1 = off) is None, a
    scalar or a sequence of ``n`` values, one per sequence.  Returns None when all three are None (the caller then takes
    the path it took before the controls existed), else the tuple (float32 (n,), int32 (n,), float32 (n,)) with None in
    the place of a control that was not given.  The mixture-of-logistics output takes a temperature > 0 only.
    Everything else is a ValueError: the device cannot refuse a value, it reads a bad one as neutral."""
    if temperature is None and top_k is None and top_p is None:
        return None

    def per_sequence(v, name, dtype):
        if v is None:
            return None
        a = np.asarray(v)
        if a.dtype.kind not in 'iuf' or (dtype == np.int32 and a.dtype.kind == 'f' and not (a == np.floor(a)).all()):
            raise ValueError('%s: %s must be %s, got %r' % (who, name, 'integers' if dtype == np.int32 else 'numbers', v))
        if a.ndim == 0:
            a = np.full((n,), a)
        if a.shape != (n,):
            raise ValueError('%s: %s must be a scalar or one value per sequence (%d), got shape %s' % (who, name, n, a.shape))
        return a

    t = per_sequence(temperature, 'temperature', np.float32)
    k = per_sequence(top_k, 'top_k', np.int32)
    p = per_sequence(top_p, 'top_p', np.float32)
    if t is not None and not (np.isfinite(t).all() and (t >= 0).all()):
        raise ValueError('%s: temperature must be finite and >= 0, got %r' % (who, temperature))
    if k is not None and not ((k >= 0).all() and (k <= _INT_MAX).all()):
        raise ValueError('%s: top_k must be >= 0 (0 = off), got %r' % (who, top_k))
    if p is not None and not ((p > 0).all() and (p <= 1).all()):          # a NaN fails both comparisons
        raise ValueError('%s: top_p must be in (0, 1] (1 = off), got %r' % (who, top_p))
    if use_logistic:
        if k is not None or p is not None:
            raise ValueError('%s: top_k and top_p truncate a categorical output; the mixture of logistics '
                             '(use_logistic) takes a temperature only' % who)
        if (t == 0).any():
            raise ValueError('%s: temperature 0 (greedy) needs the softmax output; the mixture of logistics '
                             '(use_logistic) takes a temperature > 0' % who)
    return (None if t is None else t.astype(np.float32), None if k is None else k.astype(np.int32),
            None if p is None else p.astype(np.float32))


def _upload_controls(sampling):
    """(GenSampling, the device arrays it points to) for the tuple sampling_controls returns."""
    arrays = [None if a is None else backend.to_device(np.ascontiguousarray(a)) for a in sampling]
    s = _lib.GenSampling()
    s.temperature, s.top_k, s.top_p = [None if a is None else a.ptr for a in arrays]
    return s, arrays


def sample_logits(logits, uniforms, mode=_lib.GEN_SOFTMAX, temperature=None, top_k=None, top_p=None, log_scale_min=-40.0,
                  return_probs=False):
    """The sampler of a generation step on logits of the caller's own (vqvae_sample_logits): device float32 (n, out_dim),
    host doubles ``uniforms`` (n,) for the softmax output or (n, nr_mix) for the mixture of logistics, the controls as in
    sampling_controls.  Returns the device array (n,) of int32 classes or float32 values (and, with ``return_probs``, the
    filtered probabilities (n, out_dim) the draw used; softmax output only)."""
    backend.require_device(logits)
    n, out_dim = logits.shape
    softmax = mode == _lib.GEN_SOFTMAX
    sampling = sampling_controls(n, temperature, top_k, top_p, not softmax, 'sample_logits')
    u = np.ascontiguousarray(uniforms, dtype=np.float64).reshape(n, -1)
    u_dev = backend.to_device(u.reshape(-1))
    out = backend.zeros((n,), np.int32 if softmax else np.float32)
    probs = DeviceArray((n, out_dim), np.float32) if return_probs else None
    s, keep = (None, None) if sampling is None else _upload_controls(sampling)
    _lib.call('vqvae_sample_logits', logits.ptr, n, out_dim, mode, float(log_scale_min), u_dev.ptr, u.shape[1],
              None if s is None else C.byref(s), out.ptr, None if probs is None else probs.ptr, _S())
    backend.synchronize()                                   # u_dev and the control arrays go out of scope here
    return (out, probs) if return_probs else out


class GenerationState(object):
    """Device state behind WaveNet.initialize(n): zero queues (modules.py:58-67, 232-244) as
    per-block rings of ``dilation`` slots, the 2-sample embed queue, the step counter."""
    max_n = _lib.GEN_MAX_N

    def __init__(self, wavenet, n):
        if not 1 <= n <= self.max_n:
            raise ValueError('generation runs 1..%d sequences in lockstep (generate.py:42 runs 1), got %d'
                             % (self.max_n, n))
        blocks = list(wavenet.resnet.children())
        for p in wavenet.params():
            if p.data is None:
                raise RuntimeError('WaveNet.initialize: parameters are not initialised')
            backend.require_device(p.data)
        b0 = blocks[0]
        if b0.filter_size != 2:
            raise NotImplementedError('incremental generation supports filter_size == 2 (params.py:31)')
        self.n = n
        # the state holds raw device pointers of the weights: keep their buffers alive and
        # remember which parameter layout / contents they belong to
        self._weights = [p.data for p in wavenet.params()]
        self._epochs = (core.param_epoch('layout'), core.param_epoch('load'))
        self.input_dim = wavenet.embed.W.shape[1]
        self.residual = wavenet.embed.W.shape[0]
        self.dilated = b0.conv.W.shape[0]
        self.skip = b0.skip.W.shape[0]
        self.cond_dim = b0.condition_proj.W.shape[1]
        self.out_dim = wavenet.proj2.W.shape[0]
        f32 = np.float32
        self.step = backend.zeros((1,), np.int32)
        self.x_cur = backend.zeros((n, self.input_dim), f32)
        self.x_prev = backend.zeros((n, self.input_dim), f32)
        self.h0 = backend.zeros((n, self.residual), f32)
        self.h1 = backend.zeros((n, self.residual), f32)
        self.z = backend.zeros((n, self.dilated // 2), f32)
        self.skip_acc = backend.zeros((n, self.skip), f32)
        self.s1 = backend.zeros((n, self.skip), f32)
        self.logits = backend.zeros((n, self.out_dim), f32)
        self.rings = [backend.zeros((b.dilation, n, self.residual), f32) for b in blocks]
        self._blocks = (_lib.GenBlock * len(blocks))()
        for gb, b, ring in zip(self._blocks, blocks, self.rings):
            gb.conv_W, gb.conv_b = b.conv.W.data.ptr, b.conv.b.data.ptr
            gb.cond_W, gb.cond_b = b.condition_proj.W.data.ptr, b.condition_proj.b.data.ptr
            gb.res_W, gb.res_b = b.res.W.data.ptr, b.res.b.data.ptr
            gb.skip_W, gb.skip_b = b.skip.W.data.ptr, b.skip.b.data.ptr
            gb.ring, gb.dilation = ring.ptr, b.dilation
        d = _lib.GenDesc()
        d.n, d.n_blocks = n, len(blocks)
        d.input_dim, d.residual, d.dilated, d.skip = self.input_dim, self.residual, self.dilated, self.skip
        d.cond_dim, d.out_dim = self.cond_dim, self.out_dim
        d.log_scale_min = float(wavenet.log_scale_min)
        d.embed_W, d.embed_b = wavenet.embed.W.data.ptr, wavenet.embed.b.data.ptr
        d.proj1_W, d.proj1_b = wavenet.proj1.W.data.ptr, wavenet.proj1.b.data.ptr
        d.proj2_W, d.proj2_b = wavenet.proj2.W.data.ptr, wavenet.proj2.b.data.ptr
        d.blocks = self._blocks
        for name in ('step', 'x_cur', 'x_prev', 'h0', 'h1', 'z', 'skip_acc', 's1', 'logits'):
            setattr(d, name, getattr(self, name).ptr)
        d.sample_mode = _lib.GEN_NONE
        d.max_steps = _INT_MAX
        self.desc = d

    # ---- reference-shaped single step: WaveNet.generate(x, condition) (modules.py:246-255) ----
    def step_logits(self, x, condition):
        n = self.n
        if x.size != n * self.input_dim:
            raise ValueError('generate: x must hold (n, input_dim, 1, 1) = (%d, %d, 1, 1) values, got %s'
                             % (n, self.input_dim, x.shape))
        if condition.size != n * self.cond_dim:
            raise ValueError('generate: condition must hold (n, condition_dim, 1, 1) = (%d, %d, 1, 1) '
                             'values, got %s' % (n, self.cond_dim, condition.shape))
        self.x_cur.copy_from(x)
        d = self.desc
        d.sample_mode = _lib.GEN_NONE
        d.cond, d.cond_bstride, d.cond_cstride, d.cond_follows_step = condition.ptr, self.cond_dim, 1, 0
        d.uniforms = d.forced_next = d.out = d.logits_out = None
        d.max_steps = _INT_MAX
        _lib.call('vqvae_wavenet_gen_step', C.byref(d), _S())
        self._keep = (x, condition)
        return self.logits.copy().reshape(n, self.out_dim, 1, 1)

    # ---- the whole loop of generate.py:105-145 on the device ----------------------------------
    def run(self, condition, uniforms, mode, n_steps=None, forced=None, return_logits=False,
            graph_steps=8, persistent=False, chunk=4096, sampling=None):
        """``sampling``: None or the tuple of sampling_controls(n, ...).  With controls every step ends in the filtered
        sampler of csrc/sampling.hip (vqvae_wavenet_gen_step_sampled) and ``persistent`` is not honoured: the persistent
        kernel has no filtered form, the run is a replayed hipGraph of per-step launches."""
        n = self.n
        if condition.ndim == 4:
            condition = condition.reshape(condition.shape[:3])
        if condition.shape[:2] != (n, self.cond_dim):
            raise ValueError('generate_sequence: condition must be (n, condition_dim, T[, 1]) = (%d, %d, T), got %s'
                             % (n, self.cond_dim, condition.shape))
        T = condition.shape[2]
        steps = T - 1 if n_steps is None else int(n_steps)          # generate.py:105
        if not 0 <= steps <= T:
            raise ValueError('generate_sequence: n_steps must be in [0, %d]' % T)
        softmax = mode == _lib.GEN_SOFTMAX
        n_uniform = 1 if softmax else self.out_dim // 3
        u = np.ascontiguousarray(uniforms, dtype=np.float64).reshape(-1)
        if u.size < steps * n * n_uniform:
            raise ValueError('generate_sequence: need %d uniform doubles (steps, n, %d), got %d'
                             % (steps * n * n_uniform, n_uniform, u.size))
        u_dev = backend.to_device(u[:max(1, steps * n * n_uniform)])
        out = backend.zeros((n, T), np.int32 if softmax else np.float32)     # generate.py:103
        forced_dev = None
        if forced is not None:
            forced_dev = backend.to_device(np.ascontiguousarray(
                forced, dtype=np.int32 if softmax else np.float32).reshape(-1)[:steps * n])
        logits_out = DeviceArray((max(steps, 1), n, self.out_dim), np.float32) if return_logits else None
        d = self.desc
        d.sample_mode = mode
        d.cond, d.cond_bstride, d.cond_cstride, d.cond_follows_step = condition.ptr, self.cond_dim * T, T, 1
        d.uniforms, d.n_uniform = u_dev.ptr, n_uniform
        d.forced_next = None if forced_dev is None else forced_dev.ptr
        d.out, d.out_bstride = out.ptr, T
        d.logits_out = None if logits_out is None else logits_out.ptr
        if int(self.step.get()[0]) != 0:
            raise RuntimeError('generate_sequence starts from fresh queues: call initialize(n) first')
        d.max_steps = steps
        if sampling is None:
            def step():
                _lib.call('vqvae_wavenet_gen_step', C.byref(d), _S())
        else:
            smp, self._controls = _upload_controls(sampling)
            persistent = False

            def step():
                _lib.call('vqvae_wavenet_gen_step_sampled', C.byref(d), C.byref(smp), _S())
        nbytes = 0
        if steps and persistent:
            # the library picks the width class (<= 256 or <= 512 channels per vector); shapes outside
            # both (or a device too small to hold a launch) get 0 bytes and run on the per-step
            # kernels below -- same results, more launches
            nbytes = _lib.load().vqvae_wavenet_gen_run_workspace_bytes(C.byref(d))
        if steps and persistent and nbytes:
            # one persistent launch per `chunk` steps; queues + mailboxes live in its workspace
            ws = DeviceArray((nbytes // 4 + 1,), np.int32)
            for t0 in range(0, steps, chunk):
                _lib.call('vqvae_wavenet_gen_run', C.byref(d), t0, min(chunk, steps - t0), ws.ptr,
                          ws.nbytes, _S())
            backend.synchronize()
            status = int(ws.flat_view(0, 1).get()[0])
            self._last_ws = ws
            if status:
                raise RuntimeError('persistent generation kernel gave up waiting (status %d): are all '
                                   'its workgroups resident?' % status)
            self.step.set(np.array([steps], np.int32))
        elif steps and not graph_steps:                # eager launches (profilers, debugging)
            for _ in range(steps):
                step()
            backend.synchronize()
        elif steps:
            per = max(1, min(int(graph_steps), steps))
            graph = C.c_void_p()
            _lib.call('vqvae_graph_capture_begin', _S())
            try:
                for _ in range(per):
                    step()
            finally:
                _lib.call('vqvae_graph_capture_end', _S(), C.byref(graph))
            try:
                for _ in range((steps + per - 1) // per):        # surplus steps are device no-ops
                    _lib.call('vqvae_graph_launch', graph, _S())
                backend.synchronize()
            finally:
                _lib.call('vqvae_graph_destroy', graph)
        d.max_steps = _INT_MAX
        return (out, logits_out) if return_logits else out


def run_many(wavenet, condition, uniforms, mode, n_steps=None, group=_lib.GEN_MAX_N, max_streams=8,
             chunk=4096):
    """Batched serving form of the loop: N sequences = ceil(N / group) independent persistent
    launches of <= ``group`` lockstep sequences each, spread over ``max_streams`` HIP streams so
    they run concurrently (a launch occupies 128 or 256 two-wave workgroups: a fraction of the GPU).
    condition (N, condition_dim, T) on the device, uniforms (T, N[, nr_mix]) on the host.
    Returns the host array (N, T) of sampled bins / values."""
    if condition.ndim == 4:
        condition = condition.reshape(condition.shape[:3])
    N, Cc, T = condition.shape
    steps = T - 1 if n_steps is None else int(n_steps)
    softmax = mode == _lib.GEN_SOFTMAX
    u = np.asarray(uniforms, np.float64)
    u = u.reshape(u.shape[0], N, -1)
    lib = _lib.load()
    jobs = []
    for g0 in range(0, N, group):
        n = min(group, N - g0)
        st = GenerationState(wavenet, n)
        d = st.desc
        n_uniform = 1 if softmax else st.out_dim // 3
        if u.shape[0] < steps or u.shape[2] < n_uniform:
            raise ValueError('generate_batch: need (steps, N, %d) uniform doubles, got %s' % (n_uniform, u.shape))
        u_dev = backend.to_device(np.ascontiguousarray(u[:max(steps, 1), g0:g0 + n, :n_uniform]).reshape(-1))
        out = backend.zeros((n, T), np.int32 if softmax else np.float32)
        cview = condition.flat_view(g0 * Cc * T, n * Cc * T, (n, Cc, T))
        d.sample_mode = mode
        d.cond, d.cond_bstride, d.cond_cstride, d.cond_follows_step = cview.ptr, Cc * T, T, 1
        d.uniforms, d.n_uniform = u_dev.ptr, n_uniform
        d.forced_next = d.logits_out = None
        d.out, d.out_bstride = out.ptr, T
        d.max_steps = steps
        nbytes = lib.vqvae_wavenet_gen_run_workspace_bytes(C.byref(d))
        if not nbytes:
            raise ValueError('persistent generation: ' + lib.vqvae_last_error_string().decode())
        ws = DeviceArray((nbytes // 4 + 1,), np.int32)
        jobs.append((st, d, out, ws, u_dev, cview))
    backend.synchronize()                  # buffers above were prepared on the main stream
    # every workgroup of a launch must be resident at once (its waves wait for each other): the
    # library knows the width class's workgroup count and the kernel's occupancy on this device
    resident = min(lib.vqvae_wavenet_gen_run_concurrency(C.byref(j[1])) for j in jobs)
    max_streams = max(1, min(max_streams, resident))
    for t0 in range(0, steps, chunk):
        for i, (st, d, out, ws, _, _) in enumerate(jobs):
            _lib.call('vqvae_wavenet_gen_run', C.byref(d), t0, min(chunk, steps - t0), ws.ptr, ws.nbytes,
                      backend.pool_stream(i % max_streams))
    backend.synchronize()
    res = []
    for st, d, out, ws, _, _ in jobs:
        status = int(ws.flat_view(0, 1).get()[0])
        if status:
            raise RuntimeError('persistent generation kernel gave up waiting (status %d)' % status)
        res.append(out.get())
    return np.concatenate(res, axis=0)


class LockstepState(GenerationState):
    """The same descriptor and buffers for 1..128 sequences: vqvae_wavenet_gen_step runs n > 4 on the lockstep
    kernels (csrc/generate_lockstep.hip, the batch in MFMA columns).  The persistent kernel stays at n <= 4, so
    ``run`` is used with ``persistent=False``."""
    max_n = _lib.GEN_MAX_LOCKSTEP


def plan_lockstep(N, T, lengths=None, n_steps=None, group=_lib.GEN_MAX_LOCKSTEP):
    """Who runs with whom, and for how long.  Returns (steps, groups): steps[i] = steps sequence i runs
    (lengths[i] - 1 as generate.py:105 would for a condition of that length, capped by ``n_steps``), groups = list of
    (indices, group_steps) in running order.  With ``lengths`` the sequences are sorted by length (longest first,
    ties in the caller's order) before they are cut into groups of <= ``group``, so that a group stops at its
    longest member; without, groups are consecutive slices.  A group of fewer than 5 is filled up to 5 with
    repeats of its last member."""
    if not _lib.GEN_MAX_N < group <= _lib.GEN_MAX_LOCKSTEP:
        raise ValueError('generate_lockstep: group must be %d..%d, got %d' % (_lib.GEN_MAX_N + 1, _lib.GEN_MAX_LOCKSTEP, group))
    if lengths is None:
        full = T - 1 if n_steps is None else int(n_steps)
        if not 0 <= full <= T:
            raise ValueError('generate_lockstep: n_steps must be in [0, %d]' % T)
        steps = np.full((N,), full, np.int64)
        order = np.arange(N)
    else:
        lengths = np.asarray(lengths).astype(np.int64).reshape(-1)
        if lengths.shape != (N,) or (lengths < 1).any() or (lengths > T).any():
            raise ValueError('generate_lockstep: lengths must be (N,) = (%d,) integers in [1, %d]' % (N, T))
        steps = lengths - 1
        if n_steps is not None:
            if int(n_steps) < 0:
                raise ValueError('generate_lockstep: n_steps must not be negative')
            steps = np.minimum(steps, int(n_steps))
        order = np.argsort(-steps, kind='stable')
    groups = []
    for g0 in range(0, N, group):
        idx = order[g0:g0 + group]
        if len(idx) <= _lib.GEN_MAX_N:
            # n <= 4 would run the matrix-vector kernels, which sum in another order: repeat the last member so
            # that every sequence of every call goes through the same arithmetic
            idx = np.concatenate([idx, np.repeat(idx[-1:], _lib.GEN_MAX_N + 1 - len(idx))])
        groups.append((idx, int(steps[idx].max())))
    return steps, groups


def _device_group_runner(wavenet, condition, mode, graph_steps, return_logits):
    """One group of run_lockstep on the device: fresh LockstepState, the group's condition rows gathered into one
    array, a replayed hipGraph of per-step launches on the main stream."""
    N, Cc, T = condition.shape

    def run_group(idx, u, forced, steps, sampling=None):
        n = len(idx)
        if (np.diff(idx) == 1).all():
            cview = condition.flat_view(int(idx[0]) * Cc * T, n * Cc * T, (n, Cc, T))
        else:
            cview = DeviceArray((n, Cc, T), np.float32)
            backend.copy_many([(cview.flat_view(j * Cc * T, Cc * T), condition.flat_view(int(i) * Cc * T, Cc * T))
                               for j, i in enumerate(idx)])
        st = LockstepState(wavenet, n)
        res = st.run(cview, u, mode, steps, forced, return_logits, graph_steps, persistent=False, sampling=sampling)
        if return_logits:
            return res[0].get(), res[1].get()[:steps]
        return res.get(), None
    return run_group


def run_lockstep(wavenet, condition, uniforms, mode, n_steps=None, lengths=None, forced=None, return_logits=False,
                 graph_steps=8, group=_lib.GEN_MAX_LOCKSTEP, _run_group=None, sampling=None):
    """Many sequences at once (converting a validation set or a corpus): N sequences of any count as groups of
    <= ``group`` (<= 128) lockstep sequences, each group a replayed hipGraph of ``graph_steps`` per-step launches
    (0 = eager launches), the groups one after another on the main stream.  The weights are streamed once per
    step for the whole group.

    condition (N, condition_dim, T) on the device, uniforms (T, N[, nr_mix]) host doubles, forced (T, N) or None.
    ``lengths`` (N,) integers: sequence i runs lengths[i] - 1 steps, as generate.py:105 would for a condition of
    that length, and its output columns from lengths[i] - 1 on are 0.
    Returns the host array (N, T) in the caller's order (and, with ``return_logits``, the host array
    (max steps, N, out_dim), rows past a sequence's own steps 0).  Every sequence gets the values it gets in any
    other batch of 5..128 and in any other position of it, bit for bit.
    ``sampling``: None or the tuple of sampling_controls(N, ...); every group gets its members' values, gathered with the
    group's indices like the uniforms (repeats of the last member included), and the promise above holds with them."""
    if condition.ndim == 4:
        condition = condition.reshape(condition.shape[:3])
    N, Cc, T = condition.shape
    steps, groups = plan_lockstep(N, T, lengths, n_steps, group)
    softmax = mode == _lib.GEN_SOFTMAX
    out_dim = wavenet.proj2.W.shape[0]
    n_uniform = 1 if softmax else out_dim // 3
    u = np.asarray(uniforms, np.float64)
    max_steps = int(steps.max()) if N else 0
    if u.ndim < 2 or u.shape[1] != N:
        raise ValueError('generate_lockstep: uniforms must be (T, N[, %d]) = (%d, %d, ...), got %s'
                         % (n_uniform, T, N, u.shape))
    u = u.reshape(u.shape[0], N, -1)
    if u.shape[0] < max_steps or u.shape[2] < n_uniform:
        raise ValueError('generate_lockstep: need (%d, %d, %d) uniform doubles, got %s' % (max_steps, N, n_uniform, u.shape))
    if forced is not None:
        forced = np.asarray(forced).reshape(-1, N)
        if forced.shape[0] < max_steps:
            raise ValueError('generate_lockstep: forced must be (steps, N) = (%d, %d), got %s' % (max_steps, N, forced.shape))
    run_group = _run_group or _device_group_runner(wavenet, condition, mode, graph_steps, return_logits)
    out = np.zeros((N, T), np.int32 if softmax else np.float32)                  # generate.py:103
    logits = np.zeros((max_steps, N, out_dim), np.float32) if return_logits else None
    for idx, gsteps in groups:
        ug = np.ascontiguousarray(u[:max(gsteps, 1), idx, :n_uniform])
        fg = None if forced is None else np.ascontiguousarray(forced[:gsteps, idx])
        if sampling is None:
            o, lg = run_group(idx, ug, fg, gsteps)
        else:
            o, lg = run_group(idx, ug, fg, gsteps, tuple(None if a is None else a[idx] for a in sampling))
        for j, i in enumerate(idx):
            out[i, :steps[i]] = o[j, :steps[i]]           # a shorter sequence kept running: its tail is discarded
            if return_logits:
                logits[:steps[i], i] = lg[:steps[i], j]
    return (out, logits) if return_logits else out


# ---- lockstep generation with refill (include/vqvae_gen_slots.h, csrc/generate_slots.hip) -----------------------------
def refill_queue(steps):
    """The serving order of run_lockstep_refill: longest first, ties in the caller's order, sequences with 0 steps left
    out (their output rows stay 0)."""
    steps = np.asarray(steps, np.int64).reshape(-1)
    order = np.argsort(-steps, kind='stable')
    return order[steps[order] > 0].astype(np.int32)


def refill_slots(n_queue, group=_lib.GEN_MAX_LOCKSTEP):
    """S = clamp(min(sequences to run, group), 5, 128): the slot count of a refilled run."""
    if not _lib.GEN_MAX_N < group <= _lib.GEN_MAX_LOCKSTEP:
        raise ValueError('generate_lockstep: group must be %d..%d, got %d' % (_lib.GEN_MAX_N + 1, _lib.GEN_MAX_LOCKSTEP, group))
    return max(_lib.GEN_MAX_N + 1, min(int(n_queue), int(group)))


def plan_refill(steps, slots):
    """The device scheduler's rule (csrc/generate_slots.hip) replayed on the host.  ``steps`` (N,) steps per sequence,
    ``slots`` = S.  Slot s starts with queue[s]; at the end of every tick the slots whose sequence has run all its
    steps are freed and take, in slot order, the next waiting sequences of refill_queue(steps).
    Returns (ticks, placement): the number of ticks until every slot is idle, and the int64 array (N, 2) of every
    sequence's (slot, first tick), (-1, -1) for a sequence with 0 steps, which is never queued.  The host issues
    ``ticks`` steps and never asks the device how far it is."""
    import heapq
    steps = np.asarray(steps, np.int64).reshape(-1)
    if (steps < 0).any() or slots < 1:
        raise ValueError('plan_refill: steps must be >= 0 and slots >= 1')
    queue = refill_queue(steps)
    placement = np.full((len(steps), 2), -1, np.int64)
    head = queue[:slots]
    placement[head, 0] = np.arange(len(head))
    placement[head, 1] = 0
    ends = [(int(steps[q]), s) for s, q in enumerate(head)]           # (tick at which the slot is free again, slot)
    heapq.heapify(ends)
    nxt, ticks = len(head), 0
    while ends:
        tick, slot = heapq.heappop(ends)                              # equal ticks come out in slot order
        ticks = max(ticks, tick)
        if nxt < len(queue):
            q = queue[nxt]
            nxt += 1
            placement[q] = (slot, tick)
            heapq.heappush(ends, (tick + int(steps[q]), slot))
    return ticks, placement


class LockstepRefill(object):
    """One refilled run on the device: the slot table, the queue and every sequence's inputs uploaded once, one
    LockstepState of S slots, ``graph_steps`` ticks captured as a hipGraph (0 = eager) and replayed
    ceil(ticks / graph_steps) times; surplus ticks are device no-ops.

    Device memory besides the decoder state of S slots: the condition (N, condition_dim, T) floats as the caller holds
    it, the dense uniforms max_steps x N x n_uniform doubles and forced values max_steps x N, ``out`` N x T, with
    ``return_logits`` max_steps x N x out_dim floats (a test and inspection facility: 25 MB per 100 steps of 256
    sequences and classes), and 3 N + 2 S + 2 integers of table.  For a corpus of N = 300 utterances of up to 10 s at
    16 kHz the uniforms are 384 MB; the rows are dense because ragged storage would make a sequence's addresses
    depend on its neighbours' lengths."""

    def __init__(self, wavenet, condition, steps, u, forced, mode, group, return_logits=False, sampling=None):
        N, Cc, T = condition.shape
        steps = np.ascontiguousarray(steps, dtype=np.int32)
        queue = refill_queue(steps)
        self.n_slots = S = refill_slots(len(queue), group)
        self.ticks, self.placement = plan_refill(steps, S)
        max_steps = int(steps.max())
        softmax = mode == _lib.GEN_SOFTMAX
        st = self.state = LockstepState(wavenet, S)
        n_uniform = u.shape[2]
        self._keep = [condition,
                      backend.to_device(steps), backend.to_device(queue),
                      backend.to_device(np.ascontiguousarray(u[:max_steps]).reshape(-1))]
        self.out = backend.zeros((N, T), np.int32 if softmax else np.float32)
        self.logits_out = backend.zeros((max_steps, N, st.out_dim), np.float32) if return_logits else None
        self.slot_seq = backend.zeros((S,), np.int32)
        self.slot_t = backend.zeros((S,), np.int32)
        self.next = backend.zeros((1,), np.int32)
        self.live = backend.zeros((1,), np.int32)
        self.started = backend.to_device(np.full((N, 2), -1, np.int32))
        d = self.desc = st.desc
        d.sample_mode = mode
        d.cond, d.cond_bstride, d.cond_cstride, d.cond_follows_step = condition.ptr, Cc * T, T, 1
        d.uniforms, d.n_uniform = self._keep[3].ptr, n_uniform
        d.forced_next = None
        if forced is not None:
            self._keep.append(backend.to_device(np.ascontiguousarray(
                forced[:max_steps], dtype=np.int32 if softmax else np.float32).reshape(-1)))
            d.forced_next = self._keep[-1].ptr
        d.out, d.out_bstride = self.out.ptr, T
        d.logits_out = None if self.logits_out is None else self.logits_out.ptr
        d.max_steps = self.ticks
        t = self.table = _lib.GenSlots()
        t.n_seq, t.steps, t.queue, t.n_queue = N, self._keep[1].ptr, self._keep[2].ptr, len(queue)
        t.next, t.slot_seq, t.slot_t, t.live = self.next.ptr, self.slot_seq.ptr, self.slot_t.ptr, self.live.ptr
        t.started = self.started.ptr
        self._smp = None
        if sampling is not None:
            self._smp, controls = _upload_controls(sampling)
            self._keep.append(controls)
        self._graph = None
        _lib.call('vqvae_gen_slots_init', C.byref(d), C.byref(t), _S())

    def tick(self):
        _lib.call('vqvae_wavenet_gen_step_slots', C.byref(self.desc), C.byref(self.table),
                  None if self._smp is None else C.byref(self._smp), _S())

    def replay(self):
        """One more launch of the captured graph (``graph_steps`` ticks); past the end a device no-op."""
        _lib.call('vqvae_graph_launch', self._graph, _S())

    def run(self, graph_steps=8):
        if not graph_steps:
            for _ in range(self.ticks):
                self.tick()
        elif self.ticks:
            per = max(1, min(int(graph_steps), self.ticks))
            self._graph = C.c_void_p()
            _lib.call('vqvae_graph_capture_begin', _S())
            try:
                for _ in range(per):
                    self.tick()
            finally:
                _lib.call('vqvae_graph_capture_end', _S(), C.byref(self._graph))
            for _ in range((self.ticks + per - 1) // per):
                self.replay()
        backend.synchronize()
        return self

    def close(self):
        if self._graph is not None:
            backend.synchronize()
            _lib.call('vqvae_graph_destroy', self._graph)
            self._graph = None


def _device_refill_runner(wavenet, condition, mode, graph_steps, group, return_logits):
    def run(steps, u, forced, sampling):
        r = LockstepRefill(wavenet, condition, steps, u, forced, mode, group, return_logits, sampling)
        try:
            r.run(graph_steps)
            return r.out.get(), None if r.logits_out is None else r.logits_out.get()
        finally:
            r.close()
    return run


def run_lockstep_refill(wavenet, condition, uniforms, mode, n_steps=None, lengths=None, forced=None, return_logits=False,
                        graph_steps=8, group=_lib.GEN_MAX_LOCKSTEP, _run=None, sampling=None):
    """run_lockstep with the columns refilled on the device: ``group`` is the number of slots, a slot whose sequence
    has finished takes the next waiting one (longest first) at the next step, and the whole call is one replayed
    hipGraph with no host read-back until the end (csrc/generate_slots.hip; memory: see LockstepRefill).  Arguments
    and return value as run_lockstep; every sequence gets the values run_lockstep gives it, bit for bit.
    ``_run(steps, u, forced, sampling)`` -> (out (N, T), logits (max steps, N, out_dim) or None), both in the caller's
    order, stands in for the device in host tests."""
    if condition.ndim == 4:
        condition = condition.reshape(condition.shape[:3])
    N, Cc, T = condition.shape
    steps, _ = plan_lockstep(N, T, lengths, n_steps, group)              # the same step counts and argument errors
    softmax = mode == _lib.GEN_SOFTMAX
    out_dim = wavenet.proj2.W.shape[0]
    n_uniform = 1 if softmax else out_dim // 3
    u = np.asarray(uniforms, np.float64)
    max_steps = int(steps.max()) if N else 0
    if u.ndim < 2 or u.shape[1] != N:
        raise ValueError('generate_lockstep: uniforms must be (T, N[, %d]) = (%d, %d, ...), got %s'
                         % (n_uniform, T, N, u.shape))
    u = u.reshape(u.shape[0], N, -1)
    if u.shape[0] < max_steps or u.shape[2] < n_uniform:
        raise ValueError('generate_lockstep: need (%d, %d, %d) uniform doubles, got %s' % (max_steps, N, n_uniform, u.shape))
    if forced is not None:
        forced = np.asarray(forced).reshape(-1, N)
        if forced.shape[0] < max_steps:
            raise ValueError('generate_lockstep: forced must be (steps, N) = (%d, %d), got %s' % (max_steps, N, forced.shape))
    out = np.zeros((N, T), np.int32 if softmax else np.float32)                  # generate.py:103
    logits = np.zeros((max_steps, N, out_dim), np.float32) if return_logits else None
    if max_steps:
        run = _run or _device_refill_runner(wavenet, condition, mode, graph_steps, group, return_logits)
        o, lg = run(steps, u[:max_steps, :, :n_uniform], forced, sampling)
        for i in range(N):                        # the device wrote nothing past a sequence's own steps; a stub may have
            out[i, :steps[i]] = o[i, :steps[i]]
            if return_logits:
                logits[:steps[i], i] = lg[:steps[i], i]
    return (out, logits) if return_logits else out
