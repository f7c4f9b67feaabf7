/*
 * vqvae_optim.h -- optimizer hooks on the device (csrc/optim_hooks.hip, part of libvqvae_hip.so):
 * the sum of squares of the flat gradient arena per parameter and in all, the state block that
 * global-norm clipping, the non-finite guard and the per-group norms read, and an Adam step that
 * takes its gradient scale and its skip decision from that block.
 *
 * The reference has no counterpart in its own text: chainer.optimizer.GradientClipping is what
 * its users add with optimizer.add_hook [chainer-recalled].  These entry points are additive:
 * they sit beside vqvae_hip.h, vqvae_codebook.h, vqvae_vq_ema.h and vqvae_kmeans.h (same
 * conventions: raw device pointers, asynchronous on the given stream, 0 / hipError_t / -1 return
 * codes with vqvae_last_error_string(), arguments validated before anything is launched, writes
 * only inside the outputs and ws[0, ws_bytes)) and leave the four ABIs and their versions alone.
 * vqvae_adam_step / vqvae_adam_step_dev are not touched: an optimizer without hooks launches them.
 *
 * The work-item table.  The gradient arena g[0, n) holds the parameters end to end.  Parameter p
 * occupies [off_p, off_p + size_p) and is cut into chunks of VQVAE_OPTIM_CHUNK elements counted
 * from off_p (the last one may be shorter); a parameter of size 0 has no chunk.  Item i is one
 * (parameter, chunk) pair, parameters in layout order, chunks in ascending order:
 *     items  int32 [n_items][2]  = (start, length)             element range [start, start + length)
 *     params int32 [n_params][2] = (first_item, item_count)
 * vqvae_optim_plan_items builds both on the host from the sizes alone.
 *
 * The summation order (a function of the table alone: not of the grid, the CU count, the
 * arrival order, eager or replayed execution).  Every g_i is widened to float64 and squared
 * (exact: 2 x 24 bits fit in 53), every addition below is one float64 addition.
 *   1. Inside a chunk [s, e): quad q holds the elements 4q .. 4q + 3 of the ARENA (aligned
 *      groups of four, whatever s is).  With q0 = s / 4, lane t (0 .. 255) takes the quads
 *      q0 + t, q0 + t + 256, ... below e, in that order, and inside a quad the elements in
 *      ascending order; elements outside [s, e) count +0 (adding +0 changes nothing):
 *          acc_t = 0;  acc_t = acc_t + g_i * g_i   for its elements in that order.
 *   2. The 256 lane sums are folded in halves: for h = 128, 64, ..., 1: v_t = v_t + v_{t+h}
 *      for t < h.  v_0 is the chunk's partial.
 *   3. S_p = 0; S_p = S_p + partial_c over the parameter's chunks in ascending order.
 *   4. S = 0; S = S + S_p over the parameters in layout order.
 *   5. A group's value is T = 0; T = T + S_p over its members in the order given; its norm is
 *      (float)sqrt(T).
 * No floating-point atomics; nothing is handed between workgroups inside a launch.  The same
 * arena and table give the same bits every time, on every device.
 * tests/optim_hooks_ref.py restates the order in NumPy.
 *
 * The state block (device memory, vqvae_optim_state_bytes(n_params, n_groups) bytes, 8-byte
 * aligned, owned by the caller, persistent between steps; zero it once before the first use):
 *     byte  0  float64  S          sum of squares over [0, n)
 *           8  float64  norm       sqrt(S)
 *          16  float64  rate       threshold / norm
 *          24  float32  scale      (float)rate if rate < 1, else 1.0f
 *          28  int32    nonfinite  !isfinite(S)
 *          32  int32    skipped    steps the guard has turned into a no-op so far (running)
 *          36  int32    steps      finalise launches so far (running); picks the row of the report ring
 *          40  float32  norm as float32        (what a report reads)
 *          44  float32  rate as float32
 *          48 .. 63     (reserved)
 *          64  float64  S_p [n_params]
 *          64 + 8 n_params   float32 group norms [n_groups]
 *          64 + 8 n_params + 4 n_groups   float32 report ring [n_slots][2 + n_groups]
 * The report ring keeps one row per step: launch number i (0-based, `steps` before the launch)
 * writes (norm, rate, group norms...) as float32 into row i mod n_slots, then advances `steps`.
 * A host that counts its own launches knows the row of every step without reading anything
 * back, so a log can hold one device scalar per step and read n_slots steps late at the most.
 * A NaN rate (norm is NaN or both are infinite) is not below 1: scale = 1.  A zero rate (norm
 * = +inf) gives scale = 0, and 0 * inf = NaN in the step: clipping does not mask a non-finite
 * gradient, as in Chainer.
 */
#ifndef VQVAE_OPTIM_H_
#define VQVAE_OPTIM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VQVAE_OPTIM_CHUNK         4096       /* elements per work item (a multiple of 4) */
#define VQVAE_OPTIM_THREADS       256        /* lanes of step 1, leaves of step 2 */
#define VQVAE_OPTIM_STATE_HEADER  64         /* bytes before S_p */
#define VQVAE_OPTIM_MAX_N         0x7fffffff /* elements of the arena (int32 table) */
#define VQVAE_OPTIM_GUARD         1          /* flags: the non-finite guard is present */

typedef void* vqvae_optim_stream_t;          /* hipStream_t, as vqvae_stream_t */

/* 1; independent of the four other versions */
int vqvae_optim_abi_version(void);

/* Pure host code.  sizes[n_params]: the parameters' element counts in layout order.  Returns
 * the number of work items (-1 for a negative size or more than VQVAE_OPTIM_MAX_N elements);
 * when items / params are not NULL they receive the table described above (items must hold
 * 2 * the returned count, params 2 * n_params int32). */
int vqvae_optim_plan_items(const int64_t* sizes, int n_params, int32_t* items, int32_t* params);

/* One float64 partial per work item. */
size_t vqvae_optim_workspace_bytes(int n_items);
size_t vqvae_optim_state_bytes(int n_params, int n_groups, int n_slots);

/* The norm pass and the finalise launch (two launches).  g float32 [n], 16-byte aligned;
 * items / params: the table, on the device; group_off int32 [n_groups + 1] and group_members
 * int32 [group_off[n_groups]] (parameter indexes), on the device, both may be NULL when
 * n_groups == 0; a bound of group_off outside [0, group_off[n_groups]] is clipped to it.
 * n_slots >= 1: rows of the report ring inside the state block.  threshold: of the clipping hook, +inf without one (rate = +inf, scale = 1).
 * flags & VQVAE_OPTIM_GUARD: `skipped` counts this step when S is not finite.  A table entry
 * that reaches outside [0, n) is clipped to it by the kernel; nothing outside g is read.
 * Rejected: null pointers, n < 1 or above VQVAE_OPTIM_MAX_N, n_items < 1, n_params < 1,
 * n_groups < 0, n_slots < 1, a misaligned g or state, ws_bytes below vqvae_optim_workspace_bytes(n_items). */
int vqvae_optim_sumsq(const float* g, size_t n, const int32_t* items, int n_items,
                      const int32_t* params, int n_params, const int32_t* group_off,
                      const int32_t* group_members, int n_groups, int n_slots, double threshold,
                      int flags, void* state, void* ws, size_t ws_bytes, vqvae_optim_stream_t s);

/* vqvae_adam_step / vqvae_adam_step_dev on g' = g * state.scale (one float32 product, then the
 * same expressions operation for operation).  lr_table == NULL: the step size is (float)lr_t;
 * else it is lr_table[*step] and *step advances by one behind the update (a second launch), as
 * in vqvae_adam_step_dev.  When state.scale != 1 the kernel writes g' back into g: the arena
 * then holds the clipped gradients.  With flags & VQVAE_OPTIM_GUARD and state.nonfinite set the
 * kernel returns before it touches p, m, v or g; *step advances all the same, so that the
 * device-side schedule stays where the host's step count is. */
int vqvae_optim_adam_step_hooked(float* p, float* g, float* m, float* v, size_t n, double lr_t,
                                 const float* lr_table, int32_t* step, double beta1, double beta2,
                                 double eps, const void* state, int flags, vqvae_optim_stream_t s);

#ifdef __cplusplus
}
#endif
#endif  /* VQVAE_OPTIM_H_ */
