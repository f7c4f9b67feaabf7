/*
 * vqvae_gen_slots.h -- lockstep generation with refill (csrc/generate_slots.hip, part of
 * libvqvae_hip.so): the columns of a lockstep step are SLOTS, and a slot whose sequence has
 * finished takes the next waiting sequence from a queue, on the device, so that sequences of
 * different lengths keep every column busy (continuous batching).
 *
 * The entry points are additive and sit beside vqvae_hip.h and vqvae_sampling.h (same
 * conventions: raw device pointers, asynchronous on the given stream, 0 / hipError_t /
 * VQVAE_E_INVALID return codes with vqvae_last_error_string(), arguments validated before anything
 * is launched, writes only inside the outputs and the state); the other ABIs and their versions,
 * vqvae_wavenet_gen_step[_sampled] and the persistent kernel are not touched.
 *
 * Semantics.  d->n = S slots, 5..VQVAE_GEN_MAX_LOCKSTEP, one per MFMA column.  n_seq sequences;
 * sequence q runs steps[q] >= 1 steps; `queue` lists the sequences to run in serving order (the
 * caller leaves sequences with 0 steps out: a queued sequence runs at least one step).
 *   Table.     slot_seq[s] = the sequence in slot s or -1 (idle); slot_t[s] = that sequence's own
 *              step; next = the queue position of the next waiting sequence; live = the number of
 *              slots that hold a sequence; d->step = the global TICK, which indexes the rings as
 *              tick % dilation and nothing else.
 *   A tick     is the launch sequence of vqvae_wavenet_gen_step at n = S.  What belongs to a
 *              sequence is addressed by (seq, t = slot_t): cond[seq*cond_bstride + c*cond_cstride
 *              + t], uniforms[(t*n_seq + seq)*n_uniform], forced_next[t*n_seq + seq],
 *              logits_out[(t*n_seq + seq)*out_dim], out[seq*out_bstride + t], the sampling
 *              controls [seq].  What belongs to the machine stays addressed by the slot: x_cur,
 *              x_prev, h0, h1, z, skip_acc, s1, logits and the rings (dilation, S, residual).
 *   Fresh      sequences see fresh queues without any buffer being cleared: a ring entry is read
 *              as 0 while slot_t < dilation (the entry under tick % dilation was pushed by the
 *              slot's previous tenant, or never), and the finish launch of a sequence's last step
 *              writes zeros to the slot's x_cur and x_prev instead of the feedback.
 *   Idle       slots are treated like columns >= n: operands read as 0, no pointer is derived
 *              from their sequence id, nothing is stored for them.
 *   Scheduler. The last launch of a tick, one wavefront, no atomics: every live slot's slot_t
 *              advances; a slot whose slot_t reaches steps[seq] is free; the free slots, in slot
 *              order, take queue[next], queue[next + 1], ... (a prefix count over a ballot, so
 *              the assignment is a function of steps, queue and S alone); when the queue is
 *              exhausted a free slot goes idle and `live` drops; the tick advances.  With
 *              `started` the scheduler records (slot, first tick) of every sequence.
 *   End.       Every kernel of a tick returns at once when live == 0 or tick >= d->max_steps, so
 *              calls (and replays of a captured graph) past the end are device no-ops, and the
 *              host never reads anything back while the run is going: the number of ticks is a
 *              function of steps, queue and S (vqvae_amd.generation.plan_refill computes it).
 * A sequence's values do not depend on S, on its slot, on its start tick or on its neighbours:
 * bit for bit what vqvae_wavenet_gen_step[_sampled] gives it at any n of 5..128.
 */
#ifndef VQVAE_GEN_SLOTS_H_
#define VQVAE_GEN_SLOTS_H_

#include "vqvae_sampling.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1; independent of the other versions */
int vqvae_gen_slots_abi_version(void);

typedef struct {     /* device arrays unless said otherwise */
  int        n_seq;    /* host: sequences, the row count of uniforms / forced_next / logits_out / out */
  const int* steps;    /* (n_seq,) steps of every sequence; >= 1 for a queued one */
  const int* queue;    /* (n_queue,) sequence ids in serving order, each at most once */
  int        n_queue;  /* host: 0..n_seq */
  int*       next;     /* (1,) */
  int*       slot_seq; /* (d->n,) */
  int*       slot_t;   /* (d->n,) */
  int*       live;     /* (1,) */
  int*       started;  /* (n_seq, 2) {slot, first tick} or NULL; rows of sequences never started are not written */
} vqvae_gen_slots;

/* Fills the table from the head of the queue (slot s takes queue[s] at its step 0, s < n_queue;
 * the other slots are idle), sets next and live, records the placements in `started`, and zeroes
 * the tick d->step.  The state vectors x_cur and x_prev and the rings are the caller's to zero
 * before the first run (the rings need it only for the reader's peace of mind: they are not read
 * before they are written).  Rejected: a null d, slots or table member (started may be NULL),
 * null d->step, d->n outside 5..VQVAE_GEN_MAX_LOCKSTEP, n_seq < 0, n_queue < 0 or > n_seq. */
int vqvae_gen_slots_init(const vqvae_gen_desc* d, const vqvae_gen_slots* slots, vqvae_stream_t stream);

/* One tick.  Capturable into a hipGraph like vqvae_wavenet_gen_step.  s == NULL or all three NULL:
 * the plain sampler; else the filtered sampler of vqvae_sampling.h with the controls read at [seq].
 * Rejected before any launch, besides what vqvae_gen_slots_init and
 * vqvae_wavenet_gen_step[_sampled] reject: sample_mode VQVAE_GEN_NONE without logits_out. */
int vqvae_wavenet_gen_step_slots(const vqvae_gen_desc* d, const vqvae_gen_slots* slots,
                                 const vqvae_gen_sampling* s, vqvae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif  /* VQVAE_GEN_SLOTS_H_ */
