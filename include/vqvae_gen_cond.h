/*
 * vqvae_gen_cond.h -- the condition of lockstep generation kept at the latent rate
 * (csrc/generate_cond.hip, part of libvqvae_hip.so): one small launch at the head of a step computes, for every
 * column of the step, the ONE condition column that step reads, from the latent-rate tensor and the speaker vector
 * the full-rate condition is an up-sampling of (net.py:54-63).  The step's kernels then read that compact column
 * through the descriptor as it stands (cond = column, cond_bstride = cond_dim, cond_cstride = 1,
 * cond_follows_step = 0), so the (n, cond_dim, T) tensor never exists: 4 (Cl + G) bytes per sample of audio become
 * 4 Cl / upscale bytes plus one speaker vector per sequence.
 *
 * The entry point is additive and sits beside vqvae_hip.h, vqvae_sampling.h and vqvae_gen_slots.h (same
 * conventions: raw device pointers, asynchronous on the given stream, 0 / hipError_t / VQVAE_E_INVALID return codes
 * with vqvae_last_error_string(), arguments validated before anything is launched, writes only inside `column`); the
 * other ABIs, their versions and their kernels are not touched.
 *
 * Semantics.  Sequence q has tl[q] >= 1 latent frames and T_q = upscale * tl[q] samples.  Its row (q, t) is
 *   channels ch >= Cl:  global_vec[q][ch - Cl], copied;
 *   channels ch <  Cl:  with x = the channel's latent row local[local_off[q] + ch * tl[q] ...]
 *       t >= T_q        0 (a shorter member of a group keeps running; nothing is read out of range);
 *       tl[q] == 1      v0 = v1 = 0, w0 = 0.f, w1 = 1.f;
 *       otherwise       v = t * ((tl - 1) / (T_q - 1)) in float64, v = tl - 1 exactly at t = T_q - 1;
 *                       v0 = clamp(floor(v), 0, tl - 2), v1 = v0 + 1;
 *                       w0 = (float)((double)v1 - v), w1 = (float)(v - (double)v0);
 *       value           fadd(fmul(w0, x[v0]), fmul(w1, x[v1])), each rounded to nearest, not contracted.
 * This is the align-corners linear up-sampling of vqvae_upsample_linear_fwd with the tables NumPy's
 * linspace(0, tl - 1, T_q) gives (vqvae_amd.functions.resize_tables_host), so a row carries the bits of column t of
 * the dense tensor.
 *   Plain  (slots == NULL): column c < d->n holds sequence q = col_seq ? col_seq[c] : c at t = *d->step and is
 *          written to row c of `column`, which has d->n rows.  The launch is a device no-op when
 *          *d->step >= d->max_steps.
 *   Slots: column c holds q = slot_seq[c] at t = slot_t[c] and is written to row q (the step's kernels address the
 *          condition by the sequence), so `column` has n_seq rows; idle slots (q < 0) write nothing.  The launch is a
 *          device no-op when *d->step >= d->max_steps or *live == 0.
 * A column whose sequence id is outside 0..n_seq-1 writes nothing.  Replays of a captured graph past the end stay
 * no-ops and read nothing.
 */
#ifndef VQVAE_GEN_COND_H_
#define VQVAE_GEN_COND_H_

#include "vqvae_gen_slots.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1; independent of the other versions */
int vqvae_gen_cond_abi_version(void);

typedef struct {     /* device arrays unless said otherwise */
  const float*   local;      /* ragged: sequence q is a row-major (Cl, tl[q]) block at local + local_off[q]; no padding */
  const int64_t* local_off;  /* (n_seq,) offsets in floats */
  const int32_t* tl;         /* (n_seq,) latent frames of every sequence, each >= 1 */
  const float*   global_vec; /* (n_seq, G) the speaker embedding row of every sequence */
  const int32_t* col_seq;    /* (d->n,) plain form: the sequence in column c; NULL: the identity.  Not read with slots */
  float*         column;     /* out: (rows, Cl + G); rows = d->n (plain) or n_seq (slots) */
  int            n_seq;      /* host: sequences */
  int            Cl;         /* host: local (latent) channels */
  int            G;          /* host: speaker embedding channels */
  int            upscale;    /* host: samples per latent frame, >= 1 */
} vqvae_gen_latent_cond;

/* One launch, one pass over the d->n columns.  Capturable into a hipGraph; meant to be issued in front of
 * vqvae_wavenet_gen_step[_sampled] (slots == NULL) or vqvae_wavenet_gen_step_slots on the same stream.
 * Rejected before the launch: a null c, d or d->step; a null local, local_off, tl or column, a null global_vec with
 * G > 0; n_seq, Cl or G negative; Cl + G != d->cond_dim; upscale < 1; d->n outside 1..VQVAE_GEN_MAX_LOCKSTEP; with
 * slots, a null slot_seq, slot_t or live and slots->n_seq != c->n_seq. */
int vqvae_gen_cond_column(const vqvae_gen_latent_cond* c, const vqvae_gen_desc* d, const vqvae_gen_slots* slots,
                          vqvae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif  /* VQVAE_GEN_COND_H_ */
