/*
 * vqvae_sampling.h -- sampling controls for generation on the device (csrc/sampling.hip, part of
 * libvqvae_hip.so): temperature, top-k and nucleus (top-p) truncation and greedy decoding, per
 * sequence, applied in the finish launch of a generation step.
 *
 * The reference draws from the raw softmax (generate.py:135-141) or from untempered logistic
 * samples (generate.py:113-133) and has no such controls; these entry points are additive.  They
 * sit beside vqvae_hip.h, vqvae_codebook.h, vqvae_vq_ema.h, vqvae_kmeans.h and vqvae_optim.h
 * (same conventions: raw device pointers, asynchronous on the given stream, 0 / hipError_t / -1
 * return codes with vqvae_last_error_string(), arguments validated before anything is launched,
 * writes only inside the outputs) and leave the five ABIs and their versions alone.
 * vqvae_wavenet_gen_step, vqvae_gen_desc and the persistent kernel (vqvae_wavenet_gen_run) are
 * not touched: a call without controls launches what it launched before, and the persistent
 * kernel has no filtered form.
 *
 * Semantics, softmax output.  One sequence at one step has float32 logits l[0, O), the uniform
 * double u in [0, 1) of numpy.random.choice, and its own temperature, top_k, top_p.
 *   Rank.    Classes are totally ordered by (logit descending, index ascending): equal logits
 *            (-0 equals +0) go to the lower index.  Everything below is defined on this order.
 *   Greedy.  temperature == 0: the rank-0 class; u is not read.
 *   top-k.   Ranks < top_k are kept (decided on the raw logits); 0 or >= O: all.
 *   Temperature.  x = l * (1.0f / temperature) in float32 (temperature 1: x = l bit for bit);
 *            over the kept classes m = max x, e = expf(x - m), p = e / sum(e) in float32, the sum
 *            in the order of vqvae_wavenet_gen_step's own softmax (classes outside count +0).
 *   top-p.   After top-k, on p: walk the kept classes in rank order adding p in float64 (one
 *            sequential sum) and keep the shortest prefix whose mass is >= (double)top_p; it is
 *            never empty.  >= 1: all.
 *   Draw.    Classes outside the kept set get p = 0; then numpy.random.choice: float64 cumulative
 *            sum in index order, divided by its last element, the number of entries <= u.  With
 *            u < 1 this is a kept class.
 * Rank, the prefix sum and the cumulative sum are each done in one fixed order by one workgroup
 * per sequence: no floating-point atomics, and a sequence's result does not depend on n or on its
 * position in the batch.  tests/sampling_ref.py restates all of it in NumPy.
 *
 * Mixture of logistics: temperature > 0 only.  The mixture weights are softmax(logit_probs *
 * (1.0f / temperature)), every component's scale is expf(max(log_scale, log_scale_min)) *
 * temperature (float32), the rest is generate.py:113-127.  top_k and top_p must be NULL.
 *
 * The control values are read on the device, so the host cannot reject a bad one: a temperature
 * that is negative, NaN or infinite counts as 1, a top_k < 0 as 0, a top_p that is NaN or <= 0 as
 * 1, and temperature 0 with the mixture output as 1.  Callers validate before they upload
 * (vqvae_amd.generation.sampling_controls does).  A temperature so small that l / temperature
 * overflows float32 gives NaN probabilities, as non-finite logits do.
 */
#ifndef VQVAE_SAMPLING_H_
#define VQVAE_SAMPLING_H_

#include "vqvae_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VQVAE_SAMPLING_MAX_CLASSES 1024   /* out_dim of the softmax output (classes held in LDS) */

/* 1; independent of the five other versions */
int vqvae_sampling_abi_version(void);

typedef struct {            /* device arrays of d->n entries; NULL = neutral for every sequence */
  const float* temperature; /* >= 0; 0 = greedy (softmax output only) */
  const int*   top_k;       /* 0 or >= out_dim = off */
  const float* top_p;       /* >= 1 = off; must be > 0 */
} vqvae_gen_sampling;

/* vqvae_wavenet_gen_step with the controls applied in the finish launch; s == NULL or all three
 * NULL: exactly vqvae_wavenet_gen_step.  Capturable into a hipGraph like it.  With controls the
 * step's last two launches are the filtered sampler (one workgroup per sequence, for every n) and
 * the step counter's advance.  Rejected besides what vqvae_wavenet_gen_step rejects: controls with
 * sample_mode VQVAE_GEN_NONE, top_k or top_p with VQVAE_GEN_MOL. */
int vqvae_wavenet_gen_step_sampled(const vqvae_gen_desc* d, const vqvae_gen_sampling* s, vqvae_stream_t st);

/* The sampler alone, for tests and for callers with logits of their own: logits (n, out_dim),
 * uniforms (n, n_uniform) doubles, mode = VQVAE_GEN_SOFTMAX / VQVAE_GEN_MOL; s may be NULL.
 * out: int32 (n,) or float (n,); probs_out (n, out_dim) or NULL: the filtered, renormalised
 * probabilities the draw used, (float)(p / last element of the cumulative sum), 0 outside the
 * kept set (softmax mode only).
 * Rejected: null logits / uniforms / out, n < 1, out_dim < 1 or > VQVAE_SAMPLING_MAX_CLASSES,
 * n_uniform < 1, another mode; with VQVAE_GEN_MOL also out_dim % 3 != 0, n_uniform < out_dim / 3,
 * top_k, top_p or probs_out not NULL. */
int vqvae_sample_logits(const float* logits, int n, int out_dim, int mode, float log_scale_min,
                        const double* uniforms, int n_uniform, const vqvae_gen_sampling* s,
                        void* out, float* probs_out, vqvae_stream_t st);

#ifdef __cplusplus
}
#endif
#endif  /* VQVAE_SAMPLING_H_ */
