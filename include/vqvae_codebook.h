/*
 * vqvae_codebook.h -- codebook usage statistics and dead-code re-seeding for the vector
 * quantiser (csrc/vq_codebook.hip, part of libvqvae_hip.so).
 *
 * The reference has no counterpart: with its plain codebook loss (net.py:85) a code that is
 * never selected receives a zero gradient for ever, and nothing reports how many codes are
 * alive.  These entry points are additive: they sit beside the ABI of vqvae_hip.h (same
 * conventions: raw device pointers, asynchronous on the given stream, 0 / hipError_t /
 * VQVAE_E_* return codes, vqvae_last_error_string()) and leave that ABI and its version alone.
 *
 * State.  Every buffer below is owned by the caller and persistent (never memory that a
 * recorded step recycles):
 *   counts      int32 [k]      histogram of the LAST observed step (zeroed by observe itself)
 *   usage       float32 [k]    running usage: counts of the first step, then
 *                              decay * usage + (1 - decay) * counts  (fp32, each operation rounded)
 *   reservoir   float32 [k,d]  one latent row per code, redrawn at every step: candidates for re-seeding
 *   steps_seen  int32 [1]      number of observe calls so far; the caller zeroes it once
 *   stats       float64 [VQVAE_CODEBOOK_STATS_WORDS]; the caller zeroes it to start an interval
 *                 [0] perplexity of the last step, exp(-sum_j p_j ln p_j), p_j = counts[j] / N
 *                 [1] number of codes with counts[j] > 0 in the last step
 *                 [2] sum of [0] over the calls since the caller zeroed the words
 *                 [3] sum of [1] over those calls
 *                 [4] number of those calls
 *                 [5..7] reserved, left alone
 *
 * Determinism.  The histogram is merged with INTEGER atomics only (LDS-privatised bins per
 * workgroup, one global integer add per non-empty bin): integer sums do not depend on arrival
 * order.  The statistics are reduced by one workgroup in a fixed order, in float64, without
 * atomics.  Every output is therefore the same bits from run to run.
 *
 * The largest k whose bins stay in LDS is VQVAE_CODEBOOK_LDS_MAX_K (64 KB of int32 bins per
 * workgroup); above it every index is one global integer atomic add.
 *
 * The reservoir hash (counter based, no state; all arithmetic modulo 2^64):
 *     ctr = (uint64(uint32(step)) << 32) | uint32(j)
 *     x   = seed + (ctr + 1) * 0x9E3779B97F4A7C15
 *     x  ^= x >> 30;  x *= 0xBF58476D1CE4E5B9
 *     x  ^= x >> 27;  x *= 0x94D049BB133111EB
 *     x  ^= x >> 31
 *     n_j = x mod N
 * with step = *steps_seen as observe found it.  Row n of the latents z (B,d,T) is
 * z[n / T, :, n mod T], the row vqvae_vq_nearest_fwd numbered n.
 */
#ifndef VQVAE_CODEBOOK_H_
#define VQVAE_CODEBOOK_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VQVAE_CODEBOOK_STATS_WORDS 8
#define VQVAE_CODEBOOK_LDS_MAX_K   16384

typedef void* vqvae_codebook_stream_t;     /* hipStream_t, as vqvae_stream_t */

/* 1; independent of vqvae_abi_version() */
int vqvae_codebook_abi_version(void);

/* One training step's observation; enqueues only (three kernels on `s`, no host-dependent argument
 * besides the shapes, decay and seed), so a recorded step may contain it and every replay does the
 * same work.  idx (B,T) int32 as vqvae_vq_nearest_fwd wrote it (values outside [0,k) are ignored),
 * z (B,d,T) the latents that were quantised, N = B*T.  In this order:
 *   counts <- histogram(idx);  usage <- first-step rule or the decayed blend, chosen by *steps_seen
 *   ON THE DEVICE;  stats[0..4] as above;  reservoir[j,:] <- z row n_j for every j;  *steps_seen += 1.
 * Needs no workspace.                                                                             */
int vqvae_codebook_observe(const int32_t* idx, const float* z, int B, int d, int T, int k,
                           float decay, uint64_t seed,
                           int32_t* counts, float* usage, float* reservoir, int32_t* steps_seen,
                           double* stats, vqvae_codebook_stream_t s);

/* For every code j with usage[j] < threshold:  W[j,:] <- reservoir[j,:],  m[j,:] = v[j,:] = 0 (the
 * Adam moments of W's slot; pass both or neither),  usage[j] <- revived_usage,  mask[j] <- 1.
 * Every other code keeps W, m, v and usage bit for bit and gets mask[j] <- 0.  *n_reseeded receives
 * the number of codes replaced (an integer sum).  W (k,d), mask int32 [k], n_reseeded int32 [1].  */
int vqvae_codebook_reseed(float* W, float* m, float* v, int k, int d, float* usage,
                          const float* reservoir, float threshold, float revived_usage,
                          int32_t* n_reseeded, int32_t* mask, vqvae_codebook_stream_t s);

#ifdef __cplusplus
}
#endif
#endif  /* VQVAE_CODEBOOK_H_ */
