/*
 * vqvae_vq_ema.h -- exponential-moving-average codebook updates for the vector quantiser
 * (csrc/vq_ema.hip, part of libvqvae_hip.so).
 *
 * The second update rule of the VQ-VAE paper (van den Oord et al. 2017, appendix A.1): the
 * codebook is not trained by a gradient; every code tracks a running mean of the encoder
 * outputs assigned to it (online k-means).  The reference has no counterpart.  These entry
 * points are additive: they sit beside vqvae_hip.h and vqvae_codebook.h (same conventions: raw
 * device pointers, asynchronous on the given stream, 0 / hipError_t / -1 return codes with
 * vqvae_last_error_string(), arguments validated before anything is dereferenced) and leave
 * both ABIs and their versions alone.
 *
 * State, owned by the caller and persistent (never memory that a recorded step recycles):
 *   ema_count  float32 [k]        N_j, starts at 1
 *   ema_sum    float32 [k,d]      m_j, starts at W
 *   stats      float32 [k*(d+1)]  the last step's statistics: stats[j] = n_j, the number of rows
 *                                 with idx == j;  stats[k + j*d + c] = S_jc, the sum of z[row, c]
 *                                 over those rows.  One contiguous buffer: one float all-reduce
 *                                 sums it over data-parallel ranks.
 *
 * The rule (every float32 operation rounded on its own):
 *     w1    = 1.0f - decay
 *     N_j   = decay * N_j  + w1 * n_j
 *     m_jc  = decay * m_jc + w1 * S_jc
 *     total = sum_j (double) N_j             j = 0, 1, ..., k-1 in this order, float64
 *     Nt_j  = (float) (((double) N_j + eps) / (total + k * eps) * total)
 *     W_jc  = m_jc / Nt_j                    correctly rounded float32 division
 * total == 0 leaves W as it is.
 *
 * Determinism.  No floating-point atomics.  Row n of the latents z (B,d,T) is z[n / T, :, n mod T].
 * S_jc is summed in float64 over code j's rows r_0 < r_1 < ... in ONE order that depends on the
 * list alone, not on the launch shape, and rounded to float32 once:
 *     the list is cut into pieces of VQVAE_VQ_EMA_PIECE rows;
 *     inside a piece, lane l (0..63) adds entries l, l + 64, l + 128, ... in this order;
 *     the 64 lane sums are folded v[l] += v[l + h] for h = 32, 16, 8, 4, 2, 1;
 *     the piece sums are added in piece order.
 * Every output is therefore the same bits from run to run, from eager step to replayed step, and
 * between the small-N and the large-N launch structure.
 */
#ifndef VQVAE_VQ_EMA_H_
#define VQVAE_VQ_EMA_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VQVAE_VQ_EMA_PIECE       512         /* rows per piece of one code's list */
#define VQVAE_VQ_EMA_SMALL_MAX_N 4096        /* B*T up to which accumulate is ONE launch */
#define VQVAE_VQ_EMA_MAX_N       (1 << 24)   /* n_j is a float32: exact below 2^24 rows */

typedef void* vqvae_vq_ema_stream_t;         /* hipStream_t, as vqvae_stream_t */

/* 1; independent of vqvae_abi_version() and vqvae_codebook_abi_version() */
int vqvae_vq_ema_abi_version(void);

/* Bytes of workspace accumulate needs for these shapes (0 for shapes it rejects). */
size_t vqvae_vq_ema_workspace_bytes(int B, int d, int T, int k);

/* stats <- (n, S) of idx (B,T) int32 as vqvae_vq_nearest_fwd wrote it and the latents z (B,d,T)
 * that were quantised.  stats is OVERWRITTEN (every word, n_j = 0 and S_j = 0 for a code without
 * a row), indices outside [0,k) are ignored.  Enqueues only; no launch depends on a value read
 * by the host, so a recorded step may contain it.  B*T <= VQVAE_VQ_EMA_SMALL_MAX_N: one kernel,
 * a workgroup per code; above: bucket the rows (stable counting sort), then sum per piece.
 * B*T >= VQVAE_VQ_EMA_MAX_N is rejected.  Writes only inside stats and ws[0, ws_bytes).        */
int vqvae_vq_ema_accumulate(const int32_t* idx, const float* z, int B, int d, int T, int k,
                            float* stats, void* ws, size_t ws_bytes, vqvae_vq_ema_stream_t s);

/* The rule above: ema_count, ema_sum and W (k,d) updated in place from stats.  Two kernels.
 * decay in [0,1], eps > 0.                                                                    */
int vqvae_vq_ema_apply(float* W, float* ema_count, float* ema_sum, const float* stats, int k,
                       int d, float decay, float eps, vqvae_vq_ema_stream_t s);

/* ema_count[j] <- 1, ema_sum[j,:] <- W[j,:] for every j (mask == NULL) or for the rows with
 * mask[j] != 0 (int32 [k]); every other row keeps its state bit for bit.  One kernel.          */
int vqvae_vq_ema_reset(const float* W, float* ema_count, float* ema_sum, int k, int d,
                       const int32_t* mask, vqvae_vq_ema_stream_t s);

#ifdef __cplusplus
}
#endif
#endif  /* VQVAE_VQ_EMA_H_ */
