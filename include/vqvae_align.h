/*
 * vqvae_align.h -- dynamic time warping over mel-cepstra for a RAGGED list of utterance pairs
 * (csrc/audio_align.hip, part of libvqvae_hip.so): the device side of vqvae_amd.alignment (align_many,
 * compare_aligned_many): mel-cepstral distortion along the warping path (MCD-DTW), the log-mel distance along it, and
 * the path itself.
 *
 * The entry points are additive and follow the conventions of include/vqvae_hip.h and the add-on headers: raw
 * device pointers, asynchronous on the given stream, 0 / hipError_t / VQVAE_E_INVALID return codes with
 * vqvae_last_error_string(), arguments validated before anything is launched, writes only inside the outputs
 * and the queried workspace, every address formed in 64 bits.  The header is an entry of the header table of
 * vqvae_amd/_lib.py like every other.
 *
 * The rule (normative).  Everything is float64, one rounding per operation, no contraction.  Pair i aligns the Fa
 * frames of side a with the Fb frames of side b; nothing is cut to a common length.
 *   1. Cepstra.  c[f, q] = sum_m (double)dct[q, m] * (double)log_mel[m, f], m ascending from 0, for the n_mcep rows of
 *      the metrics' dct table (coefficients 1 .. n_mcep; c0 is left out), stored frame-major: c[f * n_mcep + q].
 *   2. Local cost.  d(i, j) = C * sqrt(2 * s),  s = sum_q (0.5 * (ca[i, q] - cb[j, q]))^2, q ascending from 0, added to
 *      0.0;  C = 4.3429448190325175 (10 / ln 10, the constant of csrc/audio_metrics.hip).
 *   3. Recurrence.  Symmetric steps, no slope weights, no band.  D(0, 0) = d(0, 0).  Otherwise D(i, j) = best + d(i, j),
 *      where best is chosen from D(i-1, j-1) [direction 0], D(i-1, j) [1], D(i, j-1) [2] in that order: the first that
 *      exists is taken, a later one replaces it only when it is strictly smaller (<).  A candidate outside the matrix
 *      does not exist.  The chosen direction is kept per cell (3 at the start cell).  Every cell carries the length K of
 *      its path in cells (K(0, 0) = 1, else the chosen predecessor's + 1) and the count of direction-0 steps on it.
 *   4. Outputs.  cost = D(Fa-1, Fb-1);  K and diagonal_steps of that cell;  mcd_dtw = cost / (double)K;
 *      log_mel_mae_dtw: the path's K * n_mels terms |(double)la[m, ia[k]] - (double)lb[m, ib[k]]|, term e = k * n_mels + m:
 *      lane t of VQVAE_ALIGN_REDUCE_LANES adds terms t, t + lanes, ... in ascending order to 0.0, the partial sums are
 *      folded pairwise, s[k] += s[k + h] for h = lanes / 2 .. 1, and s[0] is divided by (double)(K * n_mels).
 *   5. Backtrack.  From (Fa-1, Fb-1) by the kept directions until the start cell; step s (0 at the end cell) is written
 *      at position K - 1 - s, so ia and ib ascend from (0, 0) to (Fa-1, Fb-1).
 * A pair's results are a pure function of its own two feature blocks and the dct table: the same bits alone, in any
 * list, at any position and in any chunking.  No floating-point atomics, no pair is split across workgroups.
 *
 * VQVAE_ALIGN_MAX_SHORT.  vqvae_align_dtw walks the anti-diagonals i + j = k with one workgroup per pair and keeps the
 * current diagonal and the two before it in LDS: D as double, K and the diagonal count as int32, 16 bytes per cell.  A
 * diagonal has at most min(Fa, Fb) cells, so a pair takes 48 * min(Fa, Fb) bytes.  A compute unit of the MI355X has
 * 160 KiB = 163840 bytes of LDS, which allows min(Fa, Fb) <= 3413; the bound is 3072 (144 KiB), the largest multiple of
 * 1024 below that: 49 s at a hop of 256 samples of 16 kHz audio on the SHORTER side.  The longer side is bounded only by
 * Fa * Fb <= 2^31 cells (one direction byte per cell, addressed per pair).
 *
 * The direction table of a pair (in vqvae_align_dtw's workspace, read by vqvae_align_path) is laid out diagonal by
 * diagonal so that a diagonal's cells are consecutive bytes: with S = min(Fa, Fb), L = max(Fa, Fb), p the cell's
 * coordinate on the shorter side (i when Fa <= Fb, else j) and k = i + j, the cell is byte
 *      cell_off[pair] + start(k) + p - max(0, k - (L - 1)),
 *      start(k) = first(k) for k <= L, else S * L - first(S + L - 1 - k),
 *      first(n) = n (n + 1) / 2 for n <= S, else S (S + 1) / 2 + (n - S) S.
 */
#ifndef VQVAE_ALIGN_H_
#define VQVAE_ALIGN_H_

#include "vqvae_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VQVAE_ALIGN_MAX_SHORT 3072     /* min(Fa, Fb) of a pair: three diagonals of 16-byte cells in 160 KiB of LDS */
#define VQVAE_ALIGN_MAX_MELS 128       /* n_mels, as VQVAE_METRICS_MAX_MELS */
#define VQVAE_ALIGN_THREADS 256        /* the DP's workgroup: a longer diagonal is looped over */
#define VQVAE_ALIGN_REDUCE_LANES 256

/* 1; independent of the other versions */
int vqvae_align_abi_version(void);

typedef struct {
  int32_t n;            /* pairs of this call, >= 1 */
  int32_t n_mels;       /* 1 .. VQVAE_ALIGN_MAX_MELS */
  int32_t n_mcep;       /* 1 .. n_mels - 1 */
  int32_t max_short;    /* the largest min(Fa, Fb) of this call, 1 .. VQVAE_ALIGN_MAX_SHORT: sizes the LDS */
  int64_t fa_tot;       /* sum of Fa = off_a[n], >= n */
  int64_t fb_tot;       /* sum of Fb = off_b[n], >= n */
  int64_t stride_a;     /* elements between the mel rows of side a's log_mel, >= fa_tot */
  int64_t stride_b;     /* the same for side b, >= fb_tot */
  int64_t cells;        /* sum of Fa * Fb = cell_off[n] */
  int64_t ptot;         /* sum of Fa + Fb - 1 = path_off[n]: the capacity of ia and ib */
} vqvae_align_desc;

typedef struct {        /* device arrays; a pair whose entries contradict the descriptor is skipped (K = 0, NaN scores) */
  const int64_t* off_a;     /* (n + 1,) first frame of every pair on side a, ascending from 0 */
  const int64_t* off_b;     /* (n + 1,) the same on side b */
  const int64_t* cell_off;  /* (n + 1,) first direction byte of every pair, ascending from 0 */
  const int64_t* path_off;  /* (n + 1,) first path position of every pair, ascending from 0 */
} vqvae_align_tables;

/* Bytes of workspace of each entry point: cepstra none; dtw the direction table, `cells` bytes; path the path of every
 * pair as int32 ia and ib (8 * ptot bytes; used only when ia or ib is NULL).  (size_t)-1 for a description the entry
 * points would refuse. */
size_t vqvae_align_cepstra_workspace_bytes(const vqvae_align_desc* d);
size_t vqvae_align_dtw_workspace_bytes(const vqvae_align_desc* d);
size_t vqvae_align_path_workspace_bytes(const vqvae_align_desc* d);

/* Step 1 for one side (side 0: a, fa_tot frames with stride_a; side 1: b): log_mel (n_mels, stride) float32 with this
 * call's first frame at log_mel[0], dct (n_mcep, n_mels) float32, c (ftot, n_mcep) float64. */
int vqvae_align_cepstra(const vqvae_align_desc* d, int side, const float* log_mel, const float* dct, double* c,
                        void* ws, size_t ws_bytes, vqvae_stream_t stream);

/* Steps 2 and 3, one workgroup per pair: ca (fa_tot, n_mcep), cb (fb_tot, n_mcep) as written above; cost (n,) float64,
 * path_len (n,) and diagonal_steps (n,) int32; the direction table goes to the workspace (`cells` bytes). */
int vqvae_align_dtw(const vqvae_align_desc* d, const vqvae_align_tables* t, const double* ca, const double* cb,
                    double* cost, int32_t* path_len, int32_t* diagonal_steps, void* ws, size_t ws_bytes,
                    vqvae_stream_t stream);

/* Steps 5 and 4: dirs is vqvae_align_dtw's workspace, cost and path_len its outputs.  ia and ib (ptot,) int32, pair i at
 * [path_off[i], path_off[i] + path_len[i]); both NULL: the path is kept in the workspace only.  scores (n, 2) float64:
 * mcd_dtw and log_mel_mae_dtw.  log_mel_a and log_mel_b as given to vqvae_align_cepstra. */
int vqvae_align_path(const vqvae_align_desc* d, const vqvae_align_tables* t, const void* dirs, const double* cost,
                     const int32_t* path_len, const float* log_mel_a, const float* log_mel_b, int32_t* ia, int32_t* ib,
                     double* scores, void* ws, size_t ws_bytes, vqvae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif  /* VQVAE_ALIGN_H_ */
