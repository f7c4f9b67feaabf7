/*
 * abx.h -- DTW distances of a RAGGED list of short item pairs over frame features (csrc/abx.hip, part of
 * libvqvae_hip.so): the device side of vqvae_amd.abx (pair_distances, abx, abx_many, ResidentCorpus.abx, code_table).
 * An item is a run of frames cut out of an utterance (a phone, a word); ABX discriminability asks, for items A and X of
 * one category and B of another, how often X lies nearer to B than to A under such a distance.  The triples and their
 * scores are formed on the host (vqvae_amd/abx.py); this header is the distances.
 *
 * The entry points are additive and follow the conventions of include/vqvae_hip.h and the add-on headers: raw device
 * pointers, asynchronous on the given stream, 0 / hipError_t / VQVAE_E_INVALID return codes with
 * vqvae_last_error_string(), arguments validated before anything is launched, a *_workspace_bytes query, writes only
 * inside the outputs and the queried workspace, every address formed in 64 bits.  This header is not under include/ and
 * is in no table of vqvae_amd/_lib.py: vqvae_amd/abx.py binds it itself and checks vqvae_abx_revision() there.
 *
 * The rule (normative).  Pair i compares the Fa = a_len[i] frames of side a that start at frame a_start[i] with the
 * Fb = b_len[i] frames of side b that start at b_start[i].  The pair is ORDERED: a is a and b is b.  Items may overlap
 * and may repeat, and the two sides may be one buffer or two.  Everything is float64, one rounding per operation, no
 * contraction; every sum runs with j ascending and starts from 0.0.
 *   1. Norms.  n[f] = sum_j x[j, f] * x[j, f], with x[j, f] the float32 feature widened to float64.
 *   2. Local cost of frame i of a and frame j of b.
 *      cosine:     q = n_a[i] * n_b[j];  q == 0: d = 1.0;  else dot = sum_j xa * xb, c = dot / sqrt(q), d = 1.0 - c, and
 *                  d = 0.0 when d < 0.  A frame against itself is exactly 0.0.
 *      euclidean:  d = sqrt(sum_j (xa - xb) * (xa - xb)), each term one subtraction, one product, one addition.
 *      codes form: d = table[ca[i] * k + cb[j]] for a (k, k) float64 table; a code outside [0, k) gives NaN.
 *      A cell's value does not depend on how the pair is tiled.
 *   3. Recurrence: step 3 of include/vqvae_align.h.  D(0, 0) = d(0, 0); otherwise D(i, j) = best + d(i, j) with best
 *      chosen from D(i-1, j-1), D(i-1, j), D(i, j-1) in that order: the first that exists is taken, a later one replaces
 *      it only when it is strictly smaller (<).  Every cell carries the length K of its path in cells (K(0, 0) = 1, else
 *      the chosen predecessor's + 1).  No direction is kept and no diagonal step is counted.
 *      cost = D(Fa-1, Fb-1), path_len = K(Fa-1, Fb-1), distance = cost / (double)path_len.
 *      Because of the candidate order, swapping the sides of a pair can change K on exact ties.
 *   4. A pair whose table entries contradict the descriptor -- an item outside [0, ftot) of its side, a length below 1,
 *      a shorter side above max_short, more than 2^31 cells, cells outside [0, cells) -- is skipped and marked: cost and
 *      distance NaN, path_len 0, and nothing else is written for it.
 * A pair's three outputs are a pure function of its two items and the metric: the same bits alone, in any list, at any
 * position, beside any neighbour and in any chunking.  No floating-point atomics, no matrix instructions.
 */
#ifndef VQVAE_ABX_H_
#define VQVAE_ABX_H_

#include "../../include/vqvae_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VQVAE_ABX_MAX_D 4096        /* channels of the dense form */
#define VQVAE_ABX_MAX_K 8192        /* codes of the codes form and of vqvae_abx_table */
#define VQVAE_ABX_WAVE_SHORT 64     /* min(Fa, Fb) up to here: one wavefront per pair, the diagonals in registers */
#define VQVAE_ABX_MAX_SHORT 1024    /* min(Fa, Fb) of a pair: three diagonals of (D, K) in 36 KB of LDS */
#define VQVAE_ABX_LANES 256         /* the DP workgroup above VQVAE_ABX_WAVE_SHORT and the cell-wise kernel's */
#define VQVAE_ABX_TILE 16           /* the local-cost kernel's tile: 16 x 16 frames on one wavefront, 2 x 2 cells a lane */
#define VQVAE_ABX_COSINE 0
#define VQVAE_ABX_EUCLIDEAN 1
#define VQVAE_ABX_DENSE 0
#define VQVAE_ABX_CODES 1

/* 1 */
int vqvae_abx_revision(void);

typedef struct {
  int32_t n;            /* pairs of this call, >= 1 */
  int32_t d;            /* channels, 1 .. VQVAE_ABX_MAX_D (dense form; not read in the codes form) */
  int32_t metric;       /* VQVAE_ABX_COSINE or VQVAE_ABX_EUCLIDEAN (dense form; not read in the codes form) */
  int32_t form;         /* VQVAE_ABX_DENSE: (d, stride) float32 features; VQVAE_ABX_CODES: int32 codes and a table */
  int32_t k;            /* codes form: 1 .. VQVAE_ABX_MAX_K; dense form: not read */
  int32_t max_short;    /* the largest min(Fa, Fb) of this call, 1 .. VQVAE_ABX_MAX_SHORT: chooses the DP's form */
  int64_t ftot_a;       /* frames of side a's buffer, >= 1 */
  int64_t ftot_b;       /* frames of side b's buffer, >= 1 */
  int64_t stride_a;     /* dense form: elements between the channel rows of side a, >= ftot_a */
  int64_t stride_b;     /* the same for side b, >= ftot_b */
  int64_t cells;        /* sum of Fa * Fb over the pairs: the float64 cells of the workspace */
} vqvae_abx_desc;

typedef struct {        /* device arrays, (n,) each */
  const int64_t* a_start;   /* first frame of the pair's item on side a */
  const int64_t* b_start;   /* the same on side b */
  const int32_t* a_len;     /* Fa */
  const int32_t* b_len;     /* Fb */
  const int64_t* cell_off;  /* first cell of the pair's local-cost table in the workspace */
} vqvae_abx_tables;

/* Bytes of workspace of vqvae_abx_local and vqvae_abx_dtw: `cells` float64, padded to 256 bytes.  (size_t)-1 for a
 * descriptor the entry points would refuse. */
size_t vqvae_abx_workspace_bytes(const vqvae_abx_desc* d);

/* Step 1 for one side (0: a, ftot_a frames with stride_a; 1: b): x (d, stride) float32, n (ftot,) float64.  Only d, the
 * side's ftot and stride are read beyond validation. */
int vqvae_abx_norms(const vqvae_abx_desc* d, int side, const float* x, double* n, vqvae_stream_t stream);

/* Step 2: the local-cost table of every pair into the workspace, pair i's (Fa, Fb) row-major at cell_off[i].
 * Dense form: xa, xb float32 features, na, nb the norms of vqvae_abx_norms (cosine; may be NULL for euclidean), table
 * NULL.  Two launches: the sums on 16 x 16 tiles, then sqrt and division cell by cell.  Codes form: xa, xb int32 codes
 * (ftot,), table (k, k) float64; one launch. */
int vqvae_abx_local(const vqvae_abx_desc* d, const vqvae_abx_tables* t, const void* xa, const void* xb, const double* na,
                    const double* nb, const double* table, void* workspace, size_t workspace_bytes, vqvae_stream_t stream);

/* Step 3 over the workspace vqvae_abx_local filled: cost (n,) float64, path_len (n,) int32, distance (n,) float64.
 * max_short <= VQVAE_ABX_WAVE_SHORT: one wavefront per pair; above: VQVAE_ABX_LANES lanes per pair. */
int vqvae_abx_dtw(const vqvae_abx_desc* d, const vqvae_abx_tables* t, const void* workspace, size_t workspace_bytes,
                  double* cost, int32_t* path_len, double* distance, vqvae_stream_t stream);

/* Steps 1 and 2 over the rows of a codebook W (k, d) float32, row against row: table (k, k) float64.  The workspace
 * holds the k norms: vqvae_abx_table_workspace_bytes(k), (size_t)-1 for a refused k. */
size_t vqvae_abx_table_workspace_bytes(int32_t k);
int vqvae_abx_table(int32_t k, int32_t d, int32_t metric, const float* W, double* table, void* workspace,
                    size_t workspace_bytes, vqvae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif  /* VQVAE_ABX_H_ */
