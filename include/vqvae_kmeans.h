/*
 * vqvae_kmeans.h -- k-means initialisation of the vector quantiser's codebook over real
 * encoder outputs (csrc/vq_kmeans.hip, part of libvqvae_hip.so): exact k-means++ seeding,
 * the centroid update of Lloyd's algorithm with a rule for empty clusters, and the inertia.
 *
 * The reference has no counterpart.  These entry points are additive: they sit beside
 * vqvae_hip.h, vqvae_codebook.h and vqvae_vq_ema.h (same conventions: raw device pointers,
 * asynchronous on the given stream, 0 / hipError_t / -1 return codes with
 * vqvae_last_error_string(), arguments validated before anything is dereferenced, writes only
 * inside the outputs and ws[0, ws_bytes)) and leave the three ABIs and their versions alone.
 *
 * The sample pool is `pool` float32 (d, N), N contiguous: the latents' own (B, d, T) layout
 * with B = 1, T = N.  One Lloyd iteration is
 *     vqvae_vq_nearest_fwd(pool, W, 1, d, N, k, 0, idx, NULL, ...)     the assignment
 *     vqvae_vq_ema_accumulate(idx, pool, 1, d, N, k, stats, ...)       counts and cluster sums
 *     vqvae_kmeans_update(pool, N, d, k, stats, seed, iter, W, ...)    the centroids
 *
 * Distances.  dist(x, c) is the squared L2 distance in the exact search's float32 operation
 * order (vqvae_hip.h, the VQ comment): acc = 0; for c = 0 .. d-1: df = x_c - c_c;
 * acc = acc + df * df, every operation rounded on its own.
 *
 * The summation tree.  Every float64 sum over rows (the seeding's total, the inertia) is ONE
 * sum whose order depends on N alone: the values v_0 .. v_{N-1} (float32 widened to float64)
 * are padded with +0 to a power of two P >= N and added pairwise,
 *     node(0, i) = v_i,   node(l, i) = node(l-1, 2i) + node(l-1, 2i+1),   total = the root.
 * Adding +0 is exact, so every P gives the same bits.  The kernels cut the rows into blocks of
 * VQVAE_KMEANS_BLOCK rows (a node of level 8 each) and finish the tree over the block sums in
 * a single workgroup.
 *
 * k-means++.  Round 0 takes row x_0 mod N.  Round j >= 1 first lowers
 * D_i = min(D_i, dist(row i, centre j-1)) for every row (D starts at +inf), builds the tree
 * over D and, with t = u_j * total (one float64 product), walks down from the root: at a node
 * with children (L, R) it goes left when t < L or R is not positive, else right with t - L.
 * In exact arithmetic the leaf it ends at is the first row whose running sum of D exceeds
 * u_j * total (D^2 sampling); in float64 it is that row up to the rounding of the tree's own
 * sums, always a row with D > 0, and the same row from run to run.  total == 0 (every row
 * coincides with a chosen centre) takes row x_j mod N instead and is not an error.
 *
 * The hash (counter based, no state; all arithmetic modulo 2^64), vqvae_codebook.h's:
 *     ctr = (uint64(uint32(word)) << 32) | uint32(j)
 *     x   = seed + (ctr + 1) * 0x9E3779B97F4A7C15
 *     x  ^= x >> 30;  x *= 0xBF58476D1CE4E5B9
 *     x  ^= x >> 27;  x *= 0x94D049BB133111EB
 *     x  ^= x >> 31
 * Seeding round j: word = 0, x_j = x, u_j = (x >> 40) * 2^-24 (24 bits, so u_j * total < total
 * after rounding).  vqvae_kmeans_update of Lloyd iteration `iter`, code j: word = iter + 1.
 *
 * Determinism.  No floating-point atomics, nothing that depends on a value the host reads back
 * in the middle.  Every output is the same bits from run to run.
 */
#ifndef VQVAE_KMEANS_H_
#define VQVAE_KMEANS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VQVAE_KMEANS_BLOCK  256          /* rows per block sum: a node of level 8 of the tree */
#define VQVAE_KMEANS_MAX_N  (1 << 24)    /* vqvae_vq_ema_accumulate's limit: N below it */
#define VQVAE_KMEANS_MAX_D  4096         /* channels */

typedef void* vqvae_kmeans_stream_t;     /* hipStream_t, as vqvae_stream_t */

/* 1; independent of the three other versions */
int vqvae_kmeans_abi_version(void);

/* Bytes of workspace vqvae_kmeans_seed and vqvae_kmeans_inertia need (0 for shapes they reject):
 * the round's centre (d floats) and one float64 per block of rows. */
size_t vqvae_kmeans_workspace_bytes(int N, int d, int k);

/* pool[:, row0 .. row0 + count - 1] <- the first `count` rows of the latents z (B,d,T); row n
 * of z is z[n / T, :, n mod T] (vqvae_vq_ema.h's convention).  One launch.  1 <= count <= B*T,
 * row0 >= 0 and row0 + count <= N, else rejected. */
int vqvae_kmeans_collect(const float* z, int B, int d, int T, int count, float* pool, int N,
                         int row0, vqvae_kmeans_stream_t s);

/* Exact k-means++ as stated above.  W (k,d) <- the chosen rows, rows int32 [k] <- their
 * indices, mind float32 [N] <- the final D (the distance of every row to its nearest chosen
 * row).  Two launches per round (distances and block sums; a single workgroup that finishes
 * the tree, picks the row and copies it into W and into the next round's centre), 2k in all.
 * k > N is allowed (the surplus rounds meet total == 0).  N < 1, N >= VQVAE_KMEANS_MAX_N,
 * k < 1, d < 1, d > VQVAE_KMEANS_MAX_D are rejected. */
int vqvae_kmeans_seed(const float* pool, int N, int d, int k, uint64_t seed, float* W,
                      int32_t* rows, float* mind, void* ws, size_t ws_bytes,
                      vqvae_kmeans_stream_t s);

/* From stats as vqvae_vq_ema_accumulate wrote it (stats[j] = n_j, stats[k + j*d + c] = S_jc):
 * W_jc <- S_jc / n_j (one correctly rounded float32 division) where n_j > 0; a code with
 * n_j == 0 takes pool row x mod N of the hash above (word = iter + 1).  *n_empty (device int32)
 * receives the number of such codes (an integer sum).  iter >= 0.  Two launches. */
int vqvae_kmeans_update(const float* pool, int N, int d, int k, const float* stats,
                        uint64_t seed, int iter, float* W, int32_t* n_empty,
                        vqvae_kmeans_stream_t s);

/* *out (device float64) <- sum_i dist(row i, W[idx_i]) over the summation tree; a row whose
 * idx is outside [0,k) counts +0.  Two launches. */
int vqvae_kmeans_inertia(const float* pool, const float* W, const int32_t* idx, int N, int d,
                         int k, double* out, void* ws, size_t ws_bytes,
                         vqvae_kmeans_stream_t s);

#ifdef __cplusplus
}
#endif
#endif  /* VQVAE_KMEANS_H_ */
