/*
 * vqvae_ragged_decoder.h -- the teacher-forced decoder pass over a RAGGED list of utterances
 * (csrc/ragged_decoder.hip, part of libvqvae_hip.so): the device side of vqvae_amd.scoring (score_many,
 * evaluate_many): per-sample negative log-likelihood of held-out speech, per-utterance sums.
 *
 * The entry points are additive and follow the conventions of include/vqvae_hip.h and the add-on headers: raw
 * device pointers, asynchronous on the given stream, 0 / hipError_t / VQVAE_E_INVALID return codes with
 * vqvae_last_error_string(), arguments validated before anything is launched, writes only inside the outputs
 * and the queried workspace, every address formed in 64 bits.  Forward only, dropout off.  The header is an entry
 * of the header table of vqvae_amd/_lib.py like every other; its macros carry the file's stem, its functions and
 * typedefs the shorter vqvae_rdec_.
 *
 * The rule (normative).  Utterance i has L_i samples with classes q (int32, in [0, Q)), tl_i latent frames and
 * T_i = upscale * tl_i.
 *   - It contributes n_i = min(T_i, L_i - 1) >= 1 positions j = 0 .. n_i - 1.
 *   - The input at j is q[j]; the embed is W[:, q[j-1], 0] + W[:, q[j], 1] + b, without the first term at j = 0.
 *   - The target is q[j+1].
 *   - The condition is column j of the dense tensor as include/vqvae_gen_cond.h defines it: channels < Cl the
 *     align-corners linear up-sampling of the utterance's (Cl, tl_i) block with that header's (v0, w0, w1),
 *     channels >= Cl the utterance's global vector.
 *   - Block with dilation d:  h = Wd[:, :, 0] x[j-d] + Wd[:, :, 1] x[j] + bd + Wc c[j] + bc,  x[j-d] = 0 for j < d
 *                             z = tanh(h[:D/2]) * sigmoid(h[D/2:])
 *                             x' = Wr z + br + x
 *                             skip += Ws z + bs
 *   - Head: y = proj2(relu(proj1(relu(skip)))),  nll_j = logsumexp(y) - y[target],  hit_j = (argmax y == target),
 *     ties to the lowest index.
 *   - The utterances' n_i columns lie end to end with no padding: a ragged activation is ONE channel-major
 *     (C, ttot) float32 tensor, channel c of column j at x[c * ttot + j], utterance i owning columns
 *     [off[i], off[i + 1]).  Every tap checks its OWN utterance's bounds, and a tap before column 0 of its utterance
 *     is a selected zero, never a load.
 *
 * The condition is projected at the latent rate: Wc c[j] = lerp(Wc[:, :Cl] local)[j] + Wc[:, Cl:] global, since
 * the lerp is linear and its weights sum to one.  vqvae_rdec_cond_project computes P = Wc_all[:, :Cl] local for
 * ALL blocks over the ragged latent columns, vqvae_rdec_cond_global g[i] = Wc_all[:, Cl:] global_vec[i] + bias_all,
 * and the gate's epilogue adds fadd(fmul(w0, P[v0]), fmul(w1, P[v1])) + g[i].  lerp(Wc local) against
 * Wc lerp(local) is a rounding difference.
 *
 * Arithmetic (per vqvae_set_matmul_dtype), as in include/vqvae_ragged.h:
 *   0        fp32 operands on v_mfma_f32_32x32x2_f32.
 *   2 and 3  the exact three-way bf16 split of both operands, six products per 16-deep K step.
 *   1        refused.
 * No per-tensor scale, no split-K, no floating-point atomics; every output element has one fixed K order
 * (channel groups of 16 ascending, taps ascending inside a group) in every tile position and tile size.  A
 * position's NLL is a pure function of its utterance, the weights and its condition block: the same bits alone,
 * in any list, at any position, beside any neighbour, in any chunking.  The log-sum-exp of a column is two passes
 * over its Q logits in ascending class order (maximum, then the sum of expf(y - max)), then logf.
 * vqvae_rdec_reduce sums in float64 in one written order: lane t of 256 adds the utterance's elements t, t + 256,
 * ... in ascending order, then the 256 partial sums are folded pairwise, s[k] += s[k + h] for h = 128, 64 .. 1.
 */
#ifndef VQVAE_RAGGED_DECODER_H_
#define VQVAE_RAGGED_DECODER_H_

#include "vqvae_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VQVAE_RAGGED_DECODER_MAX_CLASSES 512   /* Q: the head keeps a column tile's logits in LDS */
#define VQVAE_RAGGED_DECODER_MAX_DILATION 512
#define VQVAE_RAGGED_DECODER_REDUCE_LANES 256

/* 1; independent of the other versions */
int vqvae_ragged_decoder_abi_version(void);

typedef struct {
  int32_t n;            /* utterances of this call, >= 1 */
  int32_t R, D, S, Q;   /* residual, dilated (even), skip channels; classes, 1 .. VQVAE_RAGGED_DECODER_MAX_CLASSES */
  int32_t Cl, G;        /* local / global condition channels, Cl >= 1, G >= 0 */
  int32_t n_blocks;     /* residual blocks, >= 1 */
  int32_t upscale;      /* samples per latent frame, >= 1 */
  int32_t reserved;     /* 0 */
  int64_t ttot;         /* sum of n_i = off[n], >= 1 */
  int64_t tltot;        /* sum of tl_i = latoff[n], >= 1 */
} vqvae_rdec_desc;

typedef struct {        /* device arrays; they are not checked */
  const int64_t* off;     /* (n + 1,) first column of every utterance, ascending from 0, off[n] = ttot */
  const int64_t* qoff;    /* (n,)     index of the utterance's first class in q; n_i + 1 classes are read from there */
  const int64_t* latoff;  /* (n + 1,) first latent column of every utterance, ascending from 0, latoff[n] = tltot */
  const int32_t* tl;      /* (n,)     latent frames, tl[i] = latoff[i + 1] - latoff[i] >= 1, n_i <= upscale * tl[i] */
} vqvae_rdec_tables;

/* Bytes of workspace vqvae_rdec_head needs (the (S, ttot) activation between proj1 and proj2); the other entry
 * points take none.  (size_t)-1 for a description the entry points would refuse. */
size_t vqvae_rdec_workspace_bytes(const vqvae_rdec_desc* d);

/* x[c, j] = (jl > 0 ? W[c, q[jl-1], 0] : 0) + W[c, q[jl], 1] + b[c]   -- W (R, Q, 2), b (R,) or NULL, x (R, ttot).
 * A class outside [0, Q) contributes 0 (the host layer refuses such classes before it calls). */
int vqvae_rdec_embed(const vqvae_rdec_desc* d, const vqvae_rdec_tables* t, const int32_t* q, const float* W,
                     const float* b, float* x, vqvae_stream_t stream);

/* P[m, latoff[i] + p] = sum_c Wc_all[m, c] local_i[c, p] for m < n_blocks * D, c < Cl: one GEMM over the ragged
 * latent columns.  local: utterance i a row-major (Cl, tl[i]) block at local + Cl * latoff[i] (LatentCondition.local);
 * Wc_all (n_blocks * D, Cl + G): the blocks' condition_proj weights stacked; P (n_blocks * D, tltot). */
int vqvae_rdec_cond_project(const vqvae_rdec_desc* d, const vqvae_rdec_tables* t, const float* local,
                            const float* Wc_all, float* P, vqvae_stream_t stream);

/* g[i, m] = (sum_c Wc_all[m, Cl + c] global_vec[i, c], c ascending in fp32) + bias_all[m]; bias_all (n_blocks * D,) holds
 * bc + bd of every block; global_vec (n, G) (may be NULL when G == 0); g (n, n_blocks * D). */
int vqvae_rdec_cond_global(const vqvae_rdec_desc* d, const float* global_vec, const float* Wc_all,
                           const float* bias_all, float* g, vqvae_stream_t stream);

/* Block `block` (0 <= block < n_blocks) with dilation 1 .. VQVAE_RAGGED_DECODER_MAX_DILATION: the two-tap dilated GEMM with the
 * gate in its epilogue, z (D / 2, ttot); h never reaches memory.  x (R, ttot), Wd (D, R, 2), P and g as written by the
 * two calls above (whole arrays: the block's rows are picked here). */
int vqvae_rdec_gate(const vqvae_rdec_desc* d, const vqvae_rdec_tables* t, int block, int dilation, const float* x,
                    const float* Wd, const float* P, const float* g, float* z, vqvae_stream_t stream);

/* One launch reads z once: x_out = Wr z + br + x_in (skipped when Wr == NULL: the last block) and
 * skip = (accumulate ? skip : 0) + (Ws z + bs).  Wr (R, D / 2), Ws (S, D / 2); x_out may be x_in (an element is read
 * and written by one thread). */
int vqvae_rdec_res_skip(const vqvae_rdec_desc* d, const float* z, const float* Wr, const float* br, const float* Ws,
                        const float* bs, const float* x_in, float* x_out, float* skip, int accumulate,
                        vqvae_stream_t stream);

/* s1 = relu(W1 relu(skip) + b1) into the workspace, y = W2 s1 + b2, then per column the log-sum-exp, the target
 * gather (target of column jl of utterance i: q[qoff[i] + jl + 1]) and the arg-max.  nll (ttot,) float32, hit (ttot,)
 * int32 0 / 1; logits (Q, ttot) or NULL.  A target outside [0, Q) gives nll = logsumexp(y) and hit = 0. */
int vqvae_rdec_head(const vqvae_rdec_desc* d, const vqvae_rdec_tables* t, const int32_t* q, const float* skip,
                    const float* W1, const float* b1, const float* W2, const float* b2, float* nll, int32_t* hit,
                    float* logits, void* ws, size_t ws_bytes, vqvae_stream_t stream);

/* nll_sum[i] = the float64 sum of the utterance's nll in the order written above, hits[i] = its hit count (int64). */
int vqvae_rdec_reduce(const vqvae_rdec_desc* d, const vqvae_rdec_tables* t, const float* nll, const int32_t* hit,
                      double* nll_sum, int64_t* hits, vqvae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif  /* VQVAE_RAGGED_DECODER_H_ */
