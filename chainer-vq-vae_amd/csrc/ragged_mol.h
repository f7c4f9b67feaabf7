/*
 * ragged_mol.h -- the mixture-of-logistics side of the teacher-forced decoder pass over a RAGGED list of utterances
 * (csrc/ragged_mol.hip, part of libvqvae_hip.so): the device side of vqvae_amd.scoring_mol (score_many_mol,
 * evaluate_many_mol): the raw-sample embed of an input_dim = 1 decoder and the per-position negative log-likelihood of
 * the discretised mixture of logistics (WaveNet.calculate_logistic_loss, modules.py:169-230, without the mean).
 *
 * The entry points are additive and follow the conventions of include/vqvae_hip.h and the add-on headers: raw
 * device pointers, asynchronous on the given stream, 0 / hipError_t / VQVAE_E_INVALID return codes with
 * vqvae_last_error_string(), arguments validated before anything is launched, writes only inside the outputs, every
 * address formed in 64 bits.  No entry point needs a workspace.  This header is not under include/ and is in no table
 * of vqvae_amd/_lib.py: vqvae_amd/scoring_mol.py binds it itself and checks vqvae_rdmol_revision() there.
 *
 * The rule (normative).  Utterance i has L_i float32 samples w, tl_i latent frames and T_i = upscale * tl_i.
 *   - It contributes n_i = min(T_i, L_i - 1) >= 1 positions jl = 0 .. n_i - 1.  The column layout, the condition, the
 *     blocks and the head's two GEMMs are those of include/vqvae_ragged_decoder.h, unchanged.
 *   - Input at jl, sample form (embed W of shape (R, 1, 2)):
 *       x[c, j] = (jl > 0 ? W[c, 0, 0] * w[jl - 1] : nothing) + W[c, 0, 1] * w[jl] (+ b[c])
 *     in float32: two products, one sum, then the bias, no contraction; at jl = 0 the second product alone, then the bias.
 *   - Input at jl, class form (embed W of shape (R, Qin, 2), 1 < Qin <= VQVAE_RAGGED_DECODER_MAX_CLASSES): the classes
 *     of vqvae_mulaw_bins with the streaming path's Qin thresholds, through vqvae_rdec_embed.
 *   - The target at jl is the sample w[jl + 1], as a float in both forms (utils.py:106-107).
 *   - y = proj2(relu(proj1(relu(skip)))) has 3 M rows: M logits, M means, M log-scales, 1 <= M <= VQVAE_RDMOL_MAX_MIX.
 *     vqvae_rdec_head computes it with a descriptor whose Q is 3 M and leaves it in its `logits` output.
 *   - nll_j, in float32 by ONE thread per column, with half = 127.5 / (quantize - 1) rounded to float32:
 *       t = 127.5 * w[jl + 1];  left = t < 127.5f * -0.999f;  right = t > 127.5f * 0.999f
 *       lz = log(sum_k exp(logit_k - max_k logit_k)) + max_k logit_k                    (k ascending, maximum first)
 *       per component k ascending:  ls = max(logscale_k, log_scale_min);  c = t - mean_k;  is = exp(-ls)
 *         p = is * (c + half);  q = is * (c - half);  sigmoid(v) = tanh(v * 0.5) * 0.5 + 0.5
 *         softplus(v) = max(v, 0) + log1p(exp(-|v|))
 *         lpr = left ? p - softplus(p) : right ? -softplus(q) : log(max(sigmoid(p) - sigmoid(q), 1e-12))
 *         v_k = lpr + (logit_k - lz)
 *       nll_j = -(log(sum_k exp(v_k - max_k v_k)) + max_k v_k)                          (k ascending, maximum first)
 *     the operation sequence of mol_kernel<0> (csrc/misc.hip) per position.
 *   - The per-utterance sum is vqvae_rdec_reduce's: float64 in its written order.
 * A position's NLL is a pure function of its utterance, the weights and its condition block: the same bits alone, in any
 * list, at any position, beside any neighbour, in any chunking, and read in place from a corpus buffer.  No bit equality
 * with vqvae_mol_nll_fwd or the training forward is claimed.  No atomics; plain vector stores to (row < rows of the
 * output, column < ttot) only.
 */
#ifndef VQVAE_RAGGED_MOL_H_
#define VQVAE_RAGGED_MOL_H_

#include "../../include/vqvae_ragged_decoder.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VQVAE_RDMOL_MAX_MIX 16      /* M: a thread keeps a column's components in registers, as vqvae_mol_nll_fwd does */

/* 1 */
int vqvae_rdmol_revision(void);

/* The sample-form embed.  w: a float32 device buffer; woff (n,) int64 on the device: the element of w that holds the first
 * sample of every utterance (n_i + 1 samples are readable from there; the utterances may lie anywhere in w, in any
 * order).  W (R, 1, 2), b (R,) or NULL, x (R, ttot).  Of t only off is read; of d only n, R and ttot, but the whole
 * descriptor must be one the ragged decoder accepts. */
int vqvae_rdmol_embed(const vqvae_rdec_desc* d, const vqvae_rdec_tables* t, const float* w, const int64_t* woff,
                      const float* W, const float* b, float* x, vqvae_stream_t stream);

/* The per-position NLL.  y (3 n_mix, ttot) channel-major as vqvae_rdec_head's `logits`; the target of column jl of
 * utterance i is w[woff[i] + jl + 1]; nll (ttot,) float32.  Refused without a launch: null pointers, a descriptor the
 * ragged decoder refuses, n_mix outside 1 .. VQVAE_RDMOL_MAX_MIX, d->Q != 3 n_mix, quantize < 2. */
int vqvae_rdmol_nll(const vqvae_rdec_desc* d, const vqvae_rdec_tables* t, const float* y, const float* w,
                    const int64_t* woff, int n_mix, int quantize, float log_scale_min, float* nll, vqvae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif  /* VQVAE_RAGGED_MOL_H_ */
