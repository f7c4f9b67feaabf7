/*
 * speaker_id.h -- per-speaker Gaussians over mel-cepstra and their deltas for a RAGGED list of utterances
 * (csrc/speaker_id.hip, part of libvqvae_hip.so): the device side of vqvae_amd.speakerid (speaker_features,
 * fit_speakers, score_speakers, identify_many): the features, the per-utterance first and second moments a speaker's
 * Gaussian is fitted from on the host, and the mean squared Mahalanobis distance of every utterance to every model.
 *
 * The entry points are additive and follow the conventions of include/vqvae_hip.h and the add-on headers: raw
 * device pointers, asynchronous on the given stream, 0 / hipError_t / VQVAE_E_INVALID return codes with
 * vqvae_last_error_string(), arguments validated before anything is launched, writes only inside the outputs, every
 * address formed in 64 bits.  No entry point needs a workspace.  This header is not under include/ and is in no table
 * of vqvae_amd/_lib.py: vqvae_amd/speakerid.py binds it itself and checks vqvae_spk_revision() there.
 *
 * The rule (normative).  Everything is float64, one rounding per operation, no contraction, every sum started from 0.0.
 * Utterance i owns the frames [frame_off[i], frame_off[i + 1]) = F frames; D = dim.
 *   1. Cepstra.  c[f, q] = sum_m (double)dct[q, m] * (double)log_mel[m, f], m ascending: step 1 of include/vqvae_align.h
 *      verbatim, so the static half of x equals vqvae_align_cepstra's output in every bit.
 *   2. Deltas (deltas = 1, D = 2 n_mcep; else D = n_mcep).  d[f, q] = 0.5 * (c[min(f + 1, last), q] - c[max(f - 1, first), q])
 *      with first and last the frame's own utterance's: one subtraction, then one product.  x[f] = [c[f, :], d[f, :]],
 *      frame-major: x[f * D + p].
 *   3. Gate (use_gate = 1).  e[f] = sum_m (double)log_mel[m, f], m ascending;  keep[f] = e[f] >= emax - thr, emax the
 *      largest e of the frame's utterance, thr a double from the host.  The loudest frame is always kept.  use_gate = 0:
 *      keep[f] = 1.  log_mel must be finite (the floor of the metrics' log sees to it).
 *   4. Lane reduce R over an utterance.  Lane t = (f - frame_off[i]) mod VQVAE_SPK_LANES adds the terms of its kept
 *      frames in ascending f to 0.0; then s[k] += s[k + h] for h = lanes / 2 .. 1; R = s[0].  A frame that is not kept
 *      adds nothing.
 *   5. Statistics.  cnt[i]: the kept frames.  s1[i, p] = R(x[f, p]).  s2[i, tri(p, q)] = R(x[f, p] * x[f, q]) for p <= q,
 *      the upper triangle row-major: tri(p, q) = p D - p (p - 1) / 2 + (q - p).
 *   6. Score.  For frame f and model g:  y_r = sum_{c = 0 .. r} linv[g, r, c] * (x[f, c] - mu[g, c]), c ascending;
 *      qf = sum_r y_r * y_r, r ascending;  q[i, g] = R(qf) / (double)cnt[i].  linv is handed over packed: the lower
 *      triangle row-major, linv[g, r, c] at g D (D + 1) / 2 + r (r + 1) / 2 + c.
 * A frame's features, an utterance's statistics and q[i, g] are pure functions of that utterance (and that model): the
 * same bits alone, in any list, at any position, beside any neighbour, for any n_models and any tiling of the models.  No
 * floating-point atomics, no matrix instructions, no exp or log on the device.
 *
 * An utterance whose table entries contradict the descriptor -- frame_off[0] other than 0, frame_off[n] other than ftot,
 * frame_off[i + 1] <= frame_off[i], an end above ftot -- is skipped and marked: cnt 0, NaN statistics, NaN q; a frame no
 * valid utterance owns gets NaN features and keep 0.
 */
#ifndef VQVAE_SPEAKER_ID_H_
#define VQVAE_SPEAKER_ID_H_

#include "../../include/vqvae_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VQVAE_SPK_MAX_DIM 48        /* D: n_mcep <= 24 with deltas; x[f] is 96 registers of a lane in the score kernel */
#define VQVAE_SPK_MAX_MELS 128      /* n_mels, as VQVAE_METRICS_MAX_MELS */
#define VQVAE_SPK_LANES 256         /* the workgroup and the lanes of R */
#define VQVAE_SPK_ACC_TILE 8        /* accumulators a lane of the statistics kernel carries at a time */
#define VQVAE_SPK_MODEL_TILE 8      /* models whose mu and linv one workgroup of the score kernel keeps in LDS */
#define VQVAE_SPK_MAX_MODELS 524280 /* n_models: 65535 tiles on the grid's second axis */

/* 1 */
int vqvae_spk_revision(void);

typedef struct {
  int32_t n;            /* utterances of this call, >= 1 */
  int32_t n_mels;       /* 1 .. VQVAE_SPK_MAX_MELS (read by vqvae_spk_features) */
  int32_t n_mcep;       /* 1 .. n_mels - 1 */
  int32_t deltas;       /* 0 or 1 */
  int32_t dim;          /* D = n_mcep * (1 + deltas), 1 .. VQVAE_SPK_MAX_DIM */
  int32_t n_models;     /* G, 1 .. VQVAE_SPK_MAX_MODELS for vqvae_spk_score; the others ignore it (>= 0) */
  int32_t use_gate;     /* 0 or 1 (read by vqvae_spk_features) */
  int32_t reserved;     /* 0 */
  int64_t ftot;         /* frames of this call = frame_off[n], >= n */
  int64_t stride;       /* elements between the mel rows of log_mel, >= ftot */
  double thr;           /* the gate's width in the units of e, finite and >= 0 when use_gate */
} vqvae_spk_desc;

/* Steps 1 to 3: log_mel (n_mels, stride) float32 with this call's first frame at log_mel[0], dct (n_mcep, n_mels) float32,
 * frame_off (n + 1,) int64 on the device; x (ftot, dim) float64, keep (ftot,) bytes of 0 or 1. */
int vqvae_spk_features(const vqvae_spk_desc* d, const float* log_mel, const float* dct, const int64_t* frame_off, double* x,
                       unsigned char* keep, vqvae_stream_t stream);

/* Steps 4 and 5, one workgroup per utterance: s1 (n, dim) and s2 (n, dim (dim + 1) / 2) float64, cnt (n,) int64. */
int vqvae_spk_stats(const vqvae_spk_desc* d, const double* x, const unsigned char* keep, const int64_t* frame_off, double* s1,
                    double* s2, int64_t* cnt, vqvae_stream_t stream);

/* Steps 4 and 6, one workgroup per utterance and tile of models: mu (n_models, dim) and linv (n_models, dim (dim + 1) / 2,
 * packed as above) float64 on the device; q (n, n_models) float64, cnt (n,) int64. */
int vqvae_spk_score(const vqvae_spk_desc* d, const double* x, const unsigned char* keep, const int64_t* frame_off,
                    const double* mu, const double* linv, double* q, int64_t* cnt, vqvae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif  /* VQVAE_SPEAKER_ID_H_ */
