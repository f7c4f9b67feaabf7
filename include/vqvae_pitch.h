/*
 * vqvae_pitch.h -- pitch and voicing on the device (csrc/audio_pitch.hip, part of libvqvae_hip.so): a
 * per-frame YIN estimator over a RAGGED list of waveforms and the per-pair pitch statistics.  It is the
 * device side of vqvae_amd.pitch (pitch_many, compare_pitch_many): once the speaker of a synthesized wave
 * is not the input's, a spectral distance to the input says little; what is checked first is whether the
 * voicing and the contour are kept and where the mean log-F0 went.
 *
 * The entry points are additive and sit beside vqvae_hip.h and the other add-on headers (raw device
 * pointers, asynchronous on the given stream, 0 / hipError_t / VQVAE_E_INVALID return codes with
 * vqvae_last_error_string(), arguments validated before anything is launched, writes only inside the
 * outputs); the other ABIs, their versions and their kernels are not touched.  Forward only.  A program
 * that does not call them launches exactly what it launched before.
 *
 * The rule (normative).  No temporal smoothing, no octave correction: a frame's result is a pure function
 * of its own samples -- the same bits alone, in any list, at any position, in any chunking and in any
 * tile.  Samples are assumed finite.
 *
 * Configuration.  sr, frame, hop integers; fmin, fmax, threshold, min_power doubles.
 *   tau_min = floor(sr / fmax)      tau_max = ceil(sr / fmin)      W = frame - tau_max
 * (the divisions in float64).  Accepted: 2 <= tau_min < tau_max, W >= 2, frame <= VQVAE_PITCH_MAX_FRAME,
 * 1 <= hop <= frame, 0 < threshold < 1, min_power >= 0 (and sr >= 1, fmin > 0, fmax > 0, all finite).
 *
 * Framing (that of vqvae_metrics.h).  An utterance of L >= frame samples has F = 1 + (L - frame) / hop
 * frames (integer division).  Frame f reads samples [f * hop, f * hop + frame) of its OWN utterance and
 * nothing else; samples behind the last frame belong to no frame and are never loaded.  The utterances
 * of a call lie end to end along the frame axis: utterance i owns frames [frame_off[i], frame_off[i + 1]),
 * Ftot = frame_off[n]; frame fl of utterance i starts at x[off_in[i] + fl * hop].
 *
 * Arithmetic.  Every sample is converted to float64 (exact); everything below is float64 + - * / and
 * comparisons, each correctly rounded, never contracted into a fused multiply-add.
 *
 * The summation order S.  A sum of W terms t[0 .. W) is formed with FOUR accumulators a0 .. a3, each
 * starting from 0.0: term j is added to accumulator j mod 4, j ascending; the sum is (a0 + a1) + (a2 + a3).
 *
 * Difference function.  For tau = 1 .. tau_max:  d(tau) = S_j (x[j] - x[j + tau]) * (x[j] - x[j + tau]), j < W.
 * Power.  p = (S_j x[j] * x[j]) / W, j < W.
 * Normalised difference.  c(tau) = d(1) + ... + d(tau), added sequentially ascending from 0.0;
 *   d'(tau) = (d(tau) * tau) / c(tau), and 1 where c(tau) == 0; d'(0) = 1 (never needed below).
 * Power gate.  If p < min_power the frame is unvoiced with aperiodicity 1.
 * Pick.  Otherwise walk tau upward from tau_min.  At the first tau <= tau_max with d'(tau) < threshold,
 *   advance while tau + 1 <= tau_max and d'(tau + 1) < d'(tau); that tau is chosen.  If no tau qualifies
 *   the frame is unvoiced and its aperiodicity is the minimum of d' over [tau_min, tau_max].
 * Refinement.  If tau - 1 >= 1 and tau + 1 <= tau_max: with a, b, c = d'(tau - 1), d'(tau), d'(tau + 1) and
 *   q = (a - 2 * b) + c:  tau* = tau + (0.5 * (a - c)) / q  if q > 0, else tau* = tau.  Otherwise tau* = tau.
 * Outputs.  f0 = (float)(sr / tau*) in Hz, 0.0f for an unvoiced frame (so f0 > 0 IS the voicing decision);
 *   aperiodicity = (float) d'(tau) of the chosen tau, or the value stated above for an unvoiced frame.
 *
 * Pair statistics (vqvae_pitch_compare).  For pair i, `a` the reference and `b` the test, both tracked
 * over the SAME frames (the caller cuts both waves to their common length first), with F_i frames,
 * va = f0_a > 0, vb = f0_b > 0 and fa, fb the two f0 values converted to float64:
 *   out[i, 0] = voiced_ref        frames with va
 *   out[i, 1] = voiced_test       frames with vb
 *   out[i, 2] = voiced_both       frames with va and vb
 *   out[i, 3] = vuv_error         (frames with va != vb) / F_i
 *   out[i, 4] = gross_error       (both-voiced frames with |fb / fa - 1| > 0.2) / voiced_both
 *   out[i, 5] = f0_rmse_cents     sqrt((sum over both-voiced frames of (1200 * log2(fb / fa))^2) / voiced_both)
 *   out[i, 6] = log_f0_mean_ref   (sum over frames with va of log(fa)) / voiced_ref
 *   out[i, 7] = log_f0_mean_test  (sum over frames with vb of log(fb)) / voiced_test
 * One workgroup of VQVAE_PITCH_THREADS threads per pair; thread t takes frames t, t + 256, ... into one
 * accumulator per sum (the counts are integers, the three sums float64 starting from 0.0); the 256
 * partials are added in a binary tree (p[t] += p[t + h] for h = 128, 64, ..., 1); the divisions and the
 * square root follow as written, in float64.  The counts, vuv_error and gross_error are exact; log and
 * log2 are the device library's float64 functions, which are accurate to a few ulp and not correctly
 * rounded.  An empty set divides as IEEE divides: 0 / 0 = NaN.
 */
#ifndef VQVAE_PITCH_H_
#define VQVAE_PITCH_H_

#include "vqvae_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VQVAE_PITCH_THREADS 256        /* threads of a workgroup of either kernel */
#define VQVAE_PITCH_MAX_TILE 4         /* most frames of one workgroup of vqvae_pitch_yin */
#define VQVAE_PITCH_MAX_FRAME 2048
#define VQVAE_PITCH_COLUMNS 8          /* float64 values per pair of vqvae_pitch_compare */

/* 1; independent of the other versions */
int vqvae_pitch_abi_version(void);

typedef struct {
  int32_t n;            /* utterances, >= 1 */
  int32_t sr;           /* sample rate, >= 1 */
  int32_t frame;        /* samples of a frame, <= VQVAE_PITCH_MAX_FRAME */
  int32_t hop;          /* 1 <= hop <= frame */
  double fmin;          /* lowest and highest pitch looked for, Hz: tau_max = ceil(sr / fmin), */
  double fmax;          /*   tau_min = floor(sr / fmax) */
  double threshold;     /* 0 < threshold < 1 */
  double min_power;     /* >= 0: a frame whose mean power is below it is unvoiced */
  int64_t ftot;         /* frames of all utterances, = frame_off[n], >= 1 */
} vqvae_pitch_desc;

/* Bytes of workspace the two entry points need for this description: 0 today (a frame finds its
 * utterance by a search in frame_off; the difference function stays in LDS), queried like every other
 * entry point's.  (size_t)-1 for a description the entry point would refuse. */
size_t vqvae_pitch_yin_workspace_bytes(const vqvae_pitch_desc* d);
size_t vqvae_pitch_compare_workspace_bytes(const vqvae_pitch_desc* d);

/* f0 and aperiodicity of every frame of all utterances, ONE launch.
 *   x             float32, read at off_in[i] + p only for 0 <= p < frame + (F_i - 1) * hop
 *   off_in        int64 (n,)      first sample of every utterance (any order, gaps allowed: a corpus
 *                                 buffer is read in place)
 *   frame_off     int64 (n + 1,)  first frame of every utterance, ascending from 0, every utterance at
 *                                 least one frame; frame_off[n] = ftot
 *   f0            float32 (ftot,), or NULL
 *   aperiodicity  float32 (ftot,), or NULL -- at least one of the two
 *   ws            ws_bytes >= the query above (may be NULL when that is 0)
 * The tables are device data and are not checked.  Rejected: a null descriptor, x, off_in or frame_off;
 * both outputs null; n, ftot or sr < 1; a configuration outside the accepted ranges above; more than
 * 2^31 - 1 frame tiles; a workspace smaller than the query. */
int vqvae_pitch_yin(const vqvae_pitch_desc* d, const float* x, const int64_t* off_in, const int64_t* frame_off,
                    float* f0, float* aperiodicity, void* ws, size_t ws_bytes, vqvae_stream_t stream);

/* The eight statistics of every pair, ONE launch of n workgroups.
 *   f0_a, f0_b   float32 (ftot,)   reference, test
 *   frame_off    int64 (n + 1,), as above, the same for both sides
 *   out          float64 (n, VQVAE_PITCH_COLUMNS)
 * Rejected: a null descriptor or pointer; n or ftot < 1; a workspace smaller than the query.  Only n and
 * ftot of the description are read. */
int vqvae_pitch_compare(const vqvae_pitch_desc* d, const float* f0_a, const float* f0_b, const int64_t* frame_off,
                        double* out, void* ws, size_t ws_bytes, vqvae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif  /* VQVAE_PITCH_H_ */
