/*
 * vqvae_ingest.h -- from decoded audio files to the waveforms a device-resident corpus holds (csrc/ingest.hip, part of
 * libvqvae_hip.so): interleaved int16 or float32 frames at any sample rate go in; mono, band-limited resampled,
 * silence-trimmed, peak-normalised float32 comes out, the steps of the reference's Preprocess (utils.py:56-59:
 * librosa.load(path, sr, res_type), librosa.effects.trim(raw, top_db), raw /= abs(raw).max()).  Three launches per
 * batch of utterances; the file parser (RIFF/WAVE) is Python (vqvae_amd.ingest).
 *
 * The entry points are additive and sit beside vqvae_hip.h and the other add-on headers (same conventions as
 * vqvae_corpus.h: raw device pointers, asynchronous on the given stream, 0 / hipError_t / VQVAE_E_INVALID return codes
 * with vqvae_last_error_string(), arguments validated before anything is launched, writes only inside the outputs and
 * the queried workspace); the other ABIs, their versions and their kernels are not touched.  Every sum below has one
 * float64 accumulator and a fixed order, nothing is accumulated with atomics and the device evaluates no
 * transcendental, so the results are the same bits from call to call and equal an exact NumPy restatement
 * (vqvae_amd.ingest, tests/ingest_ref.py).
 *
 * The rule (normative).
 *
 * Decode to mono.  A frame holds `channels` interleaved samples, int16 (VQVAE_INGEST_I16) or float32
 * (VQVAE_INGEST_F32).  An int16 v is v / 32768 (exact).  The mono sample is the float64 sum of the frame's channels in
 * channel order, divided by `channels`, rounded to float32.
 *
 * Resample from sr_in to sr_out.  g = gcd(sr_in, sr_out), L = sr_out / g, M = sr_in / g; s = min(1, L / M);
 * J = ceil(Z / s), in integers Z when L >= M and ceil(Z M / L) otherwise; n_out = ceil(n_in L / M) in integers.
 * The tap table h[p][j], p in [0, L), j in [-J + 1, J], stored row-major with j ascending (row p, column j + J - 1), is
 * an INPUT of the entry point.  Python computes it in float64 and rounds it to float32:
 *   u = s * (p / L - j)
 *   w(v) = I0(beta * sqrt(1 - v * v)) / I0(beta) for |v| < 1, else 0
 *   h = ((s * rho) * sinc(rho * u)) * w(u / Z)
 * with numpy.sinc (sin(pi x) / (pi x)) and numpy.i0, every operation in the order written.
 * Output o: q = (o M) div L, p = (o M) mod L,
 *   y[o] = float32( sum over j = -J + 1 .. J, ascending, of double(x[q + j]) * double(h[p][j]) )
 * with one float64 accumulator that starts at 0 and x = 0 outside [0, n_in).  Each product of two float32 values is
 * exact in float64, so fused and unfused multiply-adds give the same bits.  L == M (sr_in == sr_out) is a copy of the
 * mono samples; the table is not read.
 * Presets [resampy-recalled] (the parameters of resampy's filters as remembered, not verified against the package):
 *   'kaiser_fast': Z = 16, rho = 0.85,               beta = 8.555504641634386
 *   'kaiser_best': Z = 64, rho = 0.9475937167399596, beta = 14.769656459379492
 * No bit parity with librosa is claimed: resampy samples the windowed sinc at 512 or 8192 points per zero crossing and
 * interpolates that table linearly, this rule computes every phase's taps exactly.
 *
 * Trim (librosa.effects.trim [librosa-recalled]: frame_length 2048, hop_length 512, centred frames with reflect
 * padding, the reference power is the maximum).  F = 2048, H = 512, amin = 1e-10, on the resampled signal y of
 * n >= F / 2 + 1 samples.  nf = 1 + n div H frames.  Sample m of frame t is y[i], i = t H + m - F / 2, reflected
 * once: i < 0 -> -i, i >= n -> 2 (n - 1) - i.  The frame energy E_t in a fixed order:
 *   a_l = sum over r = 0 .. 31, sequential, of double(y[i(l + 64 r)])^2, for l in [0, 64);
 *   for stride = 32, 16, ..., 1: a_l += a_(l + stride) for l < stride;
 *   E_t = a_0.
 * mse_t = E_t / F; ref = max(amin, max over t of mse_t); thr = ref * r, where r = 10.0 ** (-top_db / 10.0) is an
 * argument (a double computed by the caller, top_db > 0).  Frame t is non-silent iff max(amin, mse_t) > thr in
 * float64.  With t_first and t_last the first and the last non-silent frame,
 *   start = H t_first, end = min(n, H (t_last + 1)).
 *
 * Normalise.  peak = max |y[i]| over [start, end); out[i] = y[start + i] / peak, a correctly rounded float32 division
 * (numpy's float32 / float32).
 *
 * Status, per utterance: VQVAE_INGEST_BAD_SAMPLE (1) a non-finite sample anywhere in y: then start = 0, end = n,
 * peak = 0 and no other bit is set; VQVAE_INGEST_ZERO_PEAK (2) peak == 0; VQVAE_INGEST_EMPTY (4) end <= start.
 */
#ifndef VQVAE_INGEST_H_
#define VQVAE_INGEST_H_

#include "vqvae_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VQVAE_INGEST_I16 0
#define VQVAE_INGEST_F32 1
#define VQVAE_INGEST_BAD_SAMPLE 1
#define VQVAE_INGEST_ZERO_PEAK 2
#define VQVAE_INGEST_EMPTY 4
#define VQVAE_INGEST_TILE 1024             /* consecutive outputs of one utterance per workgroup of the resampler */
#define VQVAE_INGEST_MAX_TAPS (1 << 22)    /* entries of the tap table: L * 2J at most */
#define VQVAE_INGEST_MAX_WINDOW 16384      /* mono samples a tile's input window may hold: (TILE - 1) M / L + 2J + 1 */

/* 1; independent of the other versions */
int vqvae_ingest_abi_version(void);

/* What trim_bounds writes per utterance: 16 bytes. */
typedef struct {
  int32_t start;   /* first kept sample of y */
  int32_t end;     /* one past the last kept sample */
  float   peak;    /* max |y| over [start, end) */
  int32_t status;  /* VQVAE_INGEST_* bits; 0 = good */
} vqvae_ingest_bounds;

/* Bytes of the per-frame workspace of vqvae_ingest_trim_bounds for U utterances of at most max_n samples:
 * U * (1 + max_n div 512) float64 frame energies, then as many float32 hop peaks.  0 for arguments trim_bounds rejects. */
size_t vqvae_ingest_workspace_bytes(int U, int max_n);

/* Decode to mono and resample U utterances of one (sr_in, channels, format) group.
 *   raw        interleaved frames, int16 or float32 by `format`
 *   in_offset  int64 (U,)  first frame of utterance u in `raw`, counted in frames
 *   n_in       int32 (U,)  its frames, >= 1
 *   max_n_in   the largest n_in (host); the grid covers max_n_out = ceil(max_n_in L / M) outputs, which the caller
 *              passes as well and the call checks against the formula
 *   taps       float32 (L, 2J), see above; read only when L != M
 *   y          float32; utterance u is written at y[y_offset[u] .. y_offset[u] + ceil(n_in[u] L / M))
 *   y_offset   int64 (U,)
 * L and M must be coprime.  One launch, grid (tiles, U).  The taps lie in LDS when they fit beside the tile's window
 * (80 KB together), else they are read from global memory; the results are the same bits.
 * Rejected: a null raw, in_offset, n_in, taps, y or y_offset; U < 1 or > 65535; channels outside 1..8; a format other
 * than the two; L, M or J < 1; L * 2J > VQVAE_INGEST_MAX_TAPS; a window above VQVAE_INGEST_MAX_WINDOW; max_n_in < 1;
 * max_n_out != ceil(max_n_in L / M) or above 2^31 - 1.  in_offset, n_in and y_offset are device data and are not
 * checked: an utterance longer than max_n_in is cut at max_n_out outputs. */
int vqvae_ingest_resample(const void* raw, int format, int channels, const int64_t* in_offset, const int32_t* n_in, int U,
                          int max_n_in, const float* taps, int L, int M, int J, float* y, const int64_t* y_offset,
                          int max_n_out, vqvae_stream_t stream);

/* The silence bounds, the peak and the status of U signals y[y_offset[u] .. + n[u]).
 *   n       int32 (U,)  samples of signal u, F / 2 + 1 = 1025 <= n[u] <= max_n (device data, not checked; a shorter
 *           signal is read inside its own extent and gives unspecified bounds)
 *   r       10 ** (-top_db / 10), in [0, 1)
 *   bounds  (U,) out
 * Two launches: one wavefront per frame writes E_t and max |y| of the frame's hop [512 t, 512 (t + 1)) into the
 * workspace, then one workgroup per utterance reads those: an E_t is non-finite iff a sample of its frame is, and
 * [start, end) is the union of the hops t_first .. t_last, so the result is the rule's.
 * Rejected: a null y, y_offset, n, workspace or bounds; U < 1 or > 65535; max_n < 1025; r not in [0, 1);
 * workspace_bytes below vqvae_ingest_workspace_bytes(U, max_n). */
int vqvae_ingest_trim_bounds(const float* y, const int64_t* y_offset, const int32_t* n, int U, int max_n, double r,
                             void* workspace, size_t workspace_bytes, vqvae_ingest_bounds* bounds, vqvae_stream_t stream);

/* dst[dst_offset[u] + i] = y[y_offset[u] + start + i] / peak for i in [0, end - start), for every utterance whose
 * status is 0; nothing is written for the others.  max_n: an upper bound of end - start (host; sizes the grid).
 * Rejected: a null y, y_offset, bounds, dst_offset or dst; U < 1 or > 65535; max_n < 1. */
int vqvae_ingest_pack(const float* y, const int64_t* y_offset, const vqvae_ingest_bounds* bounds, const int64_t* dst_offset,
                      int U, int max_n, float* dst, vqvae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif  /* VQVAE_INGEST_H_ */
