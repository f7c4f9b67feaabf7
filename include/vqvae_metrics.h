/*
 * vqvae_metrics.h -- objective audio metrics on the device (csrc/audio_metrics.hip, part of
 * libvqvae_hip.so): a short-time Fourier transform, log-mel features and three per-utterance distances
 * over a RAGGED list of waveforms.  It is the device side of vqvae_amd.metrics (features_many,
 * compare_many): the waves that synthesize_many returns are compared with their inputs where they lie.
 *
 * The entry points are additive and sit beside vqvae_hip.h and the other add-on headers (raw device
 * pointers, asynchronous on the given stream, 0 / hipError_t / VQVAE_E_INVALID return codes with
 * vqvae_last_error_string(), arguments validated before anything is launched, writes only inside the
 * outputs); the other ABIs, their versions and their kernels are not touched.  Forward only.  A program
 * that does not call them launches exactly what it launched before.
 *
 * Tables.  Three float32 arrays are INPUTS, built by the caller (vqvae_amd.metrics.tables builds them in
 * float64 and rounds once), the way the resampler's taps are inputs of vqvae_ingest_resample.  With
 * nb = n_fft / 2 + 1:
 *   dft  (2 * nb, n_fft)  row b:       w[k] * cos(2 pi b k / n_fft)
 *                         row nb + b: -w[k] * sin(2 pi b k / n_fft)      (w: the analysis window)
 *   mel  (n_mels, nb)     the mel filter bank
 *   dct  (n_mcep, n_mels) the cepstral transform
 * The kernels do not interpret them: any window, filter bank and transform of these shapes is taken.
 *
 * The rule (normative).  An utterance with L samples has F = 1 + (L - n_fft) / hop frames (integer
 * division; L >= n_fft).  Frame f reads samples [f * hop, f * hop + n_fft) of its OWN utterance and
 * nothing else: no centring, no padding, no reflection; samples behind the last frame belong to no
 * frame and are never loaded.  For frame f and bin b
 *   re  = sum_k dft[b, k]      * x[f * hop + k]
 *   im  = sum_k dft[nb + b, k] * x[f * hop + k]
 *   pw  = re * re + im * im
 *   mag = sqrtf(pw)
 *   mel[m]     = sum_b mel[m, b] * pw[b]            bins ascending, one multiply and one add per bin
 *   log_mel[m] = logf(max(mel[m], floor))
 * all in float32.  re and im are sums on v_mfma_f32_32x32x2_f32 (an fp32 fused multiply-add chain) in one
 * fixed order of k for every output element: blocks of 16 samples ascending and inside a block
 * k0 + j, k0 + 8 + j for j = 0 .. 7.
 *
 * Arithmetic.  fp32 operands, fp32 MFMA, fp32 accumulation in EVERY matmul mode: nothing here depends
 * on vqvae_set_matmul_dtype.  There is no per-tensor scale, no split-K, no floating-point atomic, and one
 * K order per output element: a frame's features are a pure function of its own n_fft samples and the
 * tables -- the same bits alone, in any list, at any position and in any chunking.
 *
 * Layout (that of vqvae_ragged.h).  The utterances of a call lie end to end along the FRAME axis:
 * utterance i owns frames [frame_off[i], frame_off[i + 1]), Ftot = frame_off[n].  log_mel is one
 * channel-major (n_mels, Ftot) float32 tensor, mag one (nb, Ftot) tensor (mel_pw as log_mel): element (r, f) at r * stride + f,
 * stride = Ftot for a call that owns its tensors.
 * The waves are read where they are: frame fl of utterance i starts at x[off_in[i] + fl * hop].
 *
 * Distances (vqvae_metrics_distances).  For pair i, `a` the reference and `b` the test, both framed over
 * the SAME frames (the caller cuts both waves to their common length first), with F_i frames,
 * la / lb the log-mels and ma / mb the magnitudes:
 *   out[i, 0] = log_mel_mae          = (1 / (F_i n_mels)) sum_{f, m} |la - lb|
 *   out[i, 1] = mcd_db               = (1 / F_i) sum_f C sqrt(2 sum_q (sum_m dct[q, m] * (0.5 * (la - lb)[m, f]))^2)
 *   out[i, 2] = spectral_convergence = sqrt(sum_{f, b} (ma - mb)^2) / sqrt(sum_{f, b} ma^2)
 * with C = 10 / ln 10 taken as the double 4.3429448190325175.  The 0.5 is there because la is a log
 * POWER.  Every difference is taken of the two float32 values converted to float64, which is exact;
 * everything after it is float64 without contraction in one fixed order: one workgroup of
 * VQVAE_METRICS_THREADS threads per pair; thread t adds elements t, t + 256, ... (element index
 * f_local * rows + row; for mcd_db the element is the frame, q and m ascending inside it) into one
 * accumulator per sum, starting from 0; the 256 partials are added in a binary tree (p[t] += p[t + h] for
 * h = 128, 64, ..., 1); the divisions and square roots above follow as written.  A silent reference
 * divides as IEEE divides: spectral_convergence is +inf when the test is not silent too, and NaN (0 / 0)
 * when it is.
 */
#ifndef VQVAE_METRICS_H_
#define VQVAE_METRICS_H_

#include "vqvae_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VQVAE_METRICS_TILE 32          /* frames of one workgroup of vqvae_metrics_stft_mel */
#define VQVAE_METRICS_THREADS 256      /* threads of a workgroup of either kernel */
#define VQVAE_METRICS_MAX_NFFT 2048
#define VQVAE_METRICS_MAX_MELS 128

/* 1; independent of the other versions */
int vqvae_metrics_abi_version(void);

typedef struct {
  int32_t n;            /* utterances, >= 1 */
  int32_t n_fft;        /* a multiple of 32 in [32, VQVAE_METRICS_MAX_NFFT] */
  int32_t hop;          /* 1 <= hop <= n_fft */
  int32_t n_mels;       /* 1 <= n_mels <= VQVAE_METRICS_MAX_MELS */
  int32_t n_mcep;       /* 1 <= n_mcep < n_mels (vqvae_metrics_distances only) */
  float floor;          /* > 0: the smallest mel power the log is taken of */
  int64_t ftot;         /* frames of all utterances, = frame_off[n], >= 1 */
  int64_t stride;       /* elements between the rows of log_mel and of mag, >= ftot: a chunk of a longer list
                           writes its columns of the whole list's tensors directly */
} vqvae_metrics_desc;

/* Bytes of workspace the two entry points need for this description: 0 today (a frame finds its
 * utterance by a search in frame_off, and the power spectrum of a tile stays in LDS), queried like every
 * other entry point's so that a later planning pass changes no caller.  (size_t)-1 for a description the
 * entry point would refuse. */
size_t vqvae_metrics_stft_mel_workspace_bytes(const vqvae_metrics_desc* d);
size_t vqvae_metrics_distances_workspace_bytes(const vqvae_metrics_desc* d);

/* STFT, mel sum and log of all utterances, ONE launch: the power spectrum never leaves the chip.
 *   x          float32, read at off_in[i] + p only for 0 <= p < n_fft + (F_i - 1) * hop
 *   off_in     int64 (n,)      first sample of every utterance (any order, gaps allowed: a corpus
 *                              buffer is read in place)
 *   frame_off  int64 (n + 1,)  first frame of every utterance, ascending from 0, every utterance at
 *                              least one frame; frame_off[n] = ftot
 *   dft, mel   the tables above; dft must be 16-byte aligned
 *   log_mel    float32 (n_mels, ftot), or NULL
 *   mag        float32 (nb, ftot), or NULL
 *   mel_pw     float32 (n_mels, ftot), or NULL: mel[m] itself, before the floor and the log -- at least one
 *              of the three
 *   ws         ws_bytes >= the query above (may be NULL when that is 0)
 * The tables are device data and are not checked: frame_off must be as described and the sample ranges
 * must lie inside x.  Rejected: a null descriptor, x, off_in, frame_off, dft or mel; all outputs null;
 * n or ftot < 1; n_fft not a multiple of 32 in [32, 2048]; hop outside [1, n_fft]; n_mels outside
 * [1, 128]; floor not > 0; a dft that is not 16-byte aligned; more than 2^31 - 1 frame tiles; a workspace
 * smaller than the query. */
int vqvae_metrics_stft_mel(const vqvae_metrics_desc* d, const float* x, const int64_t* off_in,
                           const int64_t* frame_off, const float* dft, const float* mel, float* log_mel,
                           float* mag, float* mel_pw, void* ws, size_t ws_bytes, vqvae_stream_t stream);

/* The three distances of every pair, ONE launch of n workgroups.
 *   log_mel_a, log_mel_b   float32 (n_mels, ftot)   reference, test
 *   mag_a, mag_b           float32 (nb, ftot)
 *   dct                    float32 (n_mcep, n_mels)
 *   frame_off              int64 (n + 1,), as above, the same for both sides
 *   out                    float64 (n, 3): log_mel_mae, mcd_db, spectral_convergence
 * Rejected: a null descriptor or pointer; the description errors above; n_mcep outside [1, n_mels); a
 * workspace smaller than the query. */
int vqvae_metrics_distances(const vqvae_metrics_desc* d, const float* log_mel_a, const float* log_mel_b,
                            const float* mag_a, const float* mag_b, const float* dct, const int64_t* frame_off,
                            double* out, void* ws, size_t ws_bytes, vqvae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif  /* VQVAE_METRICS_H_ */
