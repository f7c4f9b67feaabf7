// The ingest rule of include/vqvae_ingest.h: decode to mono, the resampler's output sample, the reflected frame index and the
// frame energy's lane sums, the silence bounds, the normalising division.  Plain C++ with one float64 accumulator per
// sum and a fixed order, the same on the host and on the device, so a stand-alone host program can compile these very
// functions (tests/test_host_ingest.py).  No transcendental: the taps and r come from Python.
#ifndef VQ_INGEST_RULE_H_
#define VQ_INGEST_RULE_H_
#include <stdint.h>

namespace vq {

constexpr int INGEST_FMT_I16 = 0, INGEST_FMT_F32 = 1;   // VQVAE_INGEST_I16 / VQVAE_INGEST_F32
constexpr int INGEST_FRAME = 2048;                      // F
constexpr int INGEST_HOP = 512;                         // H
constexpr int INGEST_MIN_N = INGEST_FRAME / 2 + 1;      // one reflection suffices from here on
constexpr double INGEST_AMIN = 1e-10;
constexpr int INGEST_BAD_SAMPLE = 1, INGEST_ZERO_PEAK = 2, INGEST_EMPTY = 4;   // the status bits

// n_out = ceil(n_in * L / M)
__host__ __device__ __forceinline__ int64_t ingest_n_out(int64_t n_in, int L, int M) {
  return (n_in * (int64_t)L + (int64_t)M - 1) / (int64_t)M;
}

// mono sample `frame` of an utterance whose first frame is `first` of the interleaved buffer; 0 outside [0, n_in)
__host__ __device__ __forceinline__ float ingest_mono_at(const void* raw, int fmt, int channels, int64_t first, int64_t frame,
                                                         int64_t n_in) {
  if (frame < 0 || frame >= n_in) return 0.0f;
  const int64_t at = (first + frame) * (int64_t)channels;
  double sum = 0.0;
  if (fmt == INGEST_FMT_I16) {
    const int16_t* p = (const int16_t*)raw + at;
    for (int c = 0; c < channels; ++c) sum += (double)p[c] / 32768.0;
  } else {
    const float* p = (const float*)raw + at;
    for (int c = 0; c < channels; ++c) sum += (double)p[c];
  }
  return (float)(sum / (double)channels);
}

// sum over j ascending of x[j] * h[j], n products, one float64 accumulator; x: the window from sample q - J + 1 on,
// h: row p of the tap table.  Every product is exact in float64, so a fused multiply-add gives the same bits.
__host__ __device__ __forceinline__ float ingest_dot(const float* x, const float* h, int n) {
  double acc = 0.0;
  for (int j = 0; j < n; ++j) acc += (double)x[j] * (double)h[j];
  return (float)acc;
}

// output o straight from the raw buffer (the kernel stages the same window in LDS and calls ingest_dot on it)
__host__ __device__ __forceinline__ float ingest_output_at(const void* raw, int fmt, int channels, int64_t first, int64_t n_in,
                                                           const float* taps, int L, int M, int J, int64_t o) {
  if (L == M) return ingest_mono_at(raw, fmt, channels, first, o, n_in);
  const int64_t q = o * (int64_t)M / (int64_t)L;
  const int p = (int)(o * (int64_t)M % (int64_t)L);
  const float* h = taps + (int64_t)p * (int64_t)(2 * J);
  double acc = 0.0;
  for (int j = 0; j < 2 * J; ++j)
    acc += (double)ingest_mono_at(raw, fmt, channels, first, q - (int64_t)J + 1 + (int64_t)j, n_in) * (double)h[j];
  return (float)acc;
}

// sample m of frame t of a signal of n >= INGEST_MIN_N samples: i = t H + m - F / 2, reflected once.  The clamp changes
// nothing from INGEST_MIN_N on; below it, it keeps the index inside the signal.
__host__ __device__ __forceinline__ int ingest_frame_index(int t, int m, int n) {
  int64_t i = (int64_t)t * INGEST_HOP + m - INGEST_FRAME / 2;
  if (i < 0) i = -i;
  if (i >= n) i = 2 * ((int64_t)n - 1) - i;
  if (i < 0) i = 0;
  if (i >= n) i = (int64_t)n - 1;
  return (int)i;
}

// a_l of frame t: the squares of samples l, l + 64, ..., l + 64 * 31 of the frame, summed in that order
__host__ __device__ __forceinline__ double ingest_lane_energy(const float* y, int n, int t, int lane) {
  double a = 0.0;
  for (int r = 0; r < INGEST_FRAME / 64; ++r) {
    const double v = (double)y[ingest_frame_index(t, lane + 64 * r, n)];
    a += v * v;
  }
  return a;
}

// lane's share of max |y| over hop t, samples [t H, (t + 1) H) inside the signal: the peak of [start, end) is the maximum
// of the hops t_first .. t_last, because start = H t_first and end = min(n, H (t_last + 1))
__host__ __device__ __forceinline__ float ingest_lane_hop_peak(const float* y, int n, int t, int lane) {
  float peak = 0.0f;
  for (int k = 0; k < INGEST_HOP / 64; ++k) {
    const int64_t i = (int64_t)t * INGEST_HOP + lane + 64 * k;
    if (i < n) {
      const float v = y[i] < 0.0f ? -y[i] : y[i];
      peak = v > peak ? v : peak;
    }
  }
  return peak;
}

// a frame energy is finite iff every sample of the frame is: squares of finite float32 values and sums of 2048 of them
// stay far below the float64 range.  The frames cover the signal, so one non-finite E_t <=> one non-finite sample.
__host__ __device__ __forceinline__ bool ingest_finite_energy(double e) {
  union { double d; uint64_t u; } b;
  b.d = e;
  return (b.u & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// max(amin, E / F): the quantity the threshold is taken from and compared with
__host__ __device__ __forceinline__ double ingest_floor_mse(double energy) {
  const double mse = energy / (double)INGEST_FRAME;
  return mse > INGEST_AMIN ? mse : INGEST_AMIN;
}

__host__ __device__ __forceinline__ bool ingest_finite(float v) {
  union { float f; uint32_t u; } b;
  b.f = v;
  return (b.u & 0x7f800000u) != 0x7f800000u;
}

__host__ __device__ __forceinline__ float ingest_normalise(float v, float peak) { return v / peak; }

}  // namespace vq
#endif  // VQ_INGEST_RULE_H_
