// From decoded audio to the waveforms of a device-resident corpus (include/vqvae_ingest.h): decode to mono + band-limited
// resampling, silence bounds + peak, normalise + pack.  The arithmetic of the rule is csrc/ingest_rule.h.
//
// Resample: grid (ceil(max_n_out / 1024), U), 256 threads.  A workgroup owns 1024 consecutive outputs of one utterance
// (thread k takes outputs k, k + 256, k + 512, k + 768 of them, so a wave stores 64 consecutive dwords).  It stages the
// tile's input window -- samples q(first output) - J + 1 .. q(last output) + J, decoded to mono float32, zero outside the
// utterance -- once in LDS, (TILE - 1) M / L + 2J + 1 floats at most (12.7 KB for 48 -> 16 kHz with kaiser_fast), and, when
// the table fits beside it (INGEST_LDS_BUDGET), the taps too, each phase's row padded to an odd stride: consecutive outputs
// use phases that differ by M mod L, so with an odd row stride the 32 lanes of an LDS access group read 32 different banks
// whenever M is odd, and all lanes read one address (a broadcast) when L == 1.  The window reads of consecutive lanes are
// M / L apart.  Larger tables (kaiser_best at 44.1 kHz: 221 KB) are read from global memory, through L2.  Either way an
// output is ingest_dot over 2J products in float64.
//
// Trim: a wavefront per frame sums the 2048 squares in the rule's lane order and folds the 64 lane sums with the rule's
// tree (__shfl_down), writing E_t and the peak of the frame's hop to the workspace; then a workgroup per utterance walks the
// frames only: a non-finite E_t (<=> a non-finite sample), max E_t, the first and last non-silent frame and the peak of the
// kept range as the maximum of its hops.  Maxima and minima do not depend on their order.
//
// Pack: grid (ceil(max_n / 1024), U): one correctly rounded division per sample.
//
// Every address is formed in 64 bits.  Plain vector stores, no atomics, no scratch.  Stores go to y[y_offset[u] + o] with
// o < n_out(u), to the workspace's energy[u * max_nf + t] and hop_peak[u * max_nf + t] with t < nf(u) <= max_nf, to
// bounds[u] and to dst[dst_offset[u] + i] with i < end - start.
#include "common.h"
#include "ingest_rule.h"
#include "../../include/vqvae_ingest.h"

#include <limits.h>

namespace vq {

constexpr int INGEST_THREADS = 256;
constexpr int INGEST_TILE = VQVAE_INGEST_TILE;
constexpr int INGEST_SPAN = 1024;                        // samples per workgroup of the copy and pack kernels
constexpr size_t INGEST_LDS_BUDGET = 80 * 1024;          // window + taps: two workgroups per CU
static_assert(INGEST_TILE % INGEST_THREADS == 0, "a thread takes TILE / THREADS outputs");
static_assert((size_t)VQVAE_INGEST_MAX_WINDOW * 4 <= 64 * 1024, "the window alone needs no LDS opt-in");

struct ResampleArgs {
  const void* raw;
  const int64_t* in_offset;
  const int32_t* n_in;
  const float* taps;
  float* y;
  const int64_t* y_offset;
  int fmt, channels, L, M, J, max_n_out;
  int win_cap;                                           // floats reserved for the window in front of the taps
  int row;                                               // the taps' row stride in LDS (odd)
};

__host__ __device__ __forceinline__ int ingest_window_cap(int L, int M, int J) {
  return (int)(((int64_t)(INGEST_TILE - 1) * M) / L) + 2 * J + 1;
}

template <bool TAPS_IN_LDS>
__global__ __launch_bounds__(INGEST_THREADS) void ingest_resample_kernel(ResampleArgs a) {
  extern __shared__ __attribute__((aligned(16))) float ingest_lds[];
  const int u = blockIdx.y;
  const int64_t n_in = a.n_in[u];
  int64_t n_out = ingest_n_out(n_in, a.L, a.M);
  if (n_out > a.max_n_out) n_out = a.max_n_out;
  const int64_t o0 = (int64_t)blockIdx.x * INGEST_TILE;
  if (o0 >= n_out) return;                               // the whole workgroup, before any barrier
  const int count = (int)(n_out - o0 < INGEST_TILE ? n_out - o0 : INGEST_TILE);
  const int64_t first = a.in_offset[u];
  const int64_t q0 = o0 * a.M / a.L, q1 = (o0 + count - 1) * a.M / a.L;
  const int taps2 = 2 * a.J;
  const int window = (int)(q1 - q0) + taps2;             // <= win_cap
  float* win = ingest_lds;
  float* htab = ingest_lds + a.win_cap;
  for (int i = threadIdx.x; i < window; i += INGEST_THREADS)
    win[i] = ingest_mono_at(a.raw, a.fmt, a.channels, first, q0 - a.J + 1 + i, n_in);
  if (TAPS_IN_LDS) {
    for (int i = threadIdx.x; i < a.L * taps2; i += INGEST_THREADS) htab[(i / taps2) * a.row + i % taps2] = a.taps[i];
  }
  __syncthreads();
  float* out = a.y + a.y_offset[u] + o0;
#pragma unroll
  for (int k = 0; k < INGEST_TILE / INGEST_THREADS; ++k) {
    const int oo = threadIdx.x + k * INGEST_THREADS;
    if (oo < count) {
      const int64_t om = (o0 + oo) * a.M;
      const int64_t q = om / a.L;
      const int p = (int)(om % a.L);
      const float* h = TAPS_IN_LDS ? htab + p * a.row : a.taps + (int64_t)p * taps2;
      out[oo] = ingest_dot(win + (int)(q - q0), h, taps2);
    }
  }
}

// sr_in == sr_out: the mono samples as they are
__global__ __launch_bounds__(INGEST_THREADS) void ingest_copy_kernel(ResampleArgs a) {
  const int u = blockIdx.y;
  const int64_t n_in = a.n_in[u];
  const int64_t n_out = n_in < a.max_n_out ? n_in : a.max_n_out;
  const int64_t first = a.in_offset[u];
  float* out = a.y + a.y_offset[u];
  const int64_t o0 = (int64_t)blockIdx.x * INGEST_SPAN + threadIdx.x;
#pragma unroll
  for (int k = 0; k < INGEST_SPAN / INGEST_THREADS; ++k) {
    const int64_t o = o0 + k * INGEST_THREADS;
    if (o < n_out) out[o] = ingest_mono_at(a.raw, a.fmt, a.channels, first, o, n_in);
  }
}

// one wavefront per frame: grid (ceil(max_nf / 4), U).  Beside E_t it leaves the peak of the frame's hop, so that the
// bounds kernel never walks the samples: a 10 s utterance is 160 000 samples and 313 frames.
__global__ __launch_bounds__(INGEST_THREADS) void ingest_frame_energy_kernel(const float* y_all, const int64_t* y_offset,
                                                                             const int32_t* n_of, int max_nf, double* energy,
                                                                             float* hop_peak) {
  const int u = blockIdx.y;
  const int n = n_of[u];
  const int nf = 1 + n / INGEST_HOP;
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * (INGEST_THREADS / 64) + (threadIdx.x >> 6);
  if (t >= nf || t >= max_nf) return;                    // a whole wavefront; no barrier in this kernel
  const float* y = y_all + y_offset[u];
  double a = ingest_lane_energy(y, n, t, lane);
  float peak = ingest_lane_hop_peak(y, n, t, lane);
#pragma unroll
  for (int stride = 32; stride >= 1; stride >>= 1) {
    a += __shfl_down(a, stride);                         // lanes < stride hold the rule's a_l
    const float other = __shfl_down(peak, stride);
    peak = other > peak ? other : peak;
  }
  if (lane == 0) {
    energy[(int64_t)u * max_nf + t] = a;
    hop_peak[(int64_t)u * max_nf + t] = peak;
  }
}

// block-wide maximum / minimum through LDS; every thread returns the result
template <typename T, bool MAX>
__device__ __forceinline__ T ingest_block_extreme(T v, T* buf) {
  __syncthreads();                                       // buf may still be read from the previous use
  buf[threadIdx.x] = v;
  __syncthreads();
  for (int s = INGEST_THREADS / 2; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s) {
      const T o = buf[threadIdx.x + s], m = buf[threadIdx.x];
      buf[threadIdx.x] = MAX ? (o > m ? o : m) : (o < m ? o : m);
    }
    __syncthreads();
  }
  return buf[0];
}

// one workgroup per utterance, over its frames only
__global__ __launch_bounds__(INGEST_THREADS) void ingest_bounds_kernel(const int32_t* n_of, int max_nf, const double* energy,
                                                                       const float* hop_peak, double r,
                                                                       vqvae_ingest_bounds* bounds) {
  __shared__ double dbuf[INGEST_THREADS];
  __shared__ int ibuf[INGEST_THREADS];
  const int u = blockIdx.x;
  const int n = n_of[u];
  int nf = 1 + n / INGEST_HOP;
  if (nf > max_nf) nf = max_nf;
  const double* E = energy + (int64_t)u * max_nf;
  const float* P = hop_peak + (int64_t)u * max_nf;
  int bad = 0;
  double top = INGEST_AMIN;                              // ref = max(amin, max_t mse_t) = max_t max(amin, mse_t)
  for (int t = threadIdx.x; t < nf; t += INGEST_THREADS) {
    const double e = E[t];
    bad |= !ingest_finite_energy(e);
    const double m = ingest_floor_mse(e);
    top = m > top ? m : top;
  }
  if (__syncthreads_or(bad)) {
    if (threadIdx.x == 0) {
      vqvae_ingest_bounds b;
      b.start = 0; b.end = n; b.peak = 0.0f; b.status = INGEST_BAD_SAMPLE;
      bounds[u] = b;
    }
    return;
  }
  const double thr = ingest_block_extreme<double, true>(top, dbuf) * r;
  int t_first = INT_MAX, t_last = -1;
  for (int t = threadIdx.x; t < nf; t += INGEST_THREADS)
    if (ingest_floor_mse(E[t]) > thr) {
      t_first = t < t_first ? t : t_first;
      t_last = t;
    }
  t_first = ingest_block_extreme<int, false>(t_first, ibuf);
  t_last = ingest_block_extreme<int, true>(t_last, ibuf);
  int start = 0, end = 0;                                // no non-silent frame (r == 1 is rejected, so not reached): empty
  float peak = 0.0f;
  if (t_last >= 0) {
    start = INGEST_HOP * t_first;
    const int64_t e = (int64_t)INGEST_HOP * (t_last + 1);
    end = (int)(e < n ? e : n);
    for (int t = t_first + (int)threadIdx.x; t <= t_last; t += INGEST_THREADS) peak = P[t] > peak ? P[t] : peak;
  }
  peak = (float)ingest_block_extreme<double, true>((double)peak, dbuf);
  if (threadIdx.x == 0) {
    vqvae_ingest_bounds b;
    b.start = start; b.end = end; b.peak = peak;
    b.status = (end <= start ? INGEST_EMPTY : 0) | (peak == 0.0f ? INGEST_ZERO_PEAK : 0);
    bounds[u] = b;
  }
}

__global__ __launch_bounds__(INGEST_THREADS) void ingest_pack_kernel(const float* y, const int64_t* y_offset,
                                                                     const vqvae_ingest_bounds* bounds, const int64_t* dst_offset,
                                                                     float* dst) {
  const int u = blockIdx.y;
  const vqvae_ingest_bounds b = bounds[u];
  if (b.status != 0) return;
  const int len = b.end - b.start;
  const float* src = y + y_offset[u] + b.start;
  float* out = dst + dst_offset[u];
  const int i0 = blockIdx.x * INGEST_SPAN + threadIdx.x;
#pragma unroll
  for (int k = 0; k < INGEST_SPAN / INGEST_THREADS; ++k) {
    const int i = i0 + k * INGEST_THREADS;
    if (i < len) out[i] = ingest_normalise(src[i], b.peak);
  }
}

static inline int ingest_max_frames(int max_n) { return 1 + max_n / INGEST_HOP; }

}  // namespace vq

using namespace vq;

extern "C" int vqvae_ingest_abi_version(void) { return 1; }

extern "C" size_t vqvae_ingest_workspace_bytes(int U, int max_n) {
  if (U < 1 || U > 65535 || max_n < INGEST_MIN_N) return 0;
  return (size_t)U * (size_t)ingest_max_frames(max_n) * (sizeof(double) + sizeof(float));
}

extern "C" int vqvae_ingest_resample(const void* raw, int format, int channels, const int64_t* in_offset, const int32_t* n_in,
                                     int U, int max_n_in, const float* taps, int L, int M, int J, float* y,
                                     const int64_t* y_offset, int max_n_out, vqvae_stream_t stream) {
  VQ_REQUIRE(raw && in_offset && n_in && taps && y && y_offset, "ingest_resample: null raw, in_offset, n_in, taps, y or y_offset");
  VQ_REQUIRE(U >= 1 && U <= 65535, "ingest_resample: 1..65535 utterances per call (got %d)", U);
  VQ_REQUIRE(channels >= 1 && channels <= 8, "ingest_resample: channels must be 1..8 (got %d)", channels);
  VQ_REQUIRE(format == VQVAE_INGEST_I16 || format == VQVAE_INGEST_F32, "ingest_resample: format must be 0 (int16) or 1 (float32) (got %d)",
             format);
  VQ_REQUIRE(L >= 1 && M >= 1 && J >= 1, "ingest_resample: L, M and J must be at least 1 (got %d, %d, %d)", L, M, J);
  VQ_REQUIRE((long long)L * 2 * (long long)J <= (long long)VQVAE_INGEST_MAX_TAPS,
             "ingest_resample: the tap table has %lld entries, the limit is %d", (long long)L * 2 * (long long)J, VQVAE_INGEST_MAX_TAPS);
  VQ_REQUIRE((long long)(INGEST_TILE - 1) * M / L + 2ll * J + 1 <= (long long)VQVAE_INGEST_MAX_WINDOW,
             "ingest_resample: a tile's window of %lld samples is above the limit of %d",
             (long long)(INGEST_TILE - 1) * M / L + 2ll * J + 1, VQVAE_INGEST_MAX_WINDOW);
  VQ_REQUIRE(max_n_in >= 1, "ingest_resample: n_in must be at least 1 (got max_n_in %d)", max_n_in);
  const int64_t want = ingest_n_out(max_n_in, L, M);
  VQ_REQUIRE(want <= INT_MAX && (int64_t)max_n_out == want, "ingest_resample: max_n_out is %d, ceil(%d * %d / %d) is %lld (at most 2^31 - 1)",
             max_n_out, max_n_in, L, M, (long long)want);
  ResampleArgs a{};
  a.raw = raw; a.in_offset = in_offset; a.n_in = n_in; a.taps = taps; a.y = y; a.y_offset = y_offset;
  a.fmt = format; a.channels = channels; a.L = L; a.M = M; a.J = J; a.max_n_out = max_n_out;
  if (L == M) {
    const dim3 grid((unsigned)cdiv(max_n_out, INGEST_SPAN), (unsigned)U);
    hipLaunchKernelGGL(ingest_copy_kernel, grid, dim3(INGEST_THREADS), 0, (hipStream_t)stream, a);
    VQ_LAUNCH_CHECK();
    return 0;
  }
  a.win_cap = (int)align_up((size_t)ingest_window_cap(L, M, J), 4);
  a.row = (2 * J) | 1;
  const size_t win_bytes = (size_t)a.win_cap * sizeof(float);
  const size_t both = win_bytes + (size_t)L * (size_t)a.row * sizeof(float);
  const dim3 grid((unsigned)cdiv(max_n_out, INGEST_TILE), (unsigned)U);
  if (both <= INGEST_LDS_BUDGET) {
    const int rc = lds_opt_in<ingest_resample_kernel<true>>(both);
    if (rc) return rc;
    hipLaunchKernelGGL(ingest_resample_kernel<true>, grid, dim3(INGEST_THREADS), both, (hipStream_t)stream, a);
  } else {
    hipLaunchKernelGGL(ingest_resample_kernel<false>, grid, dim3(INGEST_THREADS), win_bytes, (hipStream_t)stream, a);
  }
  VQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int vqvae_ingest_trim_bounds(const float* y, const int64_t* y_offset, const int32_t* n, int U, int max_n, double r,
                                        void* workspace, size_t workspace_bytes, vqvae_ingest_bounds* bounds,
                                        vqvae_stream_t stream) {
  VQ_REQUIRE(y && y_offset && n && workspace && bounds, "ingest_trim_bounds: null y, y_offset, n, workspace or bounds");
  VQ_REQUIRE(U >= 1 && U <= 65535, "ingest_trim_bounds: 1..65535 utterances per call (got %d)", U);
  VQ_REQUIRE(max_n >= INGEST_MIN_N, "ingest_trim_bounds: a signal needs at least %d samples (got max_n %d)", INGEST_MIN_N, max_n);
  VQ_REQUIRE(r >= 0.0 && r < 1.0, "ingest_trim_bounds: r = 10 ** (-top_db / 10) must be in [0, 1) (got %g)", r);
  const size_t need = vqvae_ingest_workspace_bytes(U, max_n);
  VQ_REQUIRE(workspace_bytes >= need, "ingest_trim_bounds: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  const int max_nf = ingest_max_frames(max_n);
  const dim3 grid((unsigned)cdiv(max_nf, INGEST_THREADS / 64), (unsigned)U);
  double* energy = (double*)workspace;                   // U * max_nf float64, then as many float32 hop peaks
  float* hop_peak = (float*)(energy + (size_t)U * (size_t)max_nf);
  hipLaunchKernelGGL(ingest_frame_energy_kernel, grid, dim3(INGEST_THREADS), 0, (hipStream_t)stream, y, y_offset, n, max_nf, energy,
                     hop_peak);
  VQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(ingest_bounds_kernel, dim3((unsigned)U), dim3(INGEST_THREADS), 0, (hipStream_t)stream, n, max_nf,
                     (const double*)energy, (const float*)hop_peak, r, bounds);
  VQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int vqvae_ingest_pack(const float* y, const int64_t* y_offset, const vqvae_ingest_bounds* bounds, const int64_t* dst_offset,
                                 int U, int max_n, float* dst, vqvae_stream_t stream) {
  VQ_REQUIRE(y && y_offset && bounds && dst_offset && dst, "ingest_pack: null y, y_offset, bounds, dst_offset or dst");
  VQ_REQUIRE(U >= 1 && U <= 65535, "ingest_pack: 1..65535 utterances per call (got %d)", U);
  VQ_REQUIRE(max_n >= 1, "ingest_pack: max_n must be at least 1 (got %d)", max_n);
  const dim3 grid((unsigned)cdiv(max_n, INGEST_SPAN), (unsigned)U);
  hipLaunchKernelGGL(ingest_pack_kernel, grid, dim3(INGEST_THREADS), 0, (hipStream_t)stream, y, y_offset, bounds, dst_offset, dst);
  VQ_LAUNCH_CHECK();
  return 0;
}
