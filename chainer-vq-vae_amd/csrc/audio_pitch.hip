// Pitch and voicing over a ragged list of waveforms (include/vqvae_pitch.h): the per-frame YIN estimator in one launch per
// chunk, and the eight per-pair statistics in one more.  Everything is float64 vector arithmetic in the fixed orders of the
// header, compiled without contraction (-ffp-contract=off, the Makefile's setting for the whole library, restated below).
//
// pitch_yin_kernel: a workgroup of four waves owns a tile of up to 4 frames (plain frames of the ragged frame axis: a tile
//   may span utterances; a thread per frame finds the frame's utterance by a search in the frame_off prefix table).  Every
//   frame is staged on its own, so nothing a frame computes depends on its neighbours in the tile.
//   1. the frame's samples go to LDS as float32 (converted at every use: exact).
//   2. a lane owns one (frame, lag) and walks j with the header's four accumulators; x[j] is a broadcast read, x[j + tau]
//      consecutive across the lanes.  The items of a tile are laid end to end (frame-major), so only the tile's last wave
//      is partly filled.  The power (the same sum without the lagged term) is formed by the first lanes of the LAST wave,
//      which has the fewest lag items.
//   3. lane 0 of wave w adds c(tau) of frame w sequentially (eight loads in flight at a time).
//   4. all threads form d'(tau) = d * tau / c in place.
//   5. wave w picks for frame w: the first lag under the threshold and the minimum by a wave reduction of exact minima
//      (order-free), then lane 0 walks down to the local minimum, refines and stores.
//   LDS (dynamic): 64 + tile * (16 (tau_max + 1) + 4 frame) bytes, 33 KB at the default configuration; tile is 4 unless
//   that passes the 160 KB of a CU (never, today: frame 2048 with tau_max 2046 takes 163 840 bytes exactly).
// pitch_compare_kernel: one workgroup of 256 threads per pair, thread-strided frames, binary tree; no atomics.
//
// Every address is formed in 64 bits.  Stores: f0[f] and aperiodicity[f] for f < ftot; out[8 i + 0 .. 7]; plain vector stores.
#include <cmath>

#include "common.h"
#include "ragged_seg.h"
#include "../../include/vqvae_pitch.h"

#pragma clang fp contract(off)

namespace vq {

constexpr int PT_THREADS = VQVAE_PITCH_THREADS;
constexpr int PT_MAX_TILE = VQVAE_PITCH_MAX_TILE;
constexpr size_t PT_LDS_CAP = 160 * 1024;          // the LDS of a CU, which one workgroup may take
constexpr size_t PT_LDS_FIXED = PT_MAX_TILE * (sizeof(long long) + sizeof(double));

struct YinArgs {
  const float* x; const int64_t* off_in; const int64_t* frame_off; float* f0; float* ap;
  long long ftot;
  double sr, threshold, min_power;
  int n, frame, hop, tau_min, tau_max, tile;
};

static size_t pt_lds_frame(int frame, int tau_max) { return 2 * sizeof(double) * ((size_t)tau_max + 1) + sizeof(float) * (size_t)frame; }

// the header's order S over the W terms (a[j] - b[j])^2, or a[j]^2 for the power
template <bool POWER>
__device__ __forceinline__ double pt_sum(const float* a, const float* b, const int W) {
  auto term = [&](const int j) {
    const double t = POWER ? (double)a[j] : (double)a[j] - (double)b[j];
    return t * t;
  };
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int j = 0;
  for (; j + 4 <= W; j += 4) {
    a0 += term(j); a1 += term(j + 1); a2 += term(j + 2); a3 += term(j + 3);
  }
  if (j < W) a0 += term(j);
  if (j + 1 < W) a1 += term(j + 1);
  if (j + 2 < W) a2 += term(j + 2);
  return (a0 + a1) + (a2 + a3);
}

__global__ __launch_bounds__(PT_THREADS) void pitch_yin_kernel(YinArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pt_lds[];
  const int nl = a.tau_max + 1;                                  // d and c are indexed by tau; slot 0 is not used
  long long* s_g = reinterpret_cast<long long*>(pt_lds);         // [4] first sample of the frame in x
  double* s_pw = reinterpret_cast<double*>(s_g + PT_MAX_TILE);   // [4] the power sum
  double* s_d = s_pw + PT_MAX_TILE;                              // [tile][nl] d, then d'
  double* s_c = s_d + (size_t)a.tile * nl;                       // [tile][nl] c
  float* s_x = reinterpret_cast<float*>(s_c + (size_t)a.tile * nl);     // [tile][frame]

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const long long f0 = (long long)blockIdx.x * a.tile;
  const long long left = a.ftot - f0;
  const int nv = left < a.tile ? (int)left : a.tile;             // frames of this tile, >= 1
  const int W = a.frame - a.tau_max;
  if (tid < nv) {
    const long long f = f0 + tid;
    const int i = ragged_find_segment(a.frame_off, a.n, f);      // the utterance of frame f
    s_g[tid] = (long long)a.off_in[i] + (f - (long long)a.frame_off[i]) * a.hop;
  }
  __syncthreads();
  for (int fl = 0; fl < nv; ++fl) {
    const float* src = a.x + s_g[fl];
    for (int k = tid; k < a.frame; k += PT_THREADS) s_x[fl * a.frame + k] = src[k];
  }
  __syncthreads();

  for (int e = tid; e < nv * a.tau_max; e += PT_THREADS) {       // d(tau), tau = 1 .. tau_max, of every frame
    const int fl = e / a.tau_max, tau = 1 + (e - fl * a.tau_max);
    const float* xs = s_x + fl * a.frame;
    s_d[fl * nl + tau] = pt_sum<false>(xs, xs + tau, W);
  }
  if (wave == PT_THREADS / 64 - 1 && lane < nv) s_pw[lane] = pt_sum<true>(s_x + lane * a.frame, nullptr, W);
  __syncthreads();

  if (lane == 0 && wave < nv) {                                  // c(tau) = d(1) + ... + d(tau), sequentially
    const double* d = s_d + wave * nl;
    double* c = s_c + wave * nl;
    double run = 0.0;
    int tau = 1;
    for (; tau + 8 <= nl; tau += 8) {
      double v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = d[tau + q];
#pragma unroll
      for (int q = 0; q < 8; ++q) { run += v[q]; c[tau + q] = run; }
    }
    for (; tau < nl; ++tau) { run += d[tau]; c[tau] = run; }
  }
  __syncthreads();

  for (int e = tid; e < nv * a.tau_max; e += PT_THREADS) {       // d'(tau) in place of d(tau)
    const int fl = e / a.tau_max, tau = 1 + (e - fl * a.tau_max);
    const double d = s_d[fl * nl + tau], c = s_c[fl * nl + tau];
    s_d[fl * nl + tau] = c == 0.0 ? 1.0 : (d * (double)tau) / c;
  }
  __syncthreads();

  if (wave >= nv) return;                                        // no barrier below
  const double* dp = s_d + wave * nl;
  constexpr int NONE = 0x7fffffff;
  int first = NONE;
  double mn = __builtin_huge_val();
  for (int tau = a.tau_min + lane; tau <= a.tau_max; tau += 64) {
    const double v = dp[tau];
    if (v < a.threshold && tau < first) first = tau;
    if (v < mn) mn = v;
  }
  for (int m = 32; m >= 1; m >>= 1) {
    const int of = __shfl_xor(first, m);
    const double om = __shfl_xor(mn, m);
    first = of < first ? of : first;
    mn = om < mn ? om : mn;
  }
  if (lane != 0) return;
  float f0v = 0.f, apv;
  if (s_pw[wave] / (double)W < a.min_power) {
    apv = 1.f;
  } else if (first == NONE) {
    apv = (float)mn;
  } else {
    int tau = first;
    while (tau + 1 <= a.tau_max && dp[tau + 1] < dp[tau]) ++tau;
    double ts = (double)tau;
    if (tau - 1 >= 1 && tau + 1 <= a.tau_max) {
      const double pa = dp[tau - 1], pb = dp[tau], pc = dp[tau + 1];
      const double q = (pa - 2.0 * pb) + pc;
      if (q > 0.0) ts = (double)tau + (0.5 * (pa - pc)) / q;
    }
    f0v = (float)(a.sr / ts);
    apv = (float)dp[tau];
  }
  if (a.f0) a.f0[f0 + wave] = f0v;
  if (a.ap) a.ap[f0 + wave] = apv;
}

struct CmpArgs { const float* fa; const float* fb; const int64_t* frame_off; double* out; };

__global__ __launch_bounds__(PT_THREADS) void pitch_compare_kernel(CmpArgs a) {
  __shared__ double s_s[3][PT_THREADS];
  __shared__ unsigned s_n[5][PT_THREADS];
  const int t = threadIdx.x;
  const long long i = blockIdx.x;
  const long long fo = (long long)a.frame_off[i];
  const long long F = (long long)a.frame_off[i + 1] - fo;
  double sq = 0.0, la = 0.0, lb = 0.0;
  unsigned na = 0, nb = 0, nboth = 0, ndiff = 0, ngross = 0;
  for (long long f = t; f < F; f += PT_THREADS) {
    const double fa = (double)a.fa[fo + f], fb = (double)a.fb[fo + f];
    const bool va = fa > 0.0, vb = fb > 0.0;
    if (va) { ++na; la += log(fa); }
    if (vb) { ++nb; lb += log(fb); }
    if (va != vb) ++ndiff;
    if (va && vb) {
      ++nboth;
      const double r = fb / fa;
      if (fabs(r - 1.0) > 0.2) ++ngross;
      const double c = 1200.0 * log2(r);
      sq += c * c;
    }
  }
  s_s[0][t] = sq; s_s[1][t] = la; s_s[2][t] = lb;
  s_n[0][t] = na; s_n[1][t] = nb; s_n[2][t] = nboth; s_n[3][t] = ndiff; s_n[4][t] = ngross;
  __syncthreads();
  for (int h = PT_THREADS / 2; h >= 1; h >>= 1) {
    if (t < h) {
#pragma unroll
      for (int q = 0; q < 3; ++q) s_s[q][t] += s_s[q][t + h];
#pragma unroll
      for (int q = 0; q < 5; ++q) s_n[q][t] += s_n[q][t + h];
    }
    __syncthreads();
  }
  if (t == 0) {
    double* o = a.out + VQVAE_PITCH_COLUMNS * i;
    const double ca = (double)s_n[0][0], cb = (double)s_n[1][0], cboth = (double)s_n[2][0];
    o[0] = ca; o[1] = cb; o[2] = cboth;
    o[3] = (double)s_n[3][0] / (double)F;
    o[4] = (double)s_n[4][0] / cboth;
    o[5] = sqrt(s_s[0][0] / cboth);
    o[6] = s_s[1][0] / ca;
    o[7] = s_s[2][0] / cb;
  }
}

// tau_min = floor(sr / fmax) and tau_max = ceil(sr / fmin), checked as doubles before they become ints
struct PitchLags { bool ok; int tau_min, tau_max; };
static PitchLags pitch_lags(const vqvae_pitch_desc* d) {
  PitchLags r{false, 0, 0};
  if (d->sr < 1 || !(d->fmin > 0.0) || !(d->fmax > 0.0) || !std::isfinite(d->fmin) || !std::isfinite(d->fmax)) return r;
  const double lo = std::floor((double)d->sr / d->fmax), hi = std::ceil((double)d->sr / d->fmin);
  if (!(lo >= 2.0 && lo < hi && hi <= (double)d->frame - 2.0)) return r;
  return PitchLags{true, (int)lo, (int)hi};
}

static bool pitch_counts_ok(const vqvae_pitch_desc* d) { return d && d->n >= 1 && d->ftot >= 1; }
static bool pitch_desc_ok(const vqvae_pitch_desc* d) {
  return pitch_counts_ok(d) && d->frame >= 1 && d->frame <= VQVAE_PITCH_MAX_FRAME && d->hop >= 1 && d->hop <= d->frame &&
         d->threshold > 0.0 && d->threshold < 1.0 && d->min_power >= 0.0 && std::isfinite(d->min_power) && pitch_lags(d).ok;
}

// the one workspace plan of each entry point: nothing is taken today
struct PitchPlan { size_t total; };
static PitchPlan plan_yin(const vqvae_pitch_desc*) { WsPlan p; return PitchPlan{p.total}; }
static PitchPlan plan_compare(const vqvae_pitch_desc*) { WsPlan p; return PitchPlan{p.total}; }

}  // namespace vq

using namespace vq;

extern "C" int vqvae_pitch_abi_version(void) { return 1; }

extern "C" size_t vqvae_pitch_yin_workspace_bytes(const vqvae_pitch_desc* d) {
  if (!pitch_desc_ok(d)) return (size_t)-1;
  return plan_yin(d).total;
}

extern "C" size_t vqvae_pitch_compare_workspace_bytes(const vqvae_pitch_desc* d) {
  if (!pitch_counts_ok(d)) return (size_t)-1;
  return plan_compare(d).total;
}

#define PT_REQUIRE_COUNTS(who, d)                                                                                          \
  VQ_REQUIRE(d, who ": null descriptor");                                                                                  \
  VQ_REQUIRE(d->n >= 1, who ": n must be at least 1 (got %d)", (int)d->n);                                                 \
  VQ_REQUIRE(d->ftot >= 1, who ": ftot must be at least 1 (got %lld)", (long long)d->ftot)

extern "C" int vqvae_pitch_yin(const vqvae_pitch_desc* d, const float* x, const int64_t* off_in, const int64_t* frame_off,
                               float* f0, float* aperiodicity, void* ws, size_t ws_bytes, vqvae_stream_t stream) {
  PT_REQUIRE_COUNTS("pitch_yin", d);
  VQ_REQUIRE(d->sr >= 1, "pitch_yin: sr must be at least 1 (got %d)", (int)d->sr);
  VQ_REQUIRE(d->frame >= 1 && d->frame <= VQVAE_PITCH_MAX_FRAME, "pitch_yin: frame must be in [1, %d] (got %d)",
             VQVAE_PITCH_MAX_FRAME, (int)d->frame);
  VQ_REQUIRE(d->hop >= 1 && d->hop <= d->frame, "pitch_yin: hop must be in [1, frame] (got %d)", (int)d->hop);
  VQ_REQUIRE(d->threshold > 0.0 && d->threshold < 1.0, "pitch_yin: threshold must be in (0, 1) (got %g)", d->threshold);
  VQ_REQUIRE(d->min_power >= 0.0 && std::isfinite(d->min_power), "pitch_yin: min_power must be finite and not negative (got %g)",
             d->min_power);
  const PitchLags lags = pitch_lags(d);
  VQ_REQUIRE(lags.ok, "pitch_yin: 2 <= tau_min = floor(sr / fmax) < tau_max = ceil(sr / fmin) <= frame - 2 needed "
             "(sr %d, frame %d, fmin %g, fmax %g)", (int)d->sr, (int)d->frame, d->fmin, d->fmax);
  VQ_REQUIRE(x && off_in && frame_off, "pitch_yin: null x, off_in or frame_off");
  VQ_REQUIRE(f0 || aperiodicity, "pitch_yin: f0 and aperiodicity are both null");
  const size_t per = pt_lds_frame(d->frame, lags.tau_max);
  const size_t fit = (PT_LDS_CAP - PT_LDS_FIXED) / per;          // >= 4 for every accepted configuration
  const int tile = fit < (size_t)PT_MAX_TILE ? (int)fit : PT_MAX_TILE;
  VQ_REQUIRE(tile >= 1, "pitch_yin: a frame of %d samples with tau_max %d does not fit the LDS", (int)d->frame, lags.tau_max);
  const long long tiles = (d->ftot + tile - 1) / tile;
  VQ_REQUIRE(tiles <= 0x7fffffffLL, "pitch_yin: %lld frames are more than 2^31 - 1 frame tiles", (long long)d->ftot);
  const PitchPlan plan = plan_yin(d);
  VQ_REQUIRE(ws_bytes >= plan.total && (ws || !plan.total), "pitch_yin: workspace of %zu bytes, %zu needed", ws_bytes, plan.total);
  YinArgs a{};
  a.x = x; a.off_in = off_in; a.frame_off = frame_off; a.f0 = f0; a.ap = aperiodicity;
  a.ftot = d->ftot; a.sr = (double)d->sr; a.threshold = d->threshold; a.min_power = d->min_power;
  a.n = d->n; a.frame = d->frame; a.hop = d->hop; a.tau_min = lags.tau_min; a.tau_max = lags.tau_max; a.tile = tile;
  const size_t lds = PT_LDS_FIXED + (size_t)tile * per;
  if (int e = lds_opt_in<pitch_yin_kernel>(lds)) return e;
  hipLaunchKernelGGL(pitch_yin_kernel, dim3((unsigned)tiles), dim3(PT_THREADS), lds, (hipStream_t)stream, a);
  VQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int vqvae_pitch_compare(const vqvae_pitch_desc* d, const float* f0_a, const float* f0_b, const int64_t* frame_off,
                                   double* out, void* ws, size_t ws_bytes, vqvae_stream_t stream) {
  PT_REQUIRE_COUNTS("pitch_compare", d);
  VQ_REQUIRE(f0_a && f0_b && frame_off && out, "pitch_compare: null f0_a, f0_b, frame_off or out");
  const PitchPlan plan = plan_compare(d);
  VQ_REQUIRE(ws_bytes >= plan.total && (ws || !plan.total), "pitch_compare: workspace of %zu bytes, %zu needed", ws_bytes, plan.total);
  CmpArgs a{f0_a, f0_b, frame_off, out};
  hipLaunchKernelGGL(pitch_compare_kernel, dim3((unsigned)d->n), dim3(PT_THREADS), 0, (hipStream_t)stream, a);
  VQ_LAUNCH_CHECK();
  return 0;
}
