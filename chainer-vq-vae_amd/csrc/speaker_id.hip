// Per-speaker Gaussians over mel-cepstra for a ragged list of utterances (csrc/speaker_id.h states the rule).
//
// spk_features_kernel: a tile of 256 frames per workgroup, a thread per frame.  The tile's first and last utterance come
//   from ragged_find_segment; with the gate on, the workgroup first finds the largest frame energy of every utterance
//   that owns a frame of the tile (a strided scan of that utterance's log-mel and a max fold in LDS: a maximum has no
//   order, so every tile of an utterance finds the same bits).  A thread then sums its frame's cepstra and, for the
//   deltas, those of the two neighbours inside its utterance, sharing the dct value of a term between the three sums.
// spk_stats_kernel: ONE workgroup per utterance.  The D + D (D + 1) / 2 accumulators are walked in tiles of
//   VQVAE_SPK_ACC_TILE: a lane carries the tile's partial sums over its frames in registers, the 256 lanes' partials are
//   folded in LDS (16 KB), eight accumulators side by side.  The order is per accumulator, so the tiling is not seen.
// spk_score_kernel<DMAX>: grid (utterance, tile of VQVAE_SPK_MODEL_TILE models).  The tile's mu and packed linv sit in LDS
//   and are read at wave-uniform addresses (broadcasts); a lane owns a frame, keeps x[f] in registers and walks the
//   tile's models: z = x - mu in registers, the triangle fully unrolled (DMAX of 16, 32 or 48, the rows at and above D
//   left out by a uniform branch), so every operand index is a constant.  A lane's running sum per model lives in LDS in
//   a slot of its own; the slots are folded at the end.
//   Dynamic LDS: MODEL_TILE * 8 * (D + D (D + 1) / 2 + 256) bytes: 40512 at D = 26, 94720 at D = 48, asked for through
//   lds_opt_in above 64 KB.
//
// An utterance whose table entries contradict the descriptor is skipped and marked (the header).  Every address is formed
// in 64 bits; plain vector stores only.
#include "common.h"
#include "ragged_seg.h"
#include "speaker_id.h"

namespace vq {

constexpr int SP_LANES = VQVAE_SPK_LANES;
constexpr int SP_ACC = VQVAE_SPK_ACC_TILE;
constexpr int SP_TILE = VQVAE_SPK_MODEL_TILE;
constexpr size_t SP_LDS_CAP = 160 * 1024;            // the LDS of a CU, which one workgroup may take
constexpr size_t SP_STATIC_LDS = SP_LANES * sizeof(long long);
static_assert((SP_LANES & (SP_LANES - 1)) == 0, "the fold halves the lanes");

__host__ __device__ constexpr size_t sp_score_lds(int D) {
  return sizeof(double) * (size_t)SP_TILE * ((size_t)D + (size_t)D * (D + 1) / 2 + SP_LANES);
}
static_assert(sp_score_lds(VQVAE_SPK_MAX_DIM) + SP_STATIC_LDS <= SP_LDS_CAP, "a tile of the widest models must fit a CU's LDS");

__device__ __forceinline__ double sp_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

struct SpSeg {
  long long lo, hi;
  bool ok;
};

// utterance i of the table, and whether it agrees with the descriptor
__device__ __forceinline__ SpSeg sp_segment(const int64_t* off, int n, long long ftot, int i) {
  SpSeg s;
  s.lo = (long long)off[i];
  s.hi = (long long)off[i + 1];
  s.ok = (long long)off[0] == 0 && (long long)off[n] == ftot && s.lo >= 0 && s.hi > s.lo && s.hi <= ftot;
  return s;
}

struct SpFeatArgs {
  const float* log_mel; const float* dct; const int64_t* off; double* x; unsigned char* keep;
  long long ftot, stride;
  double thr;
  int n, n_mels, n_mcep, deltas, dim, use_gate;
};

__global__ __launch_bounds__(SP_LANES) void spk_features_kernel(SpFeatArgs a) {
  __shared__ double s_fold[SP_LANES];
  __shared__ double s_emax[SP_LANES];                       // of utterance u0 + k
  const int tid = threadIdx.x;
  const long long f0 = (long long)blockIdx.x * SP_LANES;
  const long long f = f0 + tid;
  const long long f_last = f0 + SP_LANES - 1 < a.ftot - 1 ? f0 + SP_LANES - 1 : a.ftot - 1;
  const int M = a.n_mels;
  const int u0 = ragged_find_segment(a.off, a.n, f0);
  int u1 = ragged_find_segment(a.off, a.n, f_last);
  if (u1 > u0 + SP_LANES - 1) u1 = u0 + SP_LANES - 1;       // an ascending table gives a tile at most 256 utterances
  if (a.use_gate) {                                         // uniform for the workgroup
    for (int u = u0; u <= u1; ++u) {
      const SpSeg s = sp_segment(a.off, a.n, a.ftot, u);
      double mx = sp_nan();                                 // NaN compares false: nothing of a skipped utterance is kept
      if (s.ok) {
        bool any = false;
        for (long long g = s.lo + tid; g < s.hi; g += SP_LANES) {
          double e = 0.0;
          for (int m = 0; m < M; ++m) e += (double)a.log_mel[(long long)m * a.stride + g];
          mx = (!any || e > mx) ? e : mx;
          any = true;
        }
        s_fold[tid] = any ? mx : -__builtin_huge_val();
        __syncthreads();
        for (int h = SP_LANES / 2; h >= 1; h >>= 1) {
          if (tid < h) s_fold[tid] = s_fold[tid + h] > s_fold[tid] ? s_fold[tid + h] : s_fold[tid];
          __syncthreads();
        }
        mx = s_fold[0];
        __syncthreads();
      }
      if (tid == 0) s_emax[u - u0] = mx;
    }
    __syncthreads();
  }
  if (f >= a.ftot) return;
  const int D = a.dim, Q = a.n_mcep;
  double* x = a.x + f * D;
  const int u = ragged_find_segment(a.off, a.n, f);
  const SpSeg s = sp_segment(a.off, a.n, a.ftot, u);
  if (!s.ok || f < s.lo || f >= s.hi || u < u0 || u > u1) {
    for (int p = 0; p < D; ++p) x[p] = sp_nan();
    a.keep[f] = 0;
    return;
  }
  const float* lm = a.log_mel + f;
  const long long back = f > s.lo ? -1 : 0, fwd = f + 1 < s.hi ? 1 : 0;
  for (int q = 0; q < Q; ++q) {
    const float* w = a.dct + q * M;
    double c = 0.0, cb = 0.0, cf = 0.0;
    if (a.deltas) {
      for (int m = 0; m < M; ++m) {
        const double wm = (double)w[m];
        const float* row = lm + (long long)m * a.stride;
        c += wm * (double)row[0];
        cb += wm * (double)row[back];
        cf += wm * (double)row[fwd];
      }
      x[Q + q] = 0.5 * (cf - cb);
    } else {
      for (int m = 0; m < M; ++m) c += (double)w[m] * (double)lm[(long long)m * a.stride];
    }
    x[q] = c;
  }
  unsigned char k = 1;
  if (a.use_gate) {
    double e = 0.0;
    for (int m = 0; m < M; ++m) e += (double)lm[(long long)m * a.stride];
    k = e >= s_emax[u - u0] - a.thr ? 1 : 0;
  }
  a.keep[f] = k;
}

// the kept frames of an utterance, counted by the whole workgroup; every thread gets the total
__device__ __forceinline__ long long sp_count(long long* s_c, long long mine) {
  const int tid = threadIdx.x;
  s_c[tid] = mine;
  __syncthreads();
  for (int h = SP_LANES / 2; h >= 1; h >>= 1) {
    if (tid < h) s_c[tid] += s_c[tid + h];
    __syncthreads();
  }
  return s_c[0];
}

struct SpStatArgs {
  const double* x; const unsigned char* keep; const int64_t* off; double* s1; double* s2; int64_t* cnt;
  long long ftot;
  int n, dim;
};

__global__ __launch_bounds__(SP_LANES) void spk_stats_kernel(SpStatArgs a) {
  __shared__ double s_p[SP_ACC][SP_LANES];
  __shared__ long long s_c[SP_LANES];
  const int tid = threadIdx.x;
  const int i = blockIdx.x;
  const int D = a.dim;
  const long long T = (long long)D * (D + 1) / 2;
  double* s1 = a.s1 + (long long)i * D;
  double* s2 = a.s2 + (long long)i * T;
  const SpSeg s = sp_segment(a.off, a.n, a.ftot, i);
  if (!s.ok) {                                              // uniform for the workgroup
    for (long long e = tid; e < D; e += SP_LANES) s1[e] = sp_nan();
    for (long long e = tid; e < T; e += SP_LANES) s2[e] = sp_nan();
    if (tid == 0) a.cnt[i] = 0;
    return;
  }
  long long kept = 0;
  for (long long f = s.lo + tid; f < s.hi; f += SP_LANES) kept += a.keep[f] ? 1 : 0;
  kept = sp_count(s_c, kept);
  if (tid == 0) a.cnt[i] = kept;
  // row -1 is s1, row p >= 0 the products x[p] * x[q], q = p .. D - 1; a tile is SP_ACC consecutive q of a row
  for (int p = -1; p < D; ++p) {
    for (int q0 = p < 0 ? 0 : p; q0 < D; q0 += SP_ACC) {
      double acc[SP_ACC];
#pragma unroll
      for (int j = 0; j < SP_ACC; ++j) acc[j] = 0.0;
      for (long long f = s.lo + tid; f < s.hi; f += SP_LANES) {
        if (!a.keep[f]) continue;
        const double* xf = a.x + f * D;
        if (p < 0) {
#pragma unroll
          for (int j = 0; j < SP_ACC; ++j)
            if (q0 + j < D) acc[j] += xf[q0 + j];
        } else {
          const double xp = xf[p];
#pragma unroll
          for (int j = 0; j < SP_ACC; ++j)
            if (q0 + j < D) acc[j] += xp * xf[q0 + j];
        }
      }
#pragma unroll
      for (int j = 0; j < SP_ACC; ++j) s_p[j][tid] = acc[j];
      __syncthreads();
      for (int h = SP_LANES / 2; h >= 1; h >>= 1) {
        if (tid < h) {
#pragma unroll
          for (int j = 0; j < SP_ACC; ++j) s_p[j][tid] += s_p[j][tid + h];
        }
        __syncthreads();
      }
      if (tid < SP_ACC && q0 + tid < D) {
        if (p < 0) s1[q0 + tid] = s_p[tid][0];
        else s2[(long long)p * D - (long long)p * (p - 1) / 2 + (q0 + tid - p)] = s_p[tid][0];
      }
      __syncthreads();
    }
  }
}

struct SpScoreArgs {
  const double* x; const unsigned char* keep; const int64_t* off; const double* mu; const double* linv; double* q; int64_t* cnt;
  long long ftot;
  int n, dim, n_models;
};

template <int DMAX>
__global__ __launch_bounds__(SP_LANES, 2) void spk_score_kernel(SpScoreArgs a) {
  extern __shared__ __attribute__((aligned(16))) double sp_lds[];
  __shared__ long long s_c[SP_LANES];
  const int tid = threadIdx.x;
  const int i = blockIdx.x;
  const int g0 = blockIdx.y * SP_TILE;
  const int G = a.n_models, D = a.dim;
  const int T = D * (D + 1) / 2, per = D + T;
  const int ng = G - g0 < SP_TILE ? G - g0 : SP_TILE;
  double* s_model = sp_lds;                                 // [ng][D + T]: mu, then the packed triangle
  double* s_part = sp_lds + (size_t)SP_TILE * per;          // [ng][SP_LANES]
  double* q = a.q + (long long)i * G + g0;
  const SpSeg s = sp_segment(a.off, a.n, a.ftot, i);
  if (!s.ok) {                                              // uniform for the workgroup
    if (tid < ng) q[tid] = sp_nan();
    if (tid == 0 && blockIdx.y == 0) a.cnt[i] = 0;
    return;
  }
  for (int e = tid; e < ng * per; e += SP_LANES) {
    const int g = e / per, k = e - g * per;
    s_model[e] = k < D ? a.mu[(long long)(g0 + g) * D + k] : a.linv[(long long)(g0 + g) * T + (k - D)];
  }
  for (int g = 0; g < ng; ++g) s_part[g * SP_LANES + tid] = 0.0;
  __syncthreads();
  long long kept = 0;
  for (long long f = s.lo + tid; f < s.hi; f += SP_LANES) {
    if (!a.keep[f]) continue;
    ++kept;
    const double* xf = a.x + f * D;
    double x[DMAX];
#pragma unroll
    for (int c = 0; c < DMAX; ++c) x[c] = c < D ? xf[c] : 0.0;
    for (int g = 0; g < ng; ++g) {
      const double* m = s_model + g * per;
      const double* L = m + D;
      double z[DMAX];
#pragma unroll
      for (int c = 0; c < DMAX; ++c) z[c] = c < D ? x[c] - m[c] : 0.0;
      double qf = 0.0;
#pragma unroll
      for (int r = 0; r < DMAX; ++r) {
        if (r < D) {                                        // uniform
          double y = 0.0;
#pragma unroll
          for (int c = 0; c <= r; ++c) y += L[r * (r + 1) / 2 + c] * z[c];
          qf += y * y;
        }
      }
      s_part[g * SP_LANES + tid] += qf;
    }
  }
  kept = sp_count(s_c, kept);                               // its barriers also close the lanes' slots
  for (int h = SP_LANES / 2; h >= 1; h >>= 1) {
    if (tid < h)
      for (int g = 0; g < ng; ++g) s_part[g * SP_LANES + tid] += s_part[g * SP_LANES + tid + h];
    __syncthreads();
  }
  if (tid < ng) q[tid] = s_part[tid * SP_LANES] / (double)kept;
  if (tid == 0 && blockIdx.y == 0) a.cnt[i] = kept;
}

template <int DMAX>
static int sp_launch_score(const SpScoreArgs& a, hipStream_t stream) {
  const size_t lds = sp_score_lds(a.dim);
  if (int e = lds_opt_in<spk_score_kernel<DMAX>>(lds)) return e;
  const dim3 grid((unsigned)a.n, (unsigned)((a.n_models + SP_TILE - 1) / SP_TILE));
  hipLaunchKernelGGL((spk_score_kernel<DMAX>), grid, dim3(SP_LANES), lds, stream, a);
  VQ_LAUNCH_CHECK();
  return 0;
}

}  // namespace vq

using namespace vq;

extern "C" int vqvae_spk_revision(void) { return 1; }

#define SP_REQUIRE_DESC(who, d)                                                                                            \
  VQ_REQUIRE(d, who ": null descriptor");                                                                                  \
  VQ_REQUIRE(d->n >= 1, who ": n must be at least 1 (got %d)", (int)d->n);                                                 \
  VQ_REQUIRE(d->n_mels >= 1 && d->n_mels <= VQVAE_SPK_MAX_MELS, who ": n_mels must be in [1, %d] (got %d)",                \
             VQVAE_SPK_MAX_MELS, (int)d->n_mels);                                                                          \
  VQ_REQUIRE(d->n_mcep >= 1 && d->n_mcep < d->n_mels, who ": n_mcep must be in [1, n_mels) (got %d of %d)",                \
             (int)d->n_mcep, (int)d->n_mels);                                                                              \
  VQ_REQUIRE(d->deltas == 0 || d->deltas == 1, who ": deltas must be 0 or 1 (got %d)", (int)d->deltas);                    \
  VQ_REQUIRE(d->dim == d->n_mcep * (1 + d->deltas), who ": dim must be n_mcep * (1 + deltas) = %d (got %d)",               \
             (int)(d->n_mcep * (1 + d->deltas)), (int)d->dim);                                                             \
  VQ_REQUIRE(d->dim <= VQVAE_SPK_MAX_DIM, who ": dim must be at most %d (got %d)", VQVAE_SPK_MAX_DIM, (int)d->dim);        \
  VQ_REQUIRE(d->n_models >= 0 && d->n_models <= VQVAE_SPK_MAX_MODELS, who ": n_models must be in [0, %d] (got %d)",        \
             VQVAE_SPK_MAX_MODELS, (int)d->n_models);                                                                      \
  VQ_REQUIRE(d->use_gate == 0 || d->use_gate == 1, who ": use_gate must be 0 or 1 (got %d)", (int)d->use_gate);            \
  VQ_REQUIRE(d->reserved == 0, who ": reserved must be 0 (got %d)", (int)d->reserved);                                     \
  VQ_REQUIRE(d->ftot >= d->n, who ": ftot must be at least n (got %lld of %d)", (long long)d->ftot, (int)d->n);            \
  VQ_REQUIRE(d->stride >= d->ftot, who ": stride must be at least ftot (got %lld of %lld)", (long long)d->stride,          \
             (long long)d->ftot);                                                                                          \
  VQ_REQUIRE(!d->use_gate || (d->thr >= 0.0 && d->thr <= 1.7976931348623157e308),                                          \
             who ": thr must be finite and not negative with the gate on (got %g)", d->thr)

extern "C" int vqvae_spk_features(const vqvae_spk_desc* d, const float* log_mel, const float* dct, const int64_t* frame_off,
                                  double* x, unsigned char* keep, vqvae_stream_t stream) {
  SP_REQUIRE_DESC("spk_features", d);
  VQ_REQUIRE(log_mel && dct && frame_off && x && keep, "spk_features: null log_mel, dct, frame_off, x or keep");
  SpFeatArgs a{};
  a.log_mel = log_mel; a.dct = dct; a.off = frame_off; a.x = x; a.keep = keep;
  a.ftot = d->ftot; a.stride = d->stride; a.thr = d->thr;
  a.n = d->n; a.n_mels = d->n_mels; a.n_mcep = d->n_mcep; a.deltas = d->deltas; a.dim = d->dim; a.use_gate = d->use_gate;
  const long long blocks = (a.ftot + SP_LANES - 1) / SP_LANES;
  VQ_REQUIRE(blocks <= 0x7fffffffLL, "spk_features: %lld frames are more than 2^31 - 1 workgroups", a.ftot);
  hipLaunchKernelGGL(spk_features_kernel, dim3((unsigned)blocks), dim3(SP_LANES), 0, (hipStream_t)stream, a);
  VQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int vqvae_spk_stats(const vqvae_spk_desc* d, const double* x, const unsigned char* keep, const int64_t* frame_off,
                               double* s1, double* s2, int64_t* cnt, vqvae_stream_t stream) {
  SP_REQUIRE_DESC("spk_stats", d);
  VQ_REQUIRE(x && keep && frame_off && s1 && s2 && cnt, "spk_stats: null x, keep, frame_off, s1, s2 or cnt");
  SpStatArgs a{};
  a.x = x; a.keep = keep; a.off = frame_off; a.s1 = s1; a.s2 = s2; a.cnt = cnt;
  a.ftot = d->ftot; a.n = d->n; a.dim = d->dim;
  hipLaunchKernelGGL(spk_stats_kernel, dim3((unsigned)d->n), dim3(SP_LANES), 0, (hipStream_t)stream, a);
  VQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int vqvae_spk_score(const vqvae_spk_desc* d, const double* x, const unsigned char* keep, const int64_t* frame_off,
                               const double* mu, const double* linv, double* q, int64_t* cnt, vqvae_stream_t stream) {
  SP_REQUIRE_DESC("spk_score", d);
  VQ_REQUIRE(d->n_models >= 1, "spk_score: n_models must be at least 1 (got %d)", (int)d->n_models);
  VQ_REQUIRE(x && keep && frame_off && mu && linv && q && cnt, "spk_score: null x, keep, frame_off, mu, linv, q or cnt");
  SpScoreArgs a{};
  a.x = x; a.keep = keep; a.off = frame_off; a.mu = mu; a.linv = linv; a.q = q; a.cnt = cnt;
  a.ftot = d->ftot; a.n = d->n; a.dim = d->dim; a.n_models = d->n_models;
  if (a.dim <= 16) return sp_launch_score<16>(a, (hipStream_t)stream);
  if (a.dim <= 32) return sp_launch_score<32>(a, (hipStream_t)stream);
  return sp_launch_score<48>(a, (hipStream_t)stream);
}
