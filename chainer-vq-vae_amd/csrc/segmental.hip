// Duration-penalised quantisation of a ragged list of utterances (csrc/segmental.h states the rule).
//
// seg_dist_kernel: the table D (ttot, k) float64, a tile of 64 frames x 64 codes per workgroup of 256.  Per step of 32
//   channels the z tile [32][64] and the W tile, transposed to [32][64 + 4], are staged in LDS as float32; a lane owns
//   4 frames x 4 consecutive codes (16 float64 accumulators) and walks j ascending in every cell: per channel four
//   broadcast reads of z, one 16-byte read of W, 16 subtractions, 16 products, 16 additions.  A cell's sum is its own, so
//   the tiling is not seen in the bits.  Static LDS: 8192 + 8704 bytes.
// seg_dp_kernel<CPL, WAVES>: grid (utterance, penalty).  Register r of lane l of wave w holds V of code
//   64 (w + WAVES r) + l, so the wave's ballot over register r IS stay-word w + WAVES r of the frame.  WAVES = 1
//   (k <= VQVAE_SEG_WAVE_K, CPL = 1, 2, 4, 8): one wavefront runs the whole utterance and never meets a barrier.
//   WAVES = 4 (CPL = 4, 8, 16, 32): every wave folds its own minimum and its lowest index, lane 0 leaves both in a
//   double-buffered LDS slot, ONE barrier per frame, and every lane folds the four slots.  The next frame's row of D is
//   loaded before the current frame is reduced.  The minimum is folded by value alone (exact in any order); its lowest
//   index is then the first set bit of the first non-empty ballot of V == m, registers ascending.
//   The backtrack runs at the tail of the same launch, on wave 0: while the code stays, the 64 lanes read the stay-words
//   of the current code for 64 earlier frames at once, a ballot finds the first switch, the lanes fill the codes down to
//   it and the walk jumps there: one dependent load per 64 frames of a run plus one per switch (a[t - 1]).
//
// An utterance whose table entries contradict the descriptor is skipped and marked (the header).  Every address is formed
// in 64 bits; plain vector stores only; no floating-point atomics.
#include "common.h"
#include "segmental.h"

namespace vq {

constexpr int SG_TILE = VQVAE_SEG_TILE;
constexpr int SG_JT = 32;                            // channels staged at a time
constexpr int SG_WPAD = SG_TILE + 4;                 // the transposed W tile's row: 16-byte aligned, off the z tile's banks
constexpr int SG_LANES = VQVAE_SEG_LANES;
constexpr size_t SG_LDS_CAP = 160 * 1024;
constexpr size_t SG_DIST_LDS = sizeof(float) * SG_JT * (SG_TILE + SG_WPAD);
static_assert(SG_TILE == 64 && SG_LANES == 256, "a lane owns 4 x 4 cells of a 64 x 64 tile");
static_assert(SG_DIST_LDS <= SG_LDS_CAP, "the distance tiles must fit a CU's LDS");
static_assert(VQVAE_SEG_WAVE_K == 64 * 8 && VQVAE_SEG_MAX_K == SG_LANES * 32, "the DP kernels' register blocks");

__device__ __forceinline__ double sg_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

struct SgDistArgs {
  const float* z; const float* W; double* D;
  long long ttot, stride;
  int d, k;
};

__global__ __launch_bounds__(SG_LANES) void seg_dist_kernel(SgDistArgs a) {
  __shared__ __attribute__((aligned(16))) float s_z[SG_JT][SG_TILE];
  __shared__ __attribute__((aligned(16))) float s_w[SG_JT][SG_WPAD];
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;                   // codes c0 + 4 tx + q, frames t0 + ty + 16 i
  const long long t0 = (long long)blockIdx.x * SG_TILE;
  const int c0 = (int)blockIdx.y * SG_TILE;
  double acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[i][q] = 0.0;
  for (int j0 = 0; j0 < a.d; j0 += SG_JT) {
    const int jn = a.d - j0 < SG_JT ? a.d - j0 : SG_JT;
    for (int e = tid; e < SG_JT * SG_TILE; e += SG_LANES) {
      const int j = e >> 6, t = e & 63;
      float v = 0.0f;
      if (j < jn && t0 + t < a.ttot) v = a.z[(long long)(j0 + j) * a.stride + t0 + t];
      s_z[j][t] = v;
    }
    for (int e = tid; e < SG_TILE * SG_JT; e += SG_LANES) {
      const int c = e >> 5, j = e & 31;
      float v = 0.0f;
      if (j < jn && c0 + c < a.k) v = a.W[(long long)(c0 + c) * a.d + j0 + j];
      s_w[j][c] = v;
    }
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < jn; ++j) {
      const float4 w4 = *reinterpret_cast<const float4*>(&s_w[j][4 * tx]);
      const double w[4] = {(double)w4.x, (double)w4.y, (double)w4.z, (double)w4.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const double zz = (double)s_z[j][ty + 16 * i];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const double df = zz - w[q];
          acc[i][q] += df * df;
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long long t = t0 + ty + 16 * i;
    if (t >= a.ttot) continue;
    double* row = a.D + t * a.k;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = c0 + 4 * tx + q;
      if (c < a.k) row[c] = acc[i][q];
    }
  }
}

struct SgDpArgs {
  const double* D; const int64_t* off; unsigned long long* stay; int32_t* am; int32_t* codes; int32_t* n_seg; double* cost;
  long long ttot, code_stride, utt_stride;
  int n, k, nw;
  double lam[VQVAE_SEG_MAX_PEN];
};

// the smallest V of the workgroup's codes and its lowest index; every lane gets both.  ``buf``: the LDS slot of this call
template <int CPL, int WAVES>
__device__ __forceinline__ void sg_min(const double (&V)[CPL], int k, int lane, int wave, int buf, double (*s_v)[WAVES],
                                       int (*s_i)[WAVES], double& m_out, int& arg_out) {
  double m = V[0];
#pragma unroll
  for (int r = 1; r < CPL; ++r) m = V[r] < m ? V[r] : m;
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const double o = __shfl_xor(m, s);
    m = o < m ? o : m;
  }
  int arg = 0x7fffffff;
#pragma unroll
  for (int r = 0; r < CPL; ++r) {
    const int base = 64 * (wave + WAVES * r);
    const unsigned long long hit = __ballot(V[r] == m && base + lane < k);
    if (arg == 0x7fffffff && hit) arg = base + __builtin_ctzll(hit);
  }
  if (WAVES > 1) {
    if (lane == 0) { s_v[buf][wave] = m; s_i[buf][wave] = arg; }
    __syncthreads();
    m = s_v[buf][0];
    arg = s_i[buf][0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) {
      const double v = s_v[buf][w];
      const int iw = s_i[buf][w];
      if (v < m || (v == m && iw < arg)) { m = v; arg = iw; }
    }
  }
  m_out = m;
  arg_out = arg < k ? arg : 0;                              // nothing compared equal (not finite): index 0
}

template <int CPL, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void seg_dp_kernel(SgDpArgs a) {
  __shared__ double s_v[2][WAVES];
  __shared__ int s_i[2][WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int u = blockIdx.x, p = blockIdx.y;
  const int k = a.k, nw = a.nw;
  const long long lo = (long long)a.off[u], hi = (long long)a.off[u + 1];
  const bool ok = (long long)a.off[0] == 0 && (long long)a.off[a.n] == a.ttot && lo >= 0 && hi > lo && hi <= a.ttot;
  int32_t* codes = a.codes + (long long)p * a.code_stride;
  if (!ok) {                                                // uniform for the workgroup
    const long long b0 = lo > 0 ? lo : 0, b1 = hi < a.ttot ? hi : a.ttot;
    for (long long t = b0 + tid; t < b1; t += 64 * WAVES) codes[t] = -1;
    if (tid == 0) {
      a.n_seg[(long long)p * a.utt_stride + u] = 0;
      a.cost[(long long)p * a.utt_stride + u] = sg_nan();
    }
    return;
  }
  const long long T = hi - lo;
  double lam = a.lam[0];
#pragma unroll
  for (int q = 1; q < VQVAE_SEG_MAX_PEN; ++q) lam = p == q ? a.lam[q] : lam;
  const double* D = a.D + lo * k;
  unsigned long long* stay = a.stay + ((long long)p * a.ttot + lo) * nw;
  int32_t* am = a.am + (long long)p * a.ttot + lo;
  codes += lo;
  const double inf = __builtin_huge_val();                  // a code at or above k: never the minimum, never balloted

  double V[CPL], Dn[CPL];
#pragma unroll
  for (int r = 0; r < CPL; ++r) {
    const int c = 64 * (wave + WAVES * r) + lane;
    V[r] = c < k ? D[c] : inf;
  }
  double m;
  int arg;
  for (long long t = 1; t < T; ++t) {
    const double* row = D + t * k;
#pragma unroll
    for (int r = 0; r < CPL; ++r) {
      const int c = 64 * (wave + WAVES * r) + lane;
      Dn[r] = c < k ? row[c] : inf;
    }
    sg_min<CPL, WAVES>(V, k, lane, wave, (int)(t & 1), s_v, s_i, m, arg);
    const double sw = m + lam;
    if (tid == 0) am[t - 1] = arg;
    unsigned long long* words = stay + t * nw;
#pragma unroll
    for (int r = 0; r < CPL; ++r) {
      const int word = wave + WAVES * r;
      const bool b = V[r] <= sw;
      const unsigned long long bits = __ballot(b && 64 * word + lane < k);
      if (lane == 0 && word < nw) words[word] = bits;
      V[r] = Dn[r] + (b ? V[r] : sw);
    }
  }
  sg_min<CPL, WAVES>(V, k, lane, wave, (int)(T & 1), s_v, s_i, m, arg);

  __threadfence();                                          // the stay-words and a, written by other lanes and waves
  if (WAVES > 1) __syncthreads();
  if (wave != 0) return;
  int c = arg, n_seg = 1;
  long long t = T - 1;
  if (lane == 0) codes[t] = c;
  while (t >= 1) {
    const long long tt = t - lane;                          // lane l looks at frame t - l
    bool leaves = false;
    if (tt >= 1) leaves = !((stay[tt * nw + (c >> 6)] >> (c & 63)) & 1ULL);
    const unsigned long long mask = __ballot(leaves);
    const int f = mask ? __builtin_ctzll(mask) : (int)(t < 64 ? t : 64);      // frames t, t - 1, ... that stay
    if (lane < f) codes[t - 1 - lane] = c;
    t -= f;
    if (mask) {                                             // frame t switches: c[t - 1] = a[t - 1]
      const int cn = __builtin_amdgcn_readfirstlane(am[t - 1]);
      if (lane == 0) codes[t - 1] = cn;
      n_seg += cn != c ? 1 : 0;
      c = cn;
      t -= 1;
    }
  }
  if (lane == 0) {
    a.n_seg[(long long)p * a.utt_stride + u] = n_seg;
    a.cost[(long long)p * a.utt_stride + u] = m;
  }
}

template <int CPL, int WAVES>
static int sg_launch_dp(const SgDpArgs& a, int n_pen, hipStream_t stream) {
  hipLaunchKernelGGL((seg_dp_kernel<CPL, WAVES>), dim3((unsigned)a.n, (unsigned)n_pen), dim3(64 * WAVES), 0, stream, a);
  VQ_LAUNCH_CHECK();
  return 0;
}

struct SgPlan {
  size_t table, stay, am, total;
};

// the table (ttot, k) float64, the stay-words (n_pen, ttot, ceil(k / 64)) uint64, a (n_pen, ttot) int32
static SgPlan sg_plan(const vqvae_seg_desc* d) {
  WsPlan w;
  SgPlan p;
  const size_t ttot = (size_t)d->ttot, nw = ((size_t)d->k + 63) / 64;
  p.table = w.take(ttot * (size_t)d->k * sizeof(double));
  p.stay = w.take((size_t)d->n_pen * ttot * nw * sizeof(unsigned long long));
  p.am = w.take((size_t)d->n_pen * ttot * sizeof(int32_t));
  p.total = w.total;
  return p;
}

static int sg_launch_dist(const vqvae_seg_desc* d, const float* z, const float* W, double* table, hipStream_t stream) {
  SgDistArgs a{};
  a.z = z; a.W = W; a.D = table;
  a.ttot = d->ttot; a.stride = d->stride; a.d = d->d; a.k = d->k;
  const long long tiles = (a.ttot + SG_TILE - 1) / SG_TILE;
  VQ_REQUIRE(tiles <= 0x7fffffffLL, "seg_distances: %lld frames are more than 2^31 - 1 tiles", a.ttot);
  hipLaunchKernelGGL(seg_dist_kernel, dim3((unsigned)tiles, (unsigned)((a.k + SG_TILE - 1) / SG_TILE)), dim3(SG_LANES), 0,
                     stream, a);
  VQ_LAUNCH_CHECK();
  return 0;
}

static bool sg_finite_penalties(const vqvae_seg_desc* d) {
  if (d->n_pen < 1 || d->n_pen > VQVAE_SEG_MAX_PEN) return true;      // refused under its own name
  for (int q = 0; q < d->n_pen; ++q)
    if (!(d->lam[q] >= 0.0 && d->lam[q] <= 1.7976931348623157e308)) return false;
  return true;
}

}  // namespace vq

using namespace vq;

extern "C" int vqvae_seg_revision(void) { return 1; }

#define SG_REQUIRE_DESC(who, d)                                                                                            \
  VQ_REQUIRE(d, who ": null descriptor");                                                                                  \
  VQ_REQUIRE(d->n >= 1, who ": n must be at least 1 (got %d)", (int)d->n);                                                 \
  VQ_REQUIRE(d->d >= 1, who ": d must be at least 1 (got %d)", (int)d->d);                                                 \
  VQ_REQUIRE(d->k >= 1 && d->k <= VQVAE_SEG_MAX_K, who ": k must be in [1, %d] (got %d)", VQVAE_SEG_MAX_K, (int)d->k);     \
  VQ_REQUIRE(d->n_pen >= 1 && d->n_pen <= VQVAE_SEG_MAX_PEN, who ": n_pen must be in [1, %d] (got %d)",                    \
             VQVAE_SEG_MAX_PEN, (int)d->n_pen);                                                                            \
  VQ_REQUIRE(d->ttot >= d->n, who ": ttot must be at least n (got %lld of %d)", (long long)d->ttot, (int)d->n);            \
  VQ_REQUIRE(d->stride >= d->ttot, who ": stride must be at least ttot (got %lld of %lld)", (long long)d->stride,          \
             (long long)d->ttot);                                                                                          \
  VQ_REQUIRE(d->code_stride >= d->ttot, who ": code_stride must be at least ttot (got %lld of %lld)",                      \
             (long long)d->code_stride, (long long)d->ttot);                                                               \
  VQ_REQUIRE(d->utt_stride >= d->n, who ": utt_stride must be at least n (got %lld of %d)", (long long)d->utt_stride,      \
             (int)d->n);                                                                                                   \
  VQ_REQUIRE(sg_finite_penalties(d), who ": every penalty must be finite and not negative")

extern "C" size_t vqvae_seg_workspace_bytes(const vqvae_seg_desc* d) {
  if (!d || d->n < 1 || d->d < 1 || d->k < 1 || d->k > VQVAE_SEG_MAX_K || d->n_pen < 1 || d->n_pen > VQVAE_SEG_MAX_PEN ||
      d->ttot < d->n || d->stride < d->ttot || d->code_stride < d->ttot || d->utt_stride < d->n || !sg_finite_penalties(d))
    return (size_t)-1;
  return sg_plan(d).total;
}

extern "C" int vqvae_seg_distances(const vqvae_seg_desc* d, const float* z, const float* W, double* table,
                                   vqvae_stream_t stream) {
  SG_REQUIRE_DESC("seg_distances", d);
  VQ_REQUIRE(z && W && table, "seg_distances: null z, W or table");
  return sg_launch_dist(d, z, W, table, (hipStream_t)stream);
}

extern "C" int vqvae_seg_segment(const vqvae_seg_desc* d, const float* z, const float* W, const int64_t* frame_off,
                                 int32_t* codes, int32_t* n_seg, double* cost, void* workspace, size_t workspace_bytes,
                                 vqvae_stream_t stream) {
  SG_REQUIRE_DESC("seg_segment", d);
  VQ_REQUIRE(z && W && frame_off && codes && n_seg && cost, "seg_segment: null z, W, frame_off, codes, n_seg or cost");
  const SgPlan plan = sg_plan(d);
  VQ_REQUIRE(workspace && workspace_bytes >= plan.total, "seg_segment: the workspace must hold %zu bytes (got %zu)",
             plan.total, workspace ? workspace_bytes : (size_t)0);
  VQ_REQUIRE(((uintptr_t)workspace & 7) == 0, "seg_segment: the workspace must be 8-byte aligned");
  char* ws = static_cast<char*>(workspace);
  double* table = reinterpret_cast<double*>(ws + plan.table);
  if (int e = sg_launch_dist(d, z, W, table, (hipStream_t)stream)) return e;
  SgDpArgs a{};
  a.D = table; a.off = frame_off;
  a.stay = reinterpret_cast<unsigned long long*>(ws + plan.stay);
  a.am = reinterpret_cast<int32_t*>(ws + plan.am);
  a.codes = codes; a.n_seg = n_seg; a.cost = cost;
  a.ttot = d->ttot; a.code_stride = d->code_stride; a.utt_stride = d->utt_stride;
  a.n = d->n; a.k = d->k; a.nw = (d->k + 63) / 64;
  for (int q = 0; q < VQVAE_SEG_MAX_PEN; ++q) a.lam[q] = q < d->n_pen ? d->lam[q] : 0.0;
  hipStream_t s = (hipStream_t)stream;
  const int k = d->k, P = d->n_pen;
  if (k <= 64) return sg_launch_dp<1, 1>(a, P, s);
  if (k <= 128) return sg_launch_dp<2, 1>(a, P, s);
  if (k <= 256) return sg_launch_dp<4, 1>(a, P, s);
  if (k <= VQVAE_SEG_WAVE_K) return sg_launch_dp<8, 1>(a, P, s);
  if (k <= 1024) return sg_launch_dp<4, 4>(a, P, s);
  if (k <= 2048) return sg_launch_dp<8, 4>(a, P, s);
  if (k <= 4096) return sg_launch_dp<16, 4>(a, P, s);
  return sg_launch_dp<32, 4>(a, P, s);
}
