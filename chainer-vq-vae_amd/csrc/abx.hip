// DTW distances of a ragged list of short item pairs over frame features (csrc/abx.h states the rule).
//
// abx_norms_kernel: a lane per frame, n[f] = sum_j x[j, f]^2 in float64, j ascending; a wave reads consecutive frames of
//   one channel row.
// abx_local_kernel<METRIC, ROWS>: the sums of step 2, grid (pair, slice).  ONE wavefront takes a tile of 16 x 16 frames:
//   per step of 32 channels the two tiles [32][16] are staged in LDS as float32; a lane owns 2 frames of a x 2 consecutive
//   frames of b (4 float64 accumulators) and walks j ascending in every cell: per channel two broadcast reads of a, one
//   8-byte read of b, and per cell one product and one addition (cosine) or a subtraction more (euclidean).  A cell's sum
//   is its own, so the tiling is not seen in the bits.  The workgroup's slices walk the pair's tiles, slice, slice + gridDim.y,
//   ...; most pairs are one tile.  ROWS: the operands are the rows of a codebook (k, d), one pair k x k (vqvae_abx_table).
//   Static LDS: 2 * 2048 bytes.  The kernel adds and multiplies only: nothing in it is fused.
// abx_cell_kernel<MODE>: cell by cell over the pairs' tables, 256 lanes.  MODE 0 / 1 turn the sums into the cosine /
//   euclidean cost in place (the correctly rounded square root and division live here, apart from the sums); MODE 2 is the
//   codes form: a gather from the (k, k) table.
// abx_dtw_wave_kernel: min(Fa, Fb) <= 64.  One wavefront per pair, lane p owns position p of the shorter side and walks
//   the anti-diagonals; its own (D, K) of the last diagonal and its lower neighbour's of the last two are registers, the
//   neighbour's arrive by one DPP wave shift per diagonal.  No LDS, no barrier.  The local costs of the next eight
//   diagonals are loaded while the current eight are walked, so the diagonal's dependency chain holds no load.
// abx_dtw_block_kernel: min(Fa, Fb) <= VQVAE_ABX_MAX_SHORT.  256 lanes per pair, three diagonals of (D, K) rotate through
//   LDS (36 * max_short bytes, dynamic), one barrier per diagonal, as align_dtw_kernel of audio_align.hip.
//
// A pair whose table entries contradict the descriptor is skipped and marked by the DP (the header); the other kernels
// leave it alone.  Every address is formed in 64 bits; plain vector stores only; no floating-point atomics.
#include "common.h"
#include "abx.h"

namespace vq {

constexpr int AB_TILE = VQVAE_ABX_TILE;
constexpr int AB_JT = 32;                             // channels staged at a time
constexpr int AB_LANES = VQVAE_ABX_LANES;
constexpr int AB_AHEAD = 8;                           // diagonals whose costs are loaded ahead of the walk
constexpr size_t AB_LDS_CAP = 160 * 1024;
constexpr size_t AB_CELL_BYTES = 3 * (sizeof(double) + sizeof(int));   // three diagonals of (D, K)
constexpr long long AB_MAX_CELLS = 1LL << 31;         // of one pair
constexpr long long AB_MAX_TOTAL = 1LL << 44;         // of one call: 128 TiB of float64, far above any device
static_assert(AB_TILE == 16, "a lane of one wavefront owns 2 x 2 cells of a 16 x 16 tile");
static_assert(AB_CELL_BYTES * VQVAE_ABX_MAX_SHORT <= 64 * 1024, "three diagonals at the bound need no LDS opt-in");
static_assert(2 * sizeof(float) * AB_JT * AB_TILE <= AB_LDS_CAP, "the local kernel's tiles must fit a CU's LDS");
static_assert(VQVAE_ABX_WAVE_SHORT == 64, "a lane per position of the shorter side");

__device__ __forceinline__ double ab_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

struct AbGeo {
  const int64_t* a_start; const int64_t* b_start; const int32_t* a_len; const int32_t* b_len; const int64_t* cell_off;
  long long ftot_a, ftot_b, cells;
  int max_short;
  int single;                                         // > 0: one pair, single x single frames from frame 0, cells from 0
};

struct AbPair {
  long long oa, ob, co;
  int Fa, Fb;
  bool ok;
};

__device__ __forceinline__ AbPair ab_pair(const AbGeo& g, long long i) {
  AbPair p;
  if (g.single > 0) {
    p.oa = p.ob = p.co = 0; p.Fa = p.Fb = g.single; p.ok = true;
    return p;
  }
  p.oa = (long long)g.a_start[i]; p.ob = (long long)g.b_start[i]; p.co = (long long)g.cell_off[i];
  p.Fa = g.a_len[i]; p.Fb = g.b_len[i];
  const int S = p.Fa < p.Fb ? p.Fa : p.Fb;
  const long long nc = (long long)p.Fa * (long long)p.Fb;
  p.ok = p.Fa >= 1 && p.Fb >= 1 && S <= g.max_short && p.oa >= 0 && p.ob >= 0 && p.oa <= g.ftot_a - p.Fa &&
         p.ob <= g.ftot_b - p.Fb && nc <= AB_MAX_CELLS && p.co >= 0 && p.co <= g.cells - nc;
  return p;
}

// ---- step 1 ---------------------------------------------------------------------------------------------------------------------
struct AbNormArgs {
  const float* x; double* n;
  long long ftot, cs, fs;                             // elements between channels and between frames
  int d;
};

__global__ __launch_bounds__(AB_LANES) void abx_norms_kernel(AbNormArgs a) {
  const long long f = (long long)blockIdx.x * AB_LANES + threadIdx.x;
  if (f >= a.ftot) return;
  const float* x = a.x + f * a.fs;
  double s = 0.0;
  for (int j = 0; j < a.d; ++j) {
    const double v = (double)x[(long long)j * a.cs];
    s += v * v;
  }
  a.n[f] = s;
}

// ---- step 2: the sums ---------------------------------------------------------------------------------------------------------------
struct AbLocalArgs {
  AbGeo g;
  const float* xa; const float* xb; double* out;
  long long stride_a, stride_b;
  int d;
};

template <bool ROWS>
__device__ __forceinline__ void ab_stage(float (*s)[AB_TILE], const float* x, long long stride, int d, long long o, int f0,
                                         int F, int j0, int lane) {
#pragma unroll
  for (int e = lane; e < AB_JT * AB_TILE; e += 64) {
    const int j = ROWS ? (e & (AB_JT - 1)) : (e >> 4);
    const int f = ROWS ? (e >> 5) : (e & (AB_TILE - 1));
    float v = 0.0f;
    if (j0 + j < d && f0 + f < F)
      v = ROWS ? x[(o + f0 + f) * (long long)d + j0 + j] : x[(long long)(j0 + j) * stride + o + f0 + f];
    s[j][f] = v;
  }
}

template <int METRIC, bool ROWS>
__global__ __launch_bounds__(64) void abx_local_kernel(AbLocalArgs a) {
  __shared__ __attribute__((aligned(16))) float s_a[AB_JT][AB_TILE];
  __shared__ __attribute__((aligned(16))) float s_b[AB_JT][AB_TILE];
  const int lane = threadIdx.x;
  const int tx = lane & 7, ty = lane >> 3;                  // frames of b: 2 tx + q; frames of a: ty + 8 u
  const AbPair p = ab_pair(a.g, blockIdx.x);
  if (!p.ok) return;                                        // uniform for the workgroup
  const long long tiles_b = (p.Fb + AB_TILE - 1) / AB_TILE;
  const long long tiles = (long long)((p.Fa + AB_TILE - 1) / AB_TILE) * tiles_b;
  double* out = a.out + p.co;
  for (long long tile = blockIdx.y; tile < tiles; tile += gridDim.y) {
    const int i0 = (int)(tile / tiles_b) * AB_TILE, c0 = (int)(tile % tiles_b) * AB_TILE;
    double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
    for (int j0 = 0; j0 < a.d; j0 += AB_JT) {
      const int jn = a.d - j0 < AB_JT ? a.d - j0 : AB_JT;
      ab_stage<ROWS>(s_a, a.xa, a.stride_a, a.d, p.oa, i0, p.Fa, j0, lane);
      ab_stage<ROWS>(s_b, a.xb, a.stride_b, a.d, p.ob, c0, p.Fb, j0, lane);
      __syncthreads();
#pragma unroll 8
      for (int j = 0; j < jn; ++j) {
        const float2 b2 = *reinterpret_cast<const float2*>(&s_b[j][2 * tx]);
        const double b[2] = {(double)b2.x, (double)b2.y};
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const double av = (double)s_a[j][ty + 8 * u];
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            if (METRIC == VQVAE_ABX_COSINE) {
              acc[u][q] += av * b[q];
            } else {
              const double df = av - b[q];
              acc[u][q] += df * df;
            }
          }
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int i = i0 + ty + 8 * u;
      if (i >= p.Fa) continue;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int c = c0 + 2 * tx + q;
        if (c < p.Fb) out[(long long)i * p.Fb + c] = acc[u][q];
      }
    }
  }
}

// ---- step 2: cell by cell -------------------------------------------------------------------------------------------------------
struct AbCellArgs {
  AbGeo g;
  const double* na; const double* nb;                       // MODE 0
  const int32_t* ca; const int32_t* cb; const double* table;   // MODE 2
  double* out;
  int k;
};

template <int MODE>
__global__ __launch_bounds__(AB_LANES) void abx_cell_kernel(AbCellArgs a) {
  const AbPair p = ab_pair(a.g, blockIdx.x);
  if (!p.ok) return;
  const long long nc = (long long)p.Fa * p.Fb;
  double* out = a.out + p.co;
  for (long long c = (long long)blockIdx.y * AB_LANES + threadIdx.x; c < nc; c += (long long)gridDim.y * AB_LANES) {
    const long long i = c / p.Fb;
    const long long j = c - i * p.Fb;
    double v;
    if (MODE == 0) {
      const double q = a.na[p.oa + i] * a.nb[p.ob + j];
      if (q == 0.0) {
        v = 1.0;
      } else {
        const double cs = out[c] / sqrt(q);
        v = 1.0 - cs;
        v = v < 0.0 ? 0.0 : v;
      }
    } else if (MODE == 1) {
      v = sqrt(out[c]);
    } else {
      const int x = a.ca[p.oa + i], y = a.cb[p.ob + j];
      v = (x >= 0 && x < a.k && y >= 0 && y < a.k) ? a.table[(long long)x * a.k + y] : ab_nan();
    }
    out[c] = v;
  }
}

// ---- step 3 -----------------------------------------------------------------------------------------------------------------------
struct AbDtwArgs {
  AbGeo g;
  const double* local; double* cost; int32_t* path_len; double* distance;
};

__device__ __forceinline__ void ab_mark(const AbDtwArgs& a, long long pair) {
  a.cost[pair] = ab_nan();
  a.distance[pair] = ab_nan();
  a.path_len[pair] = 0;
}

// the value of the lane below (lane - 1); lane 0 gets 0 and never uses it.  Every lane of the wave must be active.
__device__ __forceinline__ int ab_below(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ double ab_below(double v) {
  return __hiloint2double(ab_below(__double2hiint(v)), ab_below(__double2loint(v)));
}

__global__ __launch_bounds__(64) void abx_dtw_wave_kernel(AbDtwArgs a) {
  const int lane = threadIdx.x;
  const long long pair = blockIdx.x;
  const AbPair p = ab_pair(a.g, pair);
  if (!p.ok) {                                              // uniform for the wavefront
    if (lane == 0) ab_mark(a, pair);
    return;
  }
  const bool by_i = p.Fa <= p.Fb;                           // the lane's position is i, else j
  const int S = by_i ? p.Fa : p.Fb;
  const long long L = by_i ? p.Fb : p.Fa;
  const long long nd = S + L - 1;
  // cell (lane, r), r on the longer side: row-major (Fa, Fb)
  const double* mine = a.local + p.co + (by_i ? (long long)lane * p.Fb : (long long)lane);
  const long long step = by_i ? 1 : p.Fb;
  const bool in_s = lane < S;

  double cur[AB_AHEAD], nxt[AB_AHEAD];
#pragma unroll
  for (int u = 0; u < AB_AHEAD; ++u) {
    const long long r = (long long)u - lane;
    cur[u] = (in_s && r >= 0 && r < L) ? mine[r * step] : 0.0;
  }
  double Dp = 0.0, D2 = 0.0;                                // own D of diagonal k - 1; the lane below's of diagonal k - 2
  int Kp = 0, K2 = 0;
  for (long long k0 = 0; k0 < nd; k0 += AB_AHEAD) {
#pragma unroll
    for (int u = 0; u < AB_AHEAD; ++u) {
      const long long r = k0 + AB_AHEAD + u - lane;
      nxt[u] = (in_s && r >= 0 && r < L) ? mine[r * step] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < AB_AHEAD; ++u) {
      const long long r = k0 + u - lane;
      const bool active = in_s && r >= 0 && r < L;
      const double D1 = ab_below(Dp);                       // the lane below's D and K of diagonal k - 1
      const int K1 = ab_below(Kp);
      const bool low = lane > 0, back = r > 0;
      // candidates in the rule's order: (i-1, j-1), (i-1, j), (i, j-1)
      bool have = low && back;
      double best = D2;
      int Kb = K2;
      const double Dx = by_i ? D1 : Dp, Dy = by_i ? Dp : D1;
      const int Kx = by_i ? K1 : Kp, Ky = by_i ? Kp : K1;
      const bool hx = by_i ? low : back, hy = by_i ? back : low;
      if (hx && (!have || Dx < best)) { best = Dx; Kb = Kx; have = true; }
      if (hy && (!have || Dy < best)) { best = Dy; Kb = Ky; have = true; }
      const double Dc = have ? best + cur[u] : cur[u];
      const int Kc = have ? Kb + 1 : 1;
      D2 = D1; K2 = K1;
      Dp = active ? Dc : Dp;
      Kp = active ? Kc : Kp;
    }
#pragma unroll
    for (int u = 0; u < AB_AHEAD; ++u) cur[u] = nxt[u];
  }
  if (lane == S - 1) {                                      // its last cell was (S - 1, L - 1)
    a.cost[pair] = Dp;
    a.path_len[pair] = Kp;
    a.distance[pair] = Dp / (double)Kp;
  }
}

__global__ __launch_bounds__(AB_LANES) void abx_dtw_block_kernel(AbDtwArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ab_lds[];
  const int tid = threadIdx.x;
  const long long pair = blockIdx.x;
  const AbPair p = ab_pair(a.g, pair);
  if (!p.ok) {                                              // uniform for the workgroup
    if (tid == 0) ab_mark(a, pair);
    return;
  }
  const bool by_i = p.Fa <= p.Fb;
  const int S = by_i ? p.Fa : p.Fb, L = by_i ? p.Fb : p.Fa;
  double* s_D = reinterpret_cast<double*>(ab_lds);          // [3][S]
  int* s_K = reinterpret_cast<int*>(s_D + 3 * (size_t)S);   // [3][S]
  const double* local = a.local + p.co;
  const long long nd = (long long)S + L - 1;
  const int up_at = by_i ? -1 : 0, left_at = by_i ? 0 : -1; // where (i-1, j) and (i, j-1) stand in the previous diagonal
  int cur = 0, prev = 2, prev2 = 1;                         // slots of diagonals k, k - 1, k - 2
  for (long long k = 0; k < nd; ++k) {
    const int pLo = k > L - 1 ? (int)(k - (L - 1)) : 0;
    const int pHi = k < S - 1 ? (int)k : S - 1;
    const double* Dp = s_D + (size_t)prev * S; const double* Dq = s_D + (size_t)prev2 * S;
    const int* Kp = s_K + (size_t)prev * S; const int* Kq = s_K + (size_t)prev2 * S;
    for (int q = pLo + tid; q <= pHi; q += AB_LANES) {
      const long long r = k - q;                            // the coordinate on the longer side
      const long long i = by_i ? q : r, j = by_i ? r : q;
      const double dl = local[i * p.Fb + j];
      double best = 0.0;
      int Kb = 0;
      bool have = false;
      if (q > 0 && r > 0) { best = Dq[q - 1]; Kb = Kq[q - 1]; have = true; }
      if (i > 0) {
        const double v = Dp[q + up_at];
        if (!have || v < best) { best = v; Kb = Kp[q + up_at]; have = true; }
      }
      if (j > 0) {
        const double v = Dp[q + left_at];
        if (!have || v < best) { best = v; Kb = Kp[q + left_at]; have = true; }
      }
      const double Dc = have ? best + dl : dl;
      s_D[(size_t)cur * S + q] = Dc;
      s_K[(size_t)cur * S + q] = Kb + 1;
      if (k == nd - 1) {
        a.cost[pair] = Dc;
        a.path_len[pair] = Kb + 1;
        a.distance[pair] = Dc / (double)(Kb + 1);
      }
    }
    __syncthreads();
    const int f = prev2; prev2 = prev; prev = cur; cur = f;
  }
}

// ---- the host side --------------------------------------------------------------------------------------------------------------
static bool ab_desc_ok(const vqvae_abx_desc* d) {
  if (!d || d->n < 1 || (d->form != VQVAE_ABX_DENSE && d->form != VQVAE_ABX_CODES)) return false;
  if (d->form == VQVAE_ABX_DENSE) {
    if (d->d < 1 || d->d > VQVAE_ABX_MAX_D || (d->metric != VQVAE_ABX_COSINE && d->metric != VQVAE_ABX_EUCLIDEAN)) return false;
    if (d->stride_a < d->ftot_a || d->stride_b < d->ftot_b) return false;
  } else if (d->k < 1 || d->k > VQVAE_ABX_MAX_K) {
    return false;
  }
  return d->ftot_a >= 1 && d->ftot_b >= 1 && d->max_short >= 1 && d->max_short <= VQVAE_ABX_MAX_SHORT && d->cells >= d->n &&
         d->cells <= AB_MAX_TOTAL;
}

static AbGeo ab_geo(const vqvae_abx_desc* d, const vqvae_abx_tables* t) {
  AbGeo g{};
  g.a_start = t->a_start; g.b_start = t->b_start; g.a_len = t->a_len; g.b_len = t->b_len; g.cell_off = t->cell_off;
  g.ftot_a = d->ftot_a; g.ftot_b = d->ftot_b; g.cells = d->cells; g.max_short = d->max_short; g.single = 0;
  return g;
}

// slices of a pair: the average pair's work units, so that a list of small pairs is one slice each
static unsigned ab_slices(long long cells, long long n, long long per_slice) {
  const long long y = cells / (n * per_slice);
  return (unsigned)(y < 1 ? 1 : y > 1024 ? 1024 : y);
}

static int ab_launch_norms(const float* x, double* n, long long ftot, long long cs, long long fs, int d, hipStream_t stream) {
  AbNormArgs a{x, n, ftot, cs, fs, d};
  const long long blocks = (ftot + AB_LANES - 1) / AB_LANES;
  VQ_REQUIRE(blocks <= 0x7fffffffLL, "abx_norms: %lld frames are more than 2^31 - 1 workgroups", ftot);
  hipLaunchKernelGGL(abx_norms_kernel, dim3((unsigned)blocks), dim3(AB_LANES), 0, stream, a);
  VQ_LAUNCH_CHECK();
  return 0;
}

template <bool ROWS>
static int ab_launch_local(const AbLocalArgs& a, int metric, long long n, long long cells, hipStream_t stream) {
  const dim3 grid((unsigned)n, ab_slices(cells, n, AB_TILE * AB_TILE));
  if (metric == VQVAE_ABX_COSINE)
    hipLaunchKernelGGL((abx_local_kernel<VQVAE_ABX_COSINE, ROWS>), grid, dim3(64), 0, stream, a);
  else
    hipLaunchKernelGGL((abx_local_kernel<VQVAE_ABX_EUCLIDEAN, ROWS>), grid, dim3(64), 0, stream, a);
  VQ_LAUNCH_CHECK();
  return 0;
}

static int ab_launch_cell(const AbCellArgs& a, int mode, long long n, long long cells, hipStream_t stream) {
  const dim3 grid((unsigned)n, ab_slices(cells, n, 4 * AB_LANES));
  if (mode == 0) hipLaunchKernelGGL(abx_cell_kernel<0>, grid, dim3(AB_LANES), 0, stream, a);
  else if (mode == 1) hipLaunchKernelGGL(abx_cell_kernel<1>, grid, dim3(AB_LANES), 0, stream, a);
  else hipLaunchKernelGGL(abx_cell_kernel<2>, grid, dim3(AB_LANES), 0, stream, a);
  VQ_LAUNCH_CHECK();
  return 0;
}

}  // namespace vq

using namespace vq;

extern "C" int vqvae_abx_revision(void) { return 1; }

#define AB_REQUIRE_DESC(who, d)                                                                                            \
  VQ_REQUIRE(d, who ": null descriptor");                                                                                  \
  VQ_REQUIRE(d->n >= 1, who ": n must be at least 1 (got %d)", (int)d->n);                                                 \
  VQ_REQUIRE(d->form == VQVAE_ABX_DENSE || d->form == VQVAE_ABX_CODES, who ": form must be 0 (dense) or 1 (codes) (got %d)", \
             (int)d->form);                                                                                                \
  if (d->form == VQVAE_ABX_DENSE) {                                                                                        \
    VQ_REQUIRE(d->d >= 1 && d->d <= VQVAE_ABX_MAX_D, who ": d must be in [1, %d] (got %d)", VQVAE_ABX_MAX_D, (int)d->d);   \
    VQ_REQUIRE(d->metric == VQVAE_ABX_COSINE || d->metric == VQVAE_ABX_EUCLIDEAN,                                          \
               who ": metric must be 0 (cosine) or 1 (euclidean) (got %d)", (int)d->metric);                               \
  } else {                                                                                                                 \
    VQ_REQUIRE(d->k >= 1 && d->k <= VQVAE_ABX_MAX_K, who ": k must be in [1, %d] (got %d)", VQVAE_ABX_MAX_K, (int)d->k);   \
  }                                                                                                                        \
  VQ_REQUIRE(d->ftot_a >= 1 && d->ftot_b >= 1, who ": ftot_a and ftot_b must be at least 1 (got %lld and %lld)",           \
             (long long)d->ftot_a, (long long)d->ftot_b);                                                                  \
  if (d->form == VQVAE_ABX_DENSE) {                                                                                        \
    VQ_REQUIRE(d->stride_a >= d->ftot_a, who ": stride_a must be at least ftot_a (got %lld of %lld)",                      \
               (long long)d->stride_a, (long long)d->ftot_a);                                                              \
    VQ_REQUIRE(d->stride_b >= d->ftot_b, who ": stride_b must be at least ftot_b (got %lld of %lld)",                      \
               (long long)d->stride_b, (long long)d->ftot_b);                                                              \
  }                                                                                                                        \
  VQ_REQUIRE(d->max_short >= 1, who ": max_short must be at least 1 (got %d)", (int)d->max_short);                         \
  VQ_REQUIRE(d->max_short <= VQVAE_ABX_MAX_SHORT,                                                                          \
             who ": max_short must be at most %d (got %d): align whole utterances with align_many",                        \
             VQVAE_ABX_MAX_SHORT, (int)d->max_short);                                                                      \
  VQ_REQUIRE(d->cells >= d->n && d->cells <= AB_MAX_TOTAL, who ": cells must be in [n, 2^44] (got %lld of %d pairs)",      \
             (long long)d->cells, (int)d->n)

extern "C" size_t vqvae_abx_workspace_bytes(const vqvae_abx_desc* d) {
  if (!ab_desc_ok(d)) return (size_t)-1;
  return align_up((size_t)d->cells * sizeof(double), 256);
}

extern "C" int vqvae_abx_norms(const vqvae_abx_desc* d, int side, const float* x, double* n, vqvae_stream_t stream) {
  AB_REQUIRE_DESC("abx_norms", d);
  VQ_REQUIRE(d->form == VQVAE_ABX_DENSE, "abx_norms: the codes form has no norms");
  VQ_REQUIRE(side == 0 || side == 1, "abx_norms: side must be 0 (a) or 1 (b) (got %d)", side);
  VQ_REQUIRE(x && n, "abx_norms: null x or n");
  return ab_launch_norms(x, n, side ? d->ftot_b : d->ftot_a, side ? d->stride_b : d->stride_a, 1, d->d, (hipStream_t)stream);
}

static bool ab_tables_ok(const vqvae_abx_tables* t) {
  return t && t->a_start && t->b_start && t->a_len && t->b_len && t->cell_off;
}

extern "C" int vqvae_abx_local(const vqvae_abx_desc* d, const vqvae_abx_tables* t, const void* xa, const void* xb,
                               const double* na, const double* nb, const double* table, void* workspace,
                               size_t workspace_bytes, vqvae_stream_t stream) {
  AB_REQUIRE_DESC("abx_local", d);
  VQ_REQUIRE(ab_tables_ok(t), "abx_local: null tables or a null table among them");
  VQ_REQUIRE(xa && xb, "abx_local: null xa or xb");
  const size_t need = (size_t)d->cells * sizeof(double);
  VQ_REQUIRE(workspace && workspace_bytes >= need, "abx_local: the workspace must hold %zu bytes (got %zu)", need,
             workspace ? workspace_bytes : (size_t)0);
  VQ_REQUIRE(((uintptr_t)workspace & 7) == 0, "abx_local: the workspace must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  AbCellArgs c{};
  c.g = ab_geo(d, t);
  c.out = static_cast<double*>(workspace);
  if (d->form == VQVAE_ABX_CODES) {
    VQ_REQUIRE(table, "abx_local: the codes form needs a table");
    c.ca = static_cast<const int32_t*>(xa); c.cb = static_cast<const int32_t*>(xb); c.table = table; c.k = d->k;
    return ab_launch_cell(c, 2, d->n, d->cells, s);
  }
  VQ_REQUIRE(d->metric != VQVAE_ABX_COSINE || (na && nb), "abx_local: the cosine metric needs the norms na and nb");
  AbLocalArgs a{};
  a.g = c.g;
  a.xa = static_cast<const float*>(xa); a.xb = static_cast<const float*>(xb); a.out = c.out;
  a.stride_a = d->stride_a; a.stride_b = d->stride_b; a.d = d->d;
  if (int e = ab_launch_local<false>(a, d->metric, d->n, d->cells, s)) return e;
  c.na = na; c.nb = nb;
  return ab_launch_cell(c, d->metric == VQVAE_ABX_COSINE ? 0 : 1, d->n, d->cells, s);
}

extern "C" int vqvae_abx_dtw(const vqvae_abx_desc* d, const vqvae_abx_tables* t, const void* workspace, size_t workspace_bytes,
                             double* cost, int32_t* path_len, double* distance, vqvae_stream_t stream) {
  AB_REQUIRE_DESC("abx_dtw", d);
  VQ_REQUIRE(ab_tables_ok(t), "abx_dtw: null tables or a null table among them");
  VQ_REQUIRE(cost && path_len && distance, "abx_dtw: null cost, path_len or distance");
  const size_t need = (size_t)d->cells * sizeof(double);
  VQ_REQUIRE(workspace && workspace_bytes >= need, "abx_dtw: the workspace must hold %zu bytes (got %zu)", need,
             workspace ? workspace_bytes : (size_t)0);
  VQ_REQUIRE(((uintptr_t)workspace & 7) == 0, "abx_dtw: the workspace must be 8-byte aligned");
  AbDtwArgs a{};
  a.g = ab_geo(d, t);
  a.local = static_cast<const double*>(workspace);
  a.cost = cost; a.path_len = path_len; a.distance = distance;
  if (d->max_short <= VQVAE_ABX_WAVE_SHORT) {
    hipLaunchKernelGGL(abx_dtw_wave_kernel, dim3((unsigned)d->n), dim3(64), 0, (hipStream_t)stream, a);
  } else {
    const size_t lds = AB_CELL_BYTES * (size_t)d->max_short;
    hipLaunchKernelGGL(abx_dtw_block_kernel, dim3((unsigned)d->n), dim3(AB_LANES), lds, (hipStream_t)stream, a);
  }
  VQ_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t vqvae_abx_table_workspace_bytes(int32_t k) {
  if (k < 1 || k > VQVAE_ABX_MAX_K) return (size_t)-1;
  return align_up((size_t)k * sizeof(double), 256);
}

extern "C" int vqvae_abx_table(int32_t k, int32_t d, int32_t metric, const float* W, double* table, void* workspace,
                               size_t workspace_bytes, vqvae_stream_t stream) {
  VQ_REQUIRE(k >= 1 && k <= VQVAE_ABX_MAX_K, "abx_table: k must be in [1, %d] (got %d)", VQVAE_ABX_MAX_K, (int)k);
  VQ_REQUIRE(d >= 1 && d <= VQVAE_ABX_MAX_D, "abx_table: d must be in [1, %d] (got %d)", VQVAE_ABX_MAX_D, (int)d);
  VQ_REQUIRE(metric == VQVAE_ABX_COSINE || metric == VQVAE_ABX_EUCLIDEAN,
             "abx_table: metric must be 0 (cosine) or 1 (euclidean) (got %d)", (int)metric);
  VQ_REQUIRE(W && table, "abx_table: null W or table");
  const size_t need = (size_t)k * sizeof(double);
  VQ_REQUIRE(workspace && workspace_bytes >= need, "abx_table: the workspace must hold %zu bytes (got %zu)", need,
             workspace ? workspace_bytes : (size_t)0);
  VQ_REQUIRE(((uintptr_t)workspace & 7) == 0, "abx_table: the workspace must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  double* norms = static_cast<double*>(workspace);
  const long long cells = (long long)k * k;
  if (metric == VQVAE_ABX_COSINE)
    if (int e = ab_launch_norms(W, norms, k, 1, d, d, s)) return e;
  AbLocalArgs a{};
  a.g.single = k; a.g.max_short = k; a.g.ftot_a = a.g.ftot_b = k; a.g.cells = cells;
  a.xa = a.xb = W; a.out = table; a.d = d;
  if (int e = ab_launch_local<true>(a, metric, 1, cells, s)) return e;
  AbCellArgs c{};
  c.g = a.g; c.na = c.nb = norms; c.out = table;
  return ab_launch_cell(c, metric == VQVAE_ABX_COSINE ? 0 : 1, 1, cells, s);
}
