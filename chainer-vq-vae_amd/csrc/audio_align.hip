// Dynamic time warping over mel-cepstra for a ragged list of utterance pairs (include/vqvae_align.h states the rule).
//
// align_cepstra_kernel: a thread per frame; the frame's n_mels log-mel values are read once per coefficient (coalesced
//   along the frame axis, the dct row is the same address for the whole wave) and summed in float64, m ascending.
// align_dtw_kernel: ONE workgroup of 256 threads per pair walks the anti-diagonals k = i + j = 0 .. Fa + Fb - 2.  The cells
//   of a diagonal depend on the two diagonals before it only, so they are computed side by side, thread t the cells
//   pLo + t, pLo + t + 256, ... of the diagonal (p: the cell's coordinate on the SHORTER side; a diagonal has at most
//   min(Fa, Fb) cells).  Three diagonals rotate through LDS -- D double, K and the diagonal count int32, indexed by p --
//   diagonal k in slot k mod 3, so the slot written at k + 1 is the one read as "k - 2" at k: ONE barrier per diagonal
//   separates the two.  Dynamic LDS: 48 * max_short bytes, asked for through lds_opt_in above 64 KB (147456 bytes at
//   VQVAE_ALIGN_MAX_SHORT; the 160 KiB of a CU allow it).  A workgroup uses 48 * min(Fa, Fb) of it.
//   A cell's local cost reads the two frames' cepstra from global memory (2 * n_mcep doubles; the pair's cepstra are a
//   few hundred KB at most and stay in L2, a diagonal's reads are consecutive frames).  The direction byte of a cell goes
//   to the workspace diagonal-major (the header's layout), so that a diagonal's stores are consecutive bytes.
// align_path_kernel: one workgroup per pair; thread 0 walks the directions back from the end cell (a chain of dependent
//   byte loads), the path is written ascending, and after a barrier the 256 lanes add the along-path log-mel terms in the
//   header's order.
//
// A pair whose table entries contradict the descriptor (more cells, frames or path positions than the descriptor's sums, a
// shorter side above max_short) is skipped: path_len 0, NaN scores, nothing else written.  Every address is formed in 64
// bits; plain vector stores only.
#include "common.h"
#include "../../include/vqvae_align.h"

namespace vq {

constexpr int AL_THREADS = VQVAE_ALIGN_THREADS;
constexpr int AL_LANES = VQVAE_ALIGN_REDUCE_LANES;
constexpr size_t AL_LDS_CAP = 160 * 1024;           // the LDS of a CU, which one workgroup may take
constexpr size_t AL_CELL_BYTES = 3 * (sizeof(double) + 2 * sizeof(int));   // three diagonals of (D, K, diagonal count)
constexpr double AL_DB = 4.3429448190325175;        // 10 / ln 10, as MT_DB of audio_metrics.hip
static_assert(AL_CELL_BYTES * VQVAE_ALIGN_MAX_SHORT <= AL_LDS_CAP, "three diagonals of the longest pair must fit a CU's LDS");
static_assert(AL_THREADS == AL_LANES, "the path kernel reduces with its whole workgroup");

// cells of the first n diagonals of an S x L matrix (S <= L), n <= L
__host__ __device__ __forceinline__ long long al_first(long long n, long long S) {
  return n <= S ? n * (n + 1) / 2 : S * (S + 1) / 2 + (n - S) * S;
}
// first cell of diagonal k in the diagonal-major direction table
__host__ __device__ __forceinline__ long long al_diag_start(long long k, long long S, long long L) {
  return k <= L ? al_first(k, S) : S * L - al_first(S + L - 1 - k, S);
}

struct CepArgs {
  const float* log_mel; const float* dct; double* c;
  long long ftot, stride;
  int n_mels, n_mcep;
};

__global__ __launch_bounds__(AL_THREADS) void align_cepstra_kernel(CepArgs a) {
  const long long f = (long long)blockIdx.x * AL_THREADS + threadIdx.x;
  if (f >= a.ftot) return;
  for (int q = 0; q < a.n_mcep; ++q) {
    double c = 0.0;
    for (int m = 0; m < a.n_mels; ++m) c += (double)a.dct[q * a.n_mels + m] * (double)a.log_mel[(long long)m * a.stride + f];
    a.c[f * a.n_mcep + q] = c;
  }
}

struct PairGeom {
  long long oa, ob, co, po, Fa, Fb;
  bool ok;
};

__device__ __forceinline__ PairGeom al_pair(const vqvae_align_tables& t, const vqvae_align_desc& d, long long i) {
  PairGeom g;
  g.oa = (long long)t.off_a[i]; g.ob = (long long)t.off_b[i]; g.co = (long long)t.cell_off[i]; g.po = (long long)t.path_off[i];
  g.Fa = (long long)t.off_a[i + 1] - g.oa;
  g.Fb = (long long)t.off_b[i + 1] - g.ob;
  const long long S = g.Fa < g.Fb ? g.Fa : g.Fb;
  g.ok = g.Fa >= 1 && g.Fb >= 1 && S <= d.max_short && g.oa >= 0 && g.ob >= 0 && g.co >= 0 && g.po >= 0 &&
         g.oa + g.Fa <= d.fa_tot && g.ob + g.Fb <= d.fb_tot && g.Fa <= 0x7fffffffLL && g.Fb <= 0x7fffffffLL &&
         g.Fa * g.Fb <= (1LL << 31) && g.co + g.Fa * g.Fb <= d.cells && g.po + g.Fa + g.Fb - 1 <= d.ptot;
  return g;
}

struct DtwArgs {
  vqvae_align_desc d; vqvae_align_tables t;
  const double* ca; const double* cb; unsigned char* dirs;
  double* cost; int32_t* path_len; int32_t* diagonal_steps;
};

__global__ __launch_bounds__(AL_THREADS) void align_dtw_kernel(DtwArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char al_lds[];
  const int tid = threadIdx.x;
  const long long pair = blockIdx.x;
  const PairGeom g = al_pair(a.t, a.d, pair);
  if (!g.ok) {                                              // uniform for the workgroup
    if (tid == 0) { a.cost[pair] = __longlong_as_double(0x7ff8000000000000LL); a.path_len[pair] = 0; a.diagonal_steps[pair] = 0; }
    return;
  }
  const bool by_i = g.Fa <= g.Fb;                           // p is i, else j
  const int S = (int)(by_i ? g.Fa : g.Fb), L = (int)(by_i ? g.Fb : g.Fa);
  double* s_D = reinterpret_cast<double*>(al_lds);          // [3][S]
  int* s_K = reinterpret_cast<int*>(s_D + 3 * (size_t)S);   // [3][S]
  int* s_G = s_K + 3 * (size_t)S;                           // [3][S]
  const int Q = a.d.n_mcep;
  const double* ca = a.ca + g.oa * Q;
  const double* cb = a.cb + g.ob * Q;
  unsigned char* dirs = a.dirs + g.co;
  const int nd = S + L - 1;
  // where the "up" (i - 1, j) and "left" (i, j - 1) neighbours stand in the previous diagonal, relative to p
  const int up_at = by_i ? -1 : 0, left_at = by_i ? 0 : -1;

  int cur = 0, prev = 2, prev2 = 1;                         // slots of diagonals k, k - 1, k - 2
  for (int k = 0; k < nd; ++k) {
    const int pLo = k > L - 1 ? k - (L - 1) : 0;
    const int pHi = k < S - 1 ? k : S - 1;
    unsigned char* drow = dirs + al_diag_start(k, S, L) - pLo;
    const double* Dp = s_D + (size_t)prev * S; const double* Dq = s_D + (size_t)prev2 * S;
    const int* Kp = s_K + (size_t)prev * S; const int* Kq = s_K + (size_t)prev2 * S;
    const int* Gp = s_G + (size_t)prev * S; const int* Gq = s_G + (size_t)prev2 * S;
    for (int p = pLo + tid; p <= pHi; p += AL_THREADS) {
      const int r = k - p;                                  // the coordinate on the longer side
      const int i = by_i ? p : r, j = by_i ? r : p;
      const double* xa = ca + (long long)i * Q;
      const double* xb = cb + (long long)j * Q;
      double s = 0.0;
#pragma unroll 8
      for (int q = 0; q < Q; ++q) {                         // unrolled: the loads of eight coefficients travel together
        const double h = 0.5 * (xa[q] - xb[q]);
        s += h * h;
      }
      const double dl = AL_DB * sqrt(2.0 * s);
      double best = 0.0;
      int dir = 3, Kb = 0, Gb = 0;
      if (p > 0 && r > 0) { best = Dq[p - 1]; Kb = Kq[p - 1]; Gb = Gq[p - 1] + 1; dir = 0; }
      if (i > 0) {
        const double v = Dp[p + up_at];
        if (dir == 3 || v < best) { best = v; Kb = Kp[p + up_at]; Gb = Gp[p + up_at]; dir = 1; }
      }
      if (j > 0) {
        const double v = Dp[p + left_at];
        if (dir == 3 || v < best) { best = v; Kb = Kp[p + left_at]; Gb = Gp[p + left_at]; dir = 2; }
      }
      const double Dc = dir == 3 ? dl : best + dl;
      s_D[(size_t)cur * S + p] = Dc;
      s_K[(size_t)cur * S + p] = Kb + 1;
      s_G[(size_t)cur * S + p] = Gb;
      drow[p] = (unsigned char)dir;
      if (k == nd - 1) { a.cost[pair] = Dc; a.path_len[pair] = Kb + 1; a.diagonal_steps[pair] = Gb; }
    }
    __syncthreads();
    const int f = prev2; prev2 = prev; prev = cur; cur = f;
  }
}

struct PathArgs {
  vqvae_align_desc d; vqvae_align_tables t;
  const unsigned char* dirs; const double* cost; const int32_t* path_len;
  const float* la; const float* lb;
  int32_t* ia; int32_t* ib; double* scores;
};

__global__ __launch_bounds__(AL_THREADS) void align_path_kernel(PathArgs a) {
  __shared__ double s_p[AL_LANES];
  const int tid = threadIdx.x;
  const long long pair = blockIdx.x;
  const PairGeom g = al_pair(a.t, a.d, pair);
  const int K = a.path_len[pair];
  if (!g.ok || K < 1 || K > g.Fa + g.Fb - 1) {             // uniform for the workgroup
    if (tid == 0) { a.scores[2 * pair] = a.scores[2 * pair + 1] = __longlong_as_double(0x7ff8000000000000LL); }
    return;
  }
  int32_t* ia = a.ia + g.po;
  int32_t* ib = a.ib + g.po;
  if (tid == 0) {
    const bool by_i = g.Fa <= g.Fb;
    const long long S = by_i ? g.Fa : g.Fb, L = by_i ? g.Fb : g.Fa;
    const unsigned char* dirs = a.dirs + g.co;
    long long i = g.Fa - 1, j = g.Fb - 1;
    for (int s = 0; s < K; ++s) {
      ia[K - 1 - s] = (int32_t)i;
      ib[K - 1 - s] = (int32_t)j;
      const long long k = i + j, p = by_i ? i : j;
      const long long pLo = k > L - 1 ? k - (L - 1) : 0;
      const int dir = dirs[al_diag_start(k, S, L) + p - pLo];
      if (dir == 0 && i > 0 && j > 0) { --i; --j; }
      else if (dir == 1 && i > 0) --i;
      else if (dir == 2 && j > 0) --j;
      else break;                                           // the start cell (or a byte the DP did not write: stop)
    }
  }
  __threadfence_block();
  __syncthreads();
  const int M = a.d.n_mels;
  const float* la = a.la + g.oa;
  const float* lb = a.lb + g.ob;
  const long long terms = (long long)K * M;
  double acc = 0.0;
  for (long long e = tid; e < terms; e += AL_LANES) {
    const long long k = e / M;
    const long long m = e - k * M;
    acc += fabs((double)la[m * a.d.stride_a + ia[k]] - (double)lb[m * a.d.stride_b + ib[k]]);
  }
  s_p[tid] = acc;
  __syncthreads();
  for (int h = AL_LANES / 2; h >= 1; h >>= 1) {
    if (tid < h) s_p[tid] += s_p[tid + h];
    __syncthreads();
  }
  if (tid == 0) {
    a.scores[2 * pair] = a.cost[pair] / (double)K;
    a.scores[2 * pair + 1] = s_p[0] / (double)terms;
  }
}

static bool align_desc_ok(const vqvae_align_desc* d) {
  return d && d->n >= 1 && d->n_mels >= 1 && d->n_mels <= VQVAE_ALIGN_MAX_MELS && d->n_mcep >= 1 && d->n_mcep < d->n_mels &&
         d->max_short >= 1 && d->max_short <= VQVAE_ALIGN_MAX_SHORT && d->fa_tot >= d->n && d->fb_tot >= d->n &&
         d->stride_a >= d->fa_tot && d->stride_b >= d->fb_tot && d->cells >= d->n && d->ptot >= d->n;
}

// the one workspace plan of each entry point
struct AlignPlan { size_t dirs, path, total; };
static AlignPlan plan_cepstra(const vqvae_align_desc*) { WsPlan p; return AlignPlan{0, 0, p.total}; }
static AlignPlan plan_dtw(const vqvae_align_desc* d) {
  WsPlan p;
  const size_t dirs = p.take((size_t)d->cells);
  return AlignPlan{dirs, 0, p.total};
}
static AlignPlan plan_path(const vqvae_align_desc* d) {
  WsPlan p;
  const size_t path = p.take(2 * sizeof(int32_t) * (size_t)d->ptot);
  return AlignPlan{0, path, p.total};
}

}  // namespace vq

using namespace vq;

extern "C" int vqvae_align_abi_version(void) { return 1; }

extern "C" size_t vqvae_align_cepstra_workspace_bytes(const vqvae_align_desc* d) {
  if (!align_desc_ok(d)) return (size_t)-1;
  return plan_cepstra(d).total;
}

extern "C" size_t vqvae_align_dtw_workspace_bytes(const vqvae_align_desc* d) {
  if (!align_desc_ok(d)) return (size_t)-1;
  return plan_dtw(d).total;
}

extern "C" size_t vqvae_align_path_workspace_bytes(const vqvae_align_desc* d) {
  if (!align_desc_ok(d)) return (size_t)-1;
  return plan_path(d).total;
}

#define AL_REQUIRE_DESC(who, d)                                                                                            \
  VQ_REQUIRE(d, who ": null descriptor");                                                                                  \
  VQ_REQUIRE(d->n >= 1, who ": n must be at least 1 (got %d)", (int)d->n);                                                 \
  VQ_REQUIRE(d->n_mels >= 1 && d->n_mels <= VQVAE_ALIGN_MAX_MELS, who ": n_mels must be in [1, %d] (got %d)",              \
             VQVAE_ALIGN_MAX_MELS, (int)d->n_mels);                                                                        \
  VQ_REQUIRE(d->n_mcep >= 1 && d->n_mcep < d->n_mels, who ": n_mcep must be in [1, n_mels) (got %d of %d)",                \
             (int)d->n_mcep, (int)d->n_mels);                                                                              \
  VQ_REQUIRE(d->max_short >= 1 && d->max_short <= VQVAE_ALIGN_MAX_SHORT, who ": max_short must be in [1, %d] (got %d)",    \
             VQVAE_ALIGN_MAX_SHORT, (int)d->max_short);                                                                    \
  VQ_REQUIRE(d->fa_tot >= d->n && d->fb_tot >= d->n, who ": fa_tot and fb_tot must be at least n (got %lld and %lld of %d)", \
             (long long)d->fa_tot, (long long)d->fb_tot, (int)d->n);                                                       \
  VQ_REQUIRE(d->stride_a >= d->fa_tot && d->stride_b >= d->fb_tot,                                                         \
             who ": strides must be at least the frame totals (got %lld of %lld and %lld of %lld)", (long long)d->stride_a, \
             (long long)d->fa_tot, (long long)d->stride_b, (long long)d->fb_tot);                                          \
  VQ_REQUIRE(d->cells >= d->n && d->ptot >= d->n, who ": cells and ptot must be at least n (got %lld and %lld of %d)",     \
             (long long)d->cells, (long long)d->ptot, (int)d->n)

extern "C" int vqvae_align_cepstra(const vqvae_align_desc* d, int side, const float* log_mel, const float* dct, double* c,
                                   void* ws, size_t ws_bytes, vqvae_stream_t stream) {
  AL_REQUIRE_DESC("align_cepstra", d);
  VQ_REQUIRE(side == 0 || side == 1, "align_cepstra: side must be 0 or 1 (got %d)", side);
  VQ_REQUIRE(log_mel && dct && c, "align_cepstra: null log_mel, dct or c");
  const AlignPlan plan = plan_cepstra(d);
  VQ_REQUIRE(ws_bytes >= plan.total && (ws || !plan.total), "align_cepstra: workspace of %zu bytes, %zu needed", ws_bytes, plan.total);
  CepArgs a{};
  a.log_mel = log_mel; a.dct = dct; a.c = c;
  a.ftot = side ? d->fb_tot : d->fa_tot; a.stride = side ? d->stride_b : d->stride_a;
  a.n_mels = d->n_mels; a.n_mcep = d->n_mcep;
  const long long blocks = (a.ftot + AL_THREADS - 1) / AL_THREADS;
  VQ_REQUIRE(blocks <= 0x7fffffffLL, "align_cepstra: %lld frames are more than 2^31 - 1 workgroups", a.ftot);
  hipLaunchKernelGGL(align_cepstra_kernel, dim3((unsigned)blocks), dim3(AL_THREADS), 0, (hipStream_t)stream, a);
  VQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int vqvae_align_dtw(const vqvae_align_desc* d, const vqvae_align_tables* t, const double* ca, const double* cb,
                               double* cost, int32_t* path_len, int32_t* diagonal_steps, void* ws, size_t ws_bytes,
                               vqvae_stream_t stream) {
  AL_REQUIRE_DESC("align_dtw", d);
  VQ_REQUIRE(t && t->off_a && t->off_b && t->cell_off && t->path_off, "align_dtw: null tables");
  VQ_REQUIRE(ca && cb && cost && path_len && diagonal_steps, "align_dtw: null ca, cb, cost, path_len or diagonal_steps");
  const AlignPlan plan = plan_dtw(d);
  VQ_REQUIRE(ws && ws_bytes >= plan.total, "align_dtw: workspace of %zu bytes, %zu needed", ws_bytes, plan.total);
  DtwArgs a{};
  a.d = *d; a.t = *t; a.ca = ca; a.cb = cb; a.dirs = static_cast<unsigned char*>(ws) + plan.dirs;
  a.cost = cost; a.path_len = path_len; a.diagonal_steps = diagonal_steps;
  const size_t lds = AL_CELL_BYTES * (size_t)d->max_short;
  if (int e = lds_opt_in<align_dtw_kernel>(lds)) return e;
  hipLaunchKernelGGL(align_dtw_kernel, dim3((unsigned)d->n), dim3(AL_THREADS), lds, (hipStream_t)stream, a);
  VQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int vqvae_align_path(const vqvae_align_desc* d, const vqvae_align_tables* t, const void* dirs, const double* cost,
                                const int32_t* path_len, const float* log_mel_a, const float* log_mel_b, int32_t* ia,
                                int32_t* ib, double* scores, void* ws, size_t ws_bytes, vqvae_stream_t stream) {
  AL_REQUIRE_DESC("align_path", d);
  VQ_REQUIRE(t && t->off_a && t->off_b && t->cell_off && t->path_off, "align_path: null tables");
  VQ_REQUIRE(dirs && cost && path_len && log_mel_a && log_mel_b && scores,
             "align_path: null dirs, cost, path_len, log_mel_a, log_mel_b or scores");
  VQ_REQUIRE((ia == nullptr) == (ib == nullptr), "align_path: ia and ib must both be given or both be null");
  const AlignPlan plan = plan_path(d);
  if (!ia) VQ_REQUIRE(ws && ws_bytes >= plan.total, "align_path: workspace of %zu bytes, %zu needed to keep the paths", ws_bytes, plan.total);
  PathArgs a{};
  a.d = *d; a.t = *t; a.dirs = static_cast<const unsigned char*>(dirs); a.cost = cost; a.path_len = path_len;
  a.la = log_mel_a; a.lb = log_mel_b; a.scores = scores;
  if (ia) { a.ia = ia; a.ib = ib; }
  else {
    a.ia = reinterpret_cast<int32_t*>(static_cast<unsigned char*>(ws) + plan.path);
    a.ib = a.ia + d->ptot;
  }
  hipLaunchKernelGGL(align_path_kernel, dim3((unsigned)d->n), dim3(AL_THREADS), 0, (hipStream_t)stream, a);
  VQ_LAUNCH_CHECK();
  return 0;
}
