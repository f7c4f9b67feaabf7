// EMA codebook updates for the vector quantiser (include/vqvae_vq_ema.h).
//
// accumulate: per-code counts n_j and per-code float64 sums S_j of the latents, no floating-point atomics.
//   B*T <= SMALL_MAX_N   ema_scan_kernel, ONE launch: a workgroup per code compacts its ascending row list in LDS (two
//                        passes over idx, each wave a contiguous stretch of rows), then each wave sums whole channels.
//   above                memset + ema_hist + ema_colscan + ema_basescan + ema_place: a stable counting sort of the row ids by
//                        code (per-chunk integer histograms, chunk-major offsets, one wave per chunk places its rows in
//                        ascending order with its cursors in LDS); ema_sum: a workgroup per PIECE of a code's list, found by a
//                        binary search over the per-code piece offsets, so a collapsed assignment spreads over the chip;
//                        ema_combine adds the piece sums of every code with more than one piece in piece order.
// n_j is the list length in both forms.  Both sum in the order the header defines (piece_sum below): same bits.
// In piece_sum neighbouring lanes take neighbouring list entries of ONE channel: z is (B,d,T) with T contiguous, so rows
// that are close in t share cache lines, which lanes spread over channels (stride T) never do.
//
// apply = ema_count_kernel (N_j) + ema_rows_kernel (every workgroup re-derives the float64 total from the new, by then
// read-only N in the same j-ascending order, then updates its rows of m and W): no scratch word between the two launches.
#include "common.h"
#include "../../include/vqvae_vq_ema.h"

namespace {

constexpr int PIECE = VQVAE_VQ_EMA_PIECE;
constexpr int SMALL_MAX_N = VQVAE_VQ_EMA_SMALL_MAX_N;
constexpr int SCAN_THREADS = 1024, SCAN_WAVES = SCAN_THREADS / 64;
constexpr int CHUNK = 4096;                 // rows per sort chunk (one wave places a chunk)
constexpr int PLACE_LDS_MAX_K = 16384;      // cursors of one chunk in LDS up to here (64 KB), in global memory above
constexpr int SUM_THREADS = 256, SUM_WAVES = SUM_THREADS / 64;
constexpr int ROWS_THREADS = 256;
constexpr int ROWS_TILE = 2048;             // N_j staged per round of the total

// One piece of one code's list for one channel: off[0..len) are element offsets of z[row, 0], ascending rows, len <= PIECE.
// Lane l adds entries l, l + 64, ... in order; the lane sums are folded 32, 16, ..., 1.  Every lane of the wave must call.
template <typename OffPtr>
__device__ __forceinline__ double piece_sum(const float* __restrict__ zc, OffPtr off, int len, int lane) {
  float v[PIECE / 64];
#pragma unroll
  for (int i = 0; i < PIECE / 64; ++i) {
    const int q = i * 64 + lane;
    v[i] = q < len ? zc[off[q]] : 0.0f;     // (+0.0 leaves a float64 sum's bits alone)
  }
  double acc = 0.0;
#pragma unroll
  for (int i = 0; i < PIECE / 64; ++i) acc += (double)v[i];
#pragma unroll
  for (int h = 32; h > 0; h >>= 1) acc += __shfl_down(acc, h, 64);
  return acc;                                // lane 0 holds the piece's sum
}

__global__ __launch_bounds__(SCAN_THREADS) void ema_scan_kernel(const int32_t* __restrict__ idx, const float* __restrict__ z,
                                                                int N, int d, int T, int k, float* __restrict__ stats) {
  __shared__ long off[SMALL_MAX_N];          // element offset of z[row, 0] for the rows quantised to code j, ascending
  __shared__ int wcnt[SCAN_WAVES];
  const int j = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int seg = (N + SCAN_THREADS - 1) / SCAN_THREADS * 64;     // rows per wave, a multiple of 64
  const int lo = wave * seg, hi = min(lo + seg, N);
  int mine = 0;
  for (int n0 = lo; n0 < hi; n0 += 64) {
    const int n = n0 + lane;
    mine += __popcll(__ballot(n < hi && idx[n] == j));
  }
  if (lane == 0) wcnt[wave] = mine;
  __syncthreads();
  int at = 0, cnt = 0;
  for (int w = 0; w < SCAN_WAVES; ++w) {
    if (w < wave) at += wcnt[w];
    cnt += wcnt[w];
  }
  for (int n0 = lo; n0 < hi; n0 += 64) {
    const int n = n0 + lane;
    const bool hit = n < hi && idx[n] == j;
    const unsigned long long m = __ballot(hit);
    if (hit) off[at + __popcll(m & ((1ull << lane) - 1ull))] = (long)(n / T) * d * T + n % T;
    at += __popcll(m);
  }
  __syncthreads();
  if (tid == 0) stats[j] = (float)cnt;
  float* S = stats + k + (size_t)j * d;
  for (int c = wave; c < d; c += SCAN_WAVES) {
    const float* zc = z + (size_t)c * T;
    double tot = 0.0;
    for (int p0 = 0; p0 < cnt; p0 += PIECE) tot += piece_sum(zc, off + p0, min(PIECE, cnt - p0), lane);
    if (lane == 0) S[c] = (float)tot;
  }
}

// ---- large N: stable counting sort of the row ids by code ---------------------------------------------------------------
__global__ __launch_bounds__(256) void ema_hist_kernel(const int32_t* __restrict__ idx, int N, int k,
                                                       int32_t* __restrict__ hist) {
  // hist[chunk][j] = rows of this chunk quantised to j (integer atomics: exact, order-free)
  int32_t* h = hist + (size_t)blockIdx.x * k;
  const int lo = blockIdx.x * CHUNK, hi = min(lo + CHUNK, N);
  for (int n = lo + threadIdx.x; n < hi; n += 256) {
    const int32_t c = idx[n];
    if ((uint32_t)c < (uint32_t)k) atomicAdd(&h[c], 1);
  }
}

__global__ __launch_bounds__(256) void ema_colscan_kernel(int32_t* __restrict__ hist, int nchunk, int k,
                                                          int32_t* __restrict__ cnt) {
  // in place: hist[chunk][j] -> rows of code j in earlier chunks; cnt[j] = rows of code j
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= k) return;
  int32_t run = 0;
  for (int c = 0; c < nchunk; ++c) {
    const int32_t h = hist[(size_t)c * k + j];
    hist[(size_t)c * k + j] = run;
    run += h;
  }
  cnt[j] = run;
}

__global__ __launch_bounds__(1024) void ema_basescan_kernel(int32_t* __restrict__ base, int32_t* __restrict__ pbase, int k) {
  // base[j] holds cnt[j] on entry.  Exclusive scans, ONE workgroup: base[j] = first slot of code j's list, base[k] = rows
  // with a valid index; pbase[j] = first piece of code j, every code has at least one (an empty code writes zeros)
  __shared__ int32_t sa[1024], sb[1024];
  __shared__ int32_t carry_a, carry_b;
  const int tid = threadIdx.x;
  if (tid == 0) { carry_a = 0; carry_b = 0; }
  __syncthreads();
  for (int j0 = 0; j0 < k; j0 += 1024) {
    const int j = j0 + tid;
    const int32_t a = j < k ? base[j] : 0;
    const int32_t b = j < k ? max(1, (a + PIECE - 1) / PIECE) : 0;
    sa[tid] = a; sb[tid] = b;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
      const int32_t va = tid >= o ? sa[tid - o] : 0, vb = tid >= o ? sb[tid - o] : 0;
      __syncthreads();
      sa[tid] += va; sb[tid] += vb;
      __syncthreads();
    }
    if (j < k) { base[j] = carry_a + sa[tid] - a; pbase[j] = carry_b + sb[tid] - b; }
    __syncthreads();
    if (tid == 1023) { carry_a += sa[1023]; carry_b += sb[1023]; }
    __syncthreads();
  }
  if (tid == 0) { base[k] = carry_a; pbase[k] = carry_b; }
}

template <bool LDS>
__global__ __launch_bounds__(64) void ema_place_kernel(const int32_t* __restrict__ idx, int N, int k,
                                                       int32_t* __restrict__ hist, const int32_t* __restrict__ base,
                                                       int32_t* __restrict__ sorted) {
  // one wave owns one chunk and its cursors: rows are visited in ascending order, 64 at a time; lanes holding the same code
  // take consecutive slots in lane (= row) order.  volatile: the cursor accesses of different lanes keep their program order
  extern __shared__ int32_t cur_lds[];
  const int lane = threadIdx.x;
  int32_t* mine = hist + (size_t)blockIdx.x * k;
  if (LDS) {
    for (int j = lane; j < k; j += 64) cur_lds[j] = base[j] + mine[j];
    __syncthreads();
  } else {
    for (int j = lane; j < k; j += 64) mine[j] += base[j];
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
  }
  volatile int32_t* cursor = LDS ? cur_lds : mine;
  const int lo = blockIdx.x * CHUNK, hi = min(lo + CHUNK, N);
  for (int g = lo; g < hi; g += 64) {
    const int n = g + lane;
    const int32_t c = n < hi ? idx[n] : -1;
    const bool live = (uint32_t)c < (uint32_t)k;       // an index outside the codebook takes no slot
    unsigned long long todo = __ballot(live);
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const int32_t c0 = __shfl(c, leader);
      const unsigned long long m = __ballot(live && c == c0);
      const int32_t start = cursor[c0];                 // same address in every lane: one broadcast load
      if (live && c == c0) sorted[start + __popcll(m & ((1ull << lane) - 1ull))] = n;
      __builtin_amdgcn_s_waitcnt(0);                    // the load above precedes the leader's store below
      if (lane == leader) cursor[c0] = start + __popcll(m);
      __builtin_amdgcn_s_waitcnt(0);                    // ... and is complete before the next group's load
      todo &= ~m;
    }
  }
}

__global__ __launch_bounds__(SUM_THREADS) void ema_sum_kernel(const int32_t* __restrict__ sorted,
                                                              const int32_t* __restrict__ base,
                                                              const int32_t* __restrict__ pbase,
                                                              const float* __restrict__ z, int d, int T, int k,
                                                              double* __restrict__ part64, float* __restrict__ stats) {
  __shared__ long off[PIECE];
  const int p = blockIdx.x;
  if (p >= pbase[k]) return;                            // (uniform over the workgroup)
  int a = 0, b = k;                                     // the code j with pbase[j] <= p < pbase[j + 1]
  while (b - a > 1) {
    const int mid = (a + b) >> 1;
    if (pbase[mid] <= p) a = mid; else b = mid;
  }
  const int j = a, s = p - pbase[j], pieces = pbase[j + 1] - pbase[j];
  const int beg = base[j], cnt = base[j + 1] - beg;
  const int lo = s * PIECE, len = max(0, min(PIECE, cnt - lo));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int q = tid; q < len; q += SUM_THREADS) {
    const int n = sorted[beg + lo + q];
    off[q] = (long)(n / T) * d * T + n % T;
  }
  __syncthreads();
  if (s == 0 && tid == 0) stats[j] = (float)cnt;
  for (int c = wave; c < d; c += SUM_WAVES) {
    const double v = piece_sum(z + (size_t)c * T, off, len, lane);
    if (lane == 0) {
      if (pieces == 1) stats[k + (size_t)j * d + c] = (float)v;
      else part64[(size_t)p * d + c] = v;
    }
  }
}

__global__ __launch_bounds__(256) void ema_combine_kernel(const int32_t* __restrict__ pbase, const double* __restrict__ part64,
                                                          int k, int d, float* __restrict__ stats) {
  const size_t total = (size_t)k * d;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int j = (int)(i / d), c = (int)(i % d);
    const int p0 = pbase[j], pieces = pbase[j + 1] - p0;
    if (pieces <= 1) continue;                          // written by the sum kernel itself
    const double* src = part64 + (size_t)p0 * d + c;
    double acc = 0.0;
    int s = 0;
    for (; s + 8 <= pieces; s += 8) {                   // eight loads in flight, added in piece order
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = src[(size_t)(s + u) * d];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc += v[u];
    }
    for (; s < pieces; ++s) acc += src[(size_t)s * d];
    stats[k + i] = (float)acc;
  }
}

// ---- apply / reset -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ema_count_kernel(float* __restrict__ ema_count, const float* __restrict__ stats, int k,
                                                        float decay) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  const float w1 = 1.0f - decay;
  if (j < k) ema_count[j] = decay * ema_count[j] + w1 * stats[j];      // (-ffp-contract=off: two products, one sum)
}

__global__ __launch_bounds__(ROWS_THREADS) void ema_rows_kernel(float* __restrict__ W, const float* __restrict__ ema_count,
                                                                float* __restrict__ ema_sum, const float* __restrict__ stats,
                                                                int k, int d, float decay, float eps) {
  __shared__ float tile[ROWS_TILE];
  __shared__ double sh_total;
  const int tid = threadIdx.x;
  double total = 0.0;                                    // (thread 0's copy is the one that counts)
  for (int j0 = 0; j0 < k; j0 += ROWS_TILE) {
    const int n = min(ROWS_TILE, k - j0);
    for (int q = tid; q < n; q += ROWS_THREADS) tile[q] = ema_count[j0 + q];
    __syncthreads();
    if (tid == 0)
      for (int q = 0; q < n; ++q) total += (double)tile[q];            // j ascending: the order of the rule
    __syncthreads();
  }
  if (tid == 0) sh_total = total;
  __syncthreads();
  total = sh_total;
  const float w1 = 1.0f - decay;
  const double den = total + (double)k * (double)eps;
  const size_t cells = (size_t)k * d;
  for (size_t i = (size_t)blockIdx.x * ROWS_THREADS + tid; i < cells; i += (size_t)gridDim.x * ROWS_THREADS) {
    const int j = (int)(i / d);
    const float m = decay * ema_sum[i] + w1 * stats[k + i];
    ema_sum[i] = m;
    if (total != 0.0) {
      const float nt = (float)(((double)ema_count[j] + (double)eps) / den * total);
      W[i] = m / nt;
    }
  }
}

__global__ __launch_bounds__(256) void ema_reset_kernel(const float* __restrict__ W, float* __restrict__ ema_count,
                                                        float* __restrict__ ema_sum, int k, int d,
                                                        const int32_t* __restrict__ mask) {
  const size_t cells = (size_t)k * d;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < cells; i += (size_t)gridDim.x * 256) {
    const int j = (int)(i / d);
    if (mask != nullptr && mask[j] == 0) continue;
    ema_sum[i] = W[i];
    if (i == (size_t)j * d) ema_count[j] = 1.0f;
  }
}

struct LargePlan {
  size_t nchunk, max_pieces, hist_off, base_off, pbase_off, sorted_off, part_off, bytes;
};

LargePlan large_plan(size_t N, size_t d, size_t k) {
  LargePlan p;
  p.nchunk = (N + CHUNK - 1) / CHUNK;
  p.max_pieces = k + N / PIECE;                          // sum_j max(1, ceil(cnt_j / PIECE)) <= k + N / PIECE
  size_t at = 0;
  p.hist_off = at;   at += vq::align_up(p.nchunk * k * 4, 256);
  p.base_off = at;   at += vq::align_up((k + 1) * 4, 256);
  p.pbase_off = at;  at += vq::align_up((k + 1) * 4, 256);
  p.sorted_off = at; at += vq::align_up(N * 4, 256);
  p.part_off = at;   at += vq::align_up(p.max_pieces * d * 8, 256);
  p.bytes = at;
  return p;
}

bool shapes_ok(int B, int d, int T, int k) {
  return B > 0 && d > 0 && T > 0 && k > 0 && (long long)B * T < VQVAE_VQ_EMA_MAX_N && k <= (1 << 24) &&
         (long long)k * d < (1ll << 40);
}

int grid_for(size_t cells, int threads, int cap) {
  const size_t g = (cells + threads - 1) / threads;
  return (int)(g < 1 ? 1 : (g > (size_t)cap ? (size_t)cap : g));
}

}  // namespace

extern "C" {

int vqvae_vq_ema_abi_version(void) { return 1; }

size_t vqvae_vq_ema_workspace_bytes(int B, int d, int T, int k) {
  if (!shapes_ok(B, d, T, k)) return 0;
  const size_t N = (size_t)B * T;
  if (N <= (size_t)SMALL_MAX_N) return 256;              // unused: the list lives in LDS
  return large_plan(N, d, k).bytes;
}

int vqvae_vq_ema_accumulate(const int32_t* idx, const float* z, int B, int d, int T, int k, float* stats, void* ws,
                            size_t ws_bytes, vqvae_vq_ema_stream_t s) {
  VQ_REQUIRE(idx && z && stats && ws, "vqvae_vq_ema_accumulate: null pointer");
  VQ_REQUIRE(B > 0 && d > 0 && T > 0 && k > 0, "vqvae_vq_ema_accumulate: B, d, T, k must be positive (got %d, %d, %d, %d)",
             B, d, T, k);
  VQ_REQUIRE((long long)B * T < VQVAE_VQ_EMA_MAX_N,
             "vqvae_vq_ema_accumulate: B*T = %lld rows; a float32 count is exact below 2^24 rows only", (long long)B * T);
  VQ_REQUIRE(shapes_ok(B, d, T, k), "vqvae_vq_ema_accumulate: k = %d, d = %d beyond the kernels' index range", k, d);
  VQ_REQUIRE(ws_bytes >= vqvae_vq_ema_workspace_bytes(B, d, T, k),
             "vqvae_vq_ema_accumulate: workspace of %zu bytes, vqvae_vq_ema_workspace_bytes asks for %zu", ws_bytes,
             vqvae_vq_ema_workspace_bytes(B, d, T, k));
  hipStream_t st = (hipStream_t)s;
  const int N = B * T;
  if (N <= SMALL_MAX_N) {
    hipLaunchKernelGGL(ema_scan_kernel, dim3(k), dim3(SCAN_THREADS), 0, st, idx, z, N, d, T, k, stats);
    VQ_LAUNCH_CHECK();
    return 0;
  }
  const LargePlan p = large_plan((size_t)N, (size_t)d, (size_t)k);
  char* w = (char*)ws;
  int32_t* hist = (int32_t*)(w + p.hist_off);
  int32_t* base = (int32_t*)(w + p.base_off);
  int32_t* pbase = (int32_t*)(w + p.pbase_off);
  int32_t* sorted = (int32_t*)(w + p.sorted_off);
  double* part64 = (double*)(w + p.part_off);
  const int nchunk = (int)p.nchunk;
  VQ_CHECK_HIP(hipMemsetAsync(hist, 0, p.nchunk * k * 4, st));
  hipLaunchKernelGGL(ema_hist_kernel, dim3(nchunk), dim3(256), 0, st, idx, N, k, hist);
  VQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(ema_colscan_kernel, dim3(vq::cdiv(k, 256)), dim3(256), 0, st, hist, nchunk, k, base);
  VQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(ema_basescan_kernel, dim3(1), dim3(1024), 0, st, base, pbase, k);
  VQ_LAUNCH_CHECK();
  if (k <= PLACE_LDS_MAX_K)
    hipLaunchKernelGGL(ema_place_kernel<true>, dim3(nchunk), dim3(64), (size_t)k * 4, st, idx, N, k, hist,
                       (const int32_t*)base, sorted);
  else
    hipLaunchKernelGGL(ema_place_kernel<false>, dim3(nchunk), dim3(64), 0, st, idx, N, k, hist, (const int32_t*)base, sorted);
  VQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(ema_sum_kernel, dim3((unsigned)p.max_pieces), dim3(SUM_THREADS), 0, st, (const int32_t*)sorted,
                     (const int32_t*)base, (const int32_t*)pbase, z, d, T, k, part64, stats);
  VQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(ema_combine_kernel, dim3(grid_for((size_t)k * d, 256, 4096)), dim3(256), 0, st, (const int32_t*)pbase,
                     (const double*)part64, k, d, stats);
  VQ_LAUNCH_CHECK();
  return 0;
}

int vqvae_vq_ema_apply(float* W, float* ema_count, float* ema_sum, const float* stats, int k, int d, float decay, float eps,
                       vqvae_vq_ema_stream_t s) {
  VQ_REQUIRE(W && ema_count && ema_sum && stats, "vqvae_vq_ema_apply: null pointer");
  VQ_REQUIRE(shapes_ok(1, d, 1, k), "vqvae_vq_ema_apply: k, d must be positive and in range (got %d, %d)", k, d);
  VQ_REQUIRE(decay >= 0.0f && decay <= 1.0f, "vqvae_vq_ema_apply: decay %g outside [0, 1]", (double)decay);
  VQ_REQUIRE(eps > 0.0f, "vqvae_vq_ema_apply: eps %g must be positive", (double)eps);
  hipStream_t st = (hipStream_t)s;
  hipLaunchKernelGGL(ema_count_kernel, dim3(vq::cdiv(k, 256)), dim3(256), 0, st, ema_count, stats, k, decay);
  VQ_LAUNCH_CHECK();
  // every workgroup walks all k counts for the total: few, fat workgroups
  hipLaunchKernelGGL(ema_rows_kernel, dim3(grid_for((size_t)k * d, ROWS_THREADS * 8, 256)), dim3(ROWS_THREADS), 0, st, W,
                     (const float*)ema_count, ema_sum, stats, k, d, decay, eps);
  VQ_LAUNCH_CHECK();
  return 0;
}

int vqvae_vq_ema_reset(const float* W, float* ema_count, float* ema_sum, int k, int d, const int32_t* mask,
                       vqvae_vq_ema_stream_t s) {
  VQ_REQUIRE(W && ema_count && ema_sum, "vqvae_vq_ema_reset: null pointer");
  VQ_REQUIRE(shapes_ok(1, d, 1, k), "vqvae_vq_ema_reset: k, d must be positive and in range (got %d, %d)", k, d);
  hipLaunchKernelGGL(ema_reset_kernel, dim3(grid_for((size_t)k * d, 256, 4096)), dim3(256), 0, (hipStream_t)s, W, ema_count,
                     ema_sum, k, d, mask);
  VQ_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
