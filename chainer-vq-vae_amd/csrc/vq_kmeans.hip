// k-means initialisation of the codebook (include/vqvae_kmeans.h): k-means++ seeding, centroid update, inertia.
//
// seed = k rounds of two launches:
//   kmeans_pick_kernel   ONE workgroup of 1 024 threads finishes the summation tree over the block sums in LDS (2 048 leaves
//                        a chunk, every level kept), walks down it to a block, rebuilds that block's 256 leaves from D, walks
//                        down to the row and copies the row into W and into the round's centre.
//   kmeans_dist_kernel   lanes over neighbouring rows, the channel loop inside the thread: with the (d, N) layout every load is
//                        a coalesced run along N.  <4>: four rows a thread by one 16-byte load per channel (N % 4 == 0, 16-byte
//                        aligned pool and mind), a wave is one block of 256 rows; <1>: one row a thread, a workgroup is one
//                        block -- small pools spread over four times the CUs, and it takes any alignment.  Eight channels
//                        of loads are in flight per thread; the centre is read through a uniform address (scalar loads).
//                        D = min(D, dist) and the block's node of the summation tree, float64, by wave shuffles.
// Nothing is handed between workgroups inside a launch: the kernel boundary is the only synchronisation.
// Both forms of the distance kernel add the same pairs (rows 2i, 2i+1 first, then neighbouring pairs, ...): same bits.
#include "common.h"
#include "../../include/vqvae_kmeans.h"

namespace {

constexpr int BLOCK = VQVAE_KMEANS_BLOCK;    // rows per block sum
constexpr int DIST_THREADS = 256;
constexpr int PICK_THREADS = 1024;
constexpr int LEAVES = 2 * PICK_THREADS;     // block sums per chunk of the pick kernel's tree
constexpr int MAX_CHUNKS = 32;               // 2^24 rows / 256 / 2048
constexpr int UNROLL = 8;                    // channels of loads in flight per thread

__device__ __forceinline__ uint64_t kmeans_hash(uint64_t seed, uint32_t word, uint32_t j) {
  // the counter-based hash of include/vqvae_codebook.h (splitmix64 finaliser over seed + (ctr + 1) * golden ratio)
  uint64_t ctr = ((uint64_t)word << 32) | (uint64_t)j;
  uint64_t x = seed + (ctr + 1ull) * 0x9E3779B97F4A7C15ull;
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

// sum over the 64 lanes in tree order: neighbouring lanes first (a + b is the same bits in both lanes of a pair)
__device__ __forceinline__ double wave_tree_sum(double v) {
#pragma unroll
  for (int h = 1; h < 64; h <<= 1) v += __shfl_xor(v, h, 64);
  return v;
}

template <int R> struct RowVec;
template <> struct RowVec<1> { typedef float type; };
template <> struct RowVec<4> { typedef float4 type; };

__device__ __forceinline__ float lane_of(const float& v, int) { return v; }
__device__ __forceinline__ float lane_of(const float4& v, int r) { return r == 0 ? v.x : r == 1 ? v.y : r == 2 ? v.z : v.w; }

// acc[r] = dist(row r, c) in the exact search's order for the R rows at p; centre(c) is the other side's channel c
template <int R, typename Centre>
__device__ __forceinline__ void row_distances(const float* __restrict__ p, size_t N, int d, Centre centre, float (&acc)[R]) {
  typedef typename RowVec<R>::type V;
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = 0.0f;
  int c = 0;
  for (; c + UNROLL <= d; c += UNROLL) {
    V x[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) x[u] = *reinterpret_cast<const V*>(p + (size_t)(c + u) * N);
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const float cv = centre(c + u);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float df = __fsub_rn(lane_of(x[u], r), cv);
        acc[r] = __fadd_rn(acc[r], __fmul_rn(df, df));
      }
    }
  }
  for (; c < d; ++c) {
    const V x = *reinterpret_cast<const V*>(p + (size_t)c * N);
    const float cv = centre(c);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float df = __fsub_rn(lane_of(x, r), cv);
      acc[r] = __fadd_rn(acc[r], __fmul_rn(df, df));
    }
  }
}

// the block's node of the tree from this thread's values (0 for rows past N); true in the thread that holds it
template <int R>
__device__ __forceinline__ bool block_sum(const float (&v)[R], double* wsum, double& out) {
  double s;
  if constexpr (R == 4) s = ((double)v[0] + (double)v[1]) + ((double)v[2] + (double)v[3]);
  else s = (double)v[0];
  s = wave_tree_sum(s);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if constexpr (R == 4) {                                  // a wave is a block
    out = s;
    return lane == 0;
  } else {
    if (lane == 0) wsum[wave] = s;
    __syncthreads();
    out = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
    return threadIdx.x == 0;
  }
}

template <int R, bool FIRST>
__global__ __launch_bounds__(DIST_THREADS) void kmeans_dist_kernel(const float* __restrict__ pool,
                                                                   const float* __restrict__ cen, int N, int d, int nblocks,
                                                                   float* __restrict__ mind, double* __restrict__ bsum) {
  __shared__ double wsum[DIST_THREADS / 64];
  const int tid = threadIdx.x;
  const int blk = R == 4 ? blockIdx.x * 4 + (tid >> 6) : blockIdx.x;
  const long r0 = (long)blk * BLOCK + (R == 4 ? (tid & 63) * 4 : tid);
  float D[R];
#pragma unroll
  for (int r = 0; r < R; ++r) D[r] = 0.0f;
  if (r0 < N) {                                            // (R == 4: N % 4 == 0, the four rows are in or out together)
    typedef typename RowVec<R>::type V;
    row_distances<R>(pool + r0, (size_t)N, d, [&](int c) { return cen[c]; }, D);
    if (!FIRST) {
      const V old = *reinterpret_cast<const V*>(mind + r0);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float o = lane_of(old, r);
        D[r] = D[r] < o ? D[r] : o;
      }
    }
    if constexpr (R == 4) *reinterpret_cast<float4*>(mind + r0) = make_float4(D[0], D[1], D[2], D[3]);
    else mind[r0] = D[0];
  }
  double s;
  if (block_sum<R>(D, wsum, s) && blk < nblocks) bsum[blk] = s;
}

__global__ __launch_bounds__(DIST_THREADS) void kmeans_inertia_kernel(const float* __restrict__ pool,
                                                                      const float* __restrict__ W,
                                                                      const int32_t* __restrict__ idx, int N, int d, int k,
                                                                      double* __restrict__ bsum) {
  __shared__ double wsum[DIST_THREADS / 64];
  const long r0 = (long)blockIdx.x * BLOCK + threadIdx.x;
  float D[1] = {0.0f};
  if (r0 < N) {
    const int32_t j = idx[r0];
    if ((uint32_t)j < (uint32_t)k) {
      const float* __restrict__ w = W + (size_t)j * d;
      row_distances<1>(pool + r0, (size_t)N, d, [&](int c) { return w[c]; }, D);
    }
  }
  double s;
  if (block_sum<1>(D, wsum, s)) bsum[blockIdx.x] = s;
}

// ---- the tree over the block sums, one workgroup ------------------------------------------------------------------------
// heap: node i has the children 2i and 2i + 1, the root is heap[1], the leaves are heap[LEAVES + i].  Thread t brings the
// leaves 2t and 2t + 1.  Ends with a barrier: every level is in LDS.
__device__ __forceinline__ void heap_build(double* heap, double a, double b) {
  const int tid = threadIdx.x, lane = tid & 63;
  __syncthreads();                                         // (the previous tree's readers are done)
  heap[LEAVES + 2 * tid] = a;
  heap[LEAVES + 2 * tid + 1] = b;
  double v = a + b;
  heap[PICK_THREADS + tid] = v;
#pragma unroll
  for (int h = 1; h < 64; h <<= 1) {
    v += __shfl_xor(v, h, 64);
    if ((lane & (2 * h - 1)) == 0) heap[(PICK_THREADS + tid) / (2 * h)] = v;
  }
  __syncthreads();
  if (tid < 16) {                                          // over the 16 wave nodes heap[16 .. 31]
    double u = heap[16 + tid];
#pragma unroll
    for (int h = 1; h < 16; h <<= 1) {
      u += __shfl_xor(u, h, 64);
      if ((tid & (2 * h - 1)) == 0) heap[(16 + tid) / (2 * h)] = u;
    }
  }
  __syncthreads();
}

// one thread walks down from the root with the target t (include/vqvae_kmeans.h); returns the leaf, t becomes the rest
__device__ __forceinline__ int heap_descend(const double* heap, int leaves, double& t) {
  int i = 1;
  while (i < leaves) {
    const double L = heap[2 * i], R = heap[2 * i + 1];
    if (t < L || !(R > 0.0)) {
      i = 2 * i;
    } else {
      t -= L;
      i = 2 * i + 1;
    }
  }
  return i - leaves;
}

__device__ __forceinline__ void chunk_leaves(const double* __restrict__ bsum, int nblocks, int chunk, double& a, double& b) {
  const int g = chunk * LEAVES + 2 * (int)threadIdx.x;
  a = g < nblocks ? bsum[g] : 0.0;
  b = g + 1 < nblocks ? bsum[g + 1] : 0.0;
}

// the root of the whole tree; with more than one chunk, cheap[] ends as the heap over the chunk roots (MAX_CHUNKS leaves)
__device__ __forceinline__ double tree_total(const double* __restrict__ bsum, int nblocks, double* heap, double* cheap) {
  const int nchunk = (nblocks + LEAVES - 1) / LEAVES;
  const int tid = threadIdx.x;
  for (int ch = 0; ch < nchunk; ++ch) {
    double a, b;
    chunk_leaves(bsum, nblocks, ch, a, b);
    heap_build(heap, a, b);
    if (nchunk == 1) return heap[1];
    if (tid == 0) cheap[MAX_CHUNKS + ch] = heap[1];
  }
  __syncthreads();
  if (tid < MAX_CHUNKS) {
    double u = tid < nchunk ? cheap[MAX_CHUNKS + tid] : 0.0;
    cheap[MAX_CHUNKS + tid] = u;
#pragma unroll
    for (int h = 1; h < MAX_CHUNKS; h <<= 1) {
      u += __shfl_xor(u, h, 64);
      if ((tid & (2 * h - 1)) == 0) cheap[(MAX_CHUNKS + tid) / (2 * h)] = u;
    }
  }
  __syncthreads();
  return cheap[1];
}

__global__ __launch_bounds__(PICK_THREADS) void kmeans_total_kernel(const double* __restrict__ bsum, int nblocks,
                                                                    double* __restrict__ out) {
  __shared__ double heap[2 * LEAVES];
  __shared__ double cheap[2 * MAX_CHUNKS];
  const double total = tree_total(bsum, nblocks, heap, cheap);
  if (threadIdx.x == 0) *out = total;
}

__global__ __launch_bounds__(PICK_THREADS) void kmeans_pick_kernel(const float* __restrict__ pool, int N, int d, int j,
                                                                   uint64_t seed, const float* __restrict__ mind,
                                                                   const double* __restrict__ bsum, int nblocks,
                                                                   float* __restrict__ W, int32_t* __restrict__ rows,
                                                                   float* __restrict__ cen) {
  __shared__ double heap[2 * LEAVES];
  __shared__ double cheap[2 * MAX_CHUNKS];
  __shared__ double sh_t;
  __shared__ int sh_i;
  const int tid = threadIdx.x;
  const uint64_t x = kmeans_hash(seed, 0u, (uint32_t)j);
  int row = (int)(x % (uint64_t)N);                        // round 0, and the rounds that find total == 0
  if (j > 0) {
    const int nchunk = (nblocks + LEAVES - 1) / LEAVES;
    const double total = tree_total(bsum, nblocks, heap, cheap);
    if (total > 0.0) {                                     // (uniform: every thread read the same LDS word)
      if (nchunk > 1) {
        if (tid == 0) {
          double t = (double)(x >> 40) * 0x1p-24 * total;
          sh_i = heap_descend(cheap, MAX_CHUNKS, t);
          sh_t = t;
        }
        __syncthreads();
        const int chunk = sh_i;
        double a, b;
        chunk_leaves(bsum, nblocks, chunk, a, b);
        heap_build(heap, a, b);
        if (tid == 0) {
          double t = sh_t;
          sh_i = chunk * LEAVES + heap_descend(heap, LEAVES, t);
          sh_t = t;
        }
      } else if (tid == 0) {
        double t = (double)(x >> 40) * 0x1p-24 * total;
        sh_i = heap_descend(heap, LEAVES, t);
        sh_t = t;
      }
      __syncthreads();
      int blk = sh_i;
      blk = blk < nblocks ? blk : nblocks - 1;             // (only a non-finite D could lead past the last block)
      const long r0 = (long)blk * BLOCK + 2 * tid;         // the block's rows are the first 256 leaves, the rest +0
      const double a = (2 * tid < BLOCK && r0 < N) ? (double)mind[r0] : 0.0;
      const double b = (2 * tid + 1 < BLOCK && r0 + 1 < N) ? (double)mind[r0 + 1] : 0.0;
      heap_build(heap, a, b);
      if (tid == 0) {
        double t = sh_t;
        const long r = (long)blk * BLOCK + heap_descend(heap, LEAVES, t);
        sh_i = (int)(r < N ? r : N - 1);
      }
      __syncthreads();
      row = sh_i;
    }
  }
  if (tid == 0) rows[j] = row;
  for (int c = tid; c < d; c += PICK_THREADS) {
    const float v = pool[(size_t)c * N + row];
    W[(size_t)j * d + c] = v;
    cen[c] = v;
  }
}

// ---- collect / update ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kmeans_collect_kernel(const float* __restrict__ z, int d, int T, int count,
                                                             float* __restrict__ pool, int N, int row0) {
  // one thread per (channel, row): neighbouring threads take neighbouring rows, contiguous along T on both sides
  const size_t cells = (size_t)d * count;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < cells; i += (size_t)gridDim.x * 256) {
    const int c = (int)(i / count), n = (int)(i % count);
    pool[(size_t)c * N + row0 + n] = z[((size_t)(n / T) * d + c) * T + n % T];
  }
}

__global__ __launch_bounds__(256) void kmeans_update_kernel(const float* __restrict__ pool, int N, int d, int k,
                                                            const float* __restrict__ stats, uint64_t seed, int iter,
                                                            float* __restrict__ W, int32_t* __restrict__ n_empty) {
  const size_t cells = (size_t)k * d;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < cells; i += (size_t)gridDim.x * 256) {
    const int j = (int)(i / d), c = (int)(i % d);
    const float n = stats[j];
    if (n > 0.0f) {
      W[i] = __fdiv_rn(stats[k + i], n);
    } else {
      const int row = (int)(kmeans_hash(seed, (uint32_t)iter + 1u, (uint32_t)j) % (uint64_t)N);
      W[i] = pool[(size_t)c * N + row];
      if (c == 0) atomicAdd(n_empty, 1);                   // an integer sum: exact, order-free
    }
  }
}

bool shapes_ok(int N, int d, int k) {
  return N >= 1 && N < VQVAE_KMEANS_MAX_N && d >= 1 && d <= VQVAE_KMEANS_MAX_D && k >= 1 && (long long)k * d < (1ll << 40);
}

// centre of the round | one float64 per block of rows
struct KmeansPlan { size_t nblocks, cen, bsum, total; };
KmeansPlan kmeans_plan(int N, int d) {
  vq::WsPlan w; KmeansPlan p;
  p.nblocks = ((size_t)N + BLOCK - 1) / BLOCK;
  p.cen = w.take((size_t)d * 4);
  p.bsum = w.take(p.nblocks * 8);
  p.total = w.total;
  return p;
}

int grid_for(size_t cells, int threads, int cap) {
  const size_t g = (cells + threads - 1) / threads;
  return (int)(g < 1 ? 1 : (g > (size_t)cap ? (size_t)cap : g));
}

template <int R>
void launch_dist(bool first, hipStream_t st, const float* pool, const float* cen, int N, int d, int nblocks, float* mind,
                 double* bsum) {
  const int grid = R == 4 ? (nblocks + 3) / 4 : nblocks;
  if (first)
    hipLaunchKernelGGL((kmeans_dist_kernel<R, true>), dim3(grid), dim3(DIST_THREADS), 0, st, pool, cen, N, d, nblocks, mind, bsum);
  else
    hipLaunchKernelGGL((kmeans_dist_kernel<R, false>), dim3(grid), dim3(DIST_THREADS), 0, st, pool, cen, N, d, nblocks, mind, bsum);
}

}  // namespace

extern "C" {

int vqvae_kmeans_abi_version(void) { return 1; }

size_t vqvae_kmeans_workspace_bytes(int N, int d, int k) {
  if (!shapes_ok(N, d, k)) return 0;
  return kmeans_plan(N, d).total;
}

int vqvae_kmeans_collect(const float* z, int B, int d, int T, int count, float* pool, int N, int row0,
                         vqvae_kmeans_stream_t s) {
  VQ_REQUIRE(z && pool, "vqvae_kmeans_collect: null pointer");
  VQ_REQUIRE(B > 0 && d > 0 && T > 0, "vqvae_kmeans_collect: B, d, T must be positive (got %d, %d, %d)", B, d, T);
  VQ_REQUIRE(N >= 1 && N < VQVAE_KMEANS_MAX_N, "vqvae_kmeans_collect: a pool of N = %d rows; 1 <= N < 2^24", N);
  VQ_REQUIRE(d <= VQVAE_KMEANS_MAX_D, "vqvae_kmeans_collect: d = %d channels, at most %d", d, VQVAE_KMEANS_MAX_D);
  VQ_REQUIRE(count >= 1 && (long long)count <= (long long)B * T, "vqvae_kmeans_collect: count = %d of %lld rows", count,
             (long long)B * T);
  VQ_REQUIRE(row0 >= 0 && (long long)row0 + count <= N,
             "vqvae_kmeans_collect: rows row0 = %d .. %lld do not fit a pool of N = %d rows", row0,
             (long long)row0 + count - 1, N);
  hipLaunchKernelGGL(kmeans_collect_kernel, dim3(grid_for((size_t)d * count, 256, 4096)), dim3(256), 0, (hipStream_t)s, z, d,
                     T, count, pool, N, row0);
  VQ_LAUNCH_CHECK();
  return 0;
}

int vqvae_kmeans_seed(const float* pool, int N, int d, int k, uint64_t seed, float* W, int32_t* rows, float* mind, void* ws,
                      size_t ws_bytes, vqvae_kmeans_stream_t s) {
  VQ_REQUIRE(pool && W && rows && mind && ws, "vqvae_kmeans_seed: null pointer");
  VQ_REQUIRE(N >= 1 && N < VQVAE_KMEANS_MAX_N, "vqvae_kmeans_seed: a pool of N = %d rows; 1 <= N < 2^24", N);
  VQ_REQUIRE(k >= 1 && d >= 1, "vqvae_kmeans_seed: k, d must be positive (got %d, %d)", k, d);
  VQ_REQUIRE(shapes_ok(N, d, k), "vqvae_kmeans_seed: k = %d, d = %d beyond the kernels' range (d <= %d)", k, d,
             VQVAE_KMEANS_MAX_D);
  const KmeansPlan p = kmeans_plan(N, d);
  VQ_REQUIRE(ws_bytes >= p.total, "vqvae_kmeans_seed: workspace of %zu bytes, vqvae_kmeans_workspace_bytes asks for %zu",
             ws_bytes, p.total);
  hipStream_t st = (hipStream_t)s;
  float* cen = (float*)((char*)ws + p.cen);
  double* bsum = (double*)((char*)ws + p.bsum);
  const int nblocks = (int)p.nblocks;
  // four rows a thread where 16-byte loads line up and a wave per block still fills the chip
  const bool wide = N % 4 == 0 && nblocks >= 1024 && ((uintptr_t)pool & 15) == 0 && ((uintptr_t)mind & 15) == 0;
  for (int j = 0; j < k; ++j) {
    hipLaunchKernelGGL(kmeans_pick_kernel, dim3(1), dim3(PICK_THREADS), 0, st, pool, N, d, j, seed, (const float*)mind,
                       (const double*)bsum, nblocks, W, rows, cen);
    VQ_LAUNCH_CHECK();
    if (wide) launch_dist<4>(j == 0, st, pool, cen, N, d, nblocks, mind, bsum);
    else launch_dist<1>(j == 0, st, pool, cen, N, d, nblocks, mind, bsum);
    VQ_LAUNCH_CHECK();
  }
  return 0;
}

int vqvae_kmeans_update(const float* pool, int N, int d, int k, const float* stats, uint64_t seed, int iter, float* W,
                        int32_t* n_empty, vqvae_kmeans_stream_t s) {
  VQ_REQUIRE(pool && stats && W && n_empty, "vqvae_kmeans_update: null pointer");
  VQ_REQUIRE(N >= 1 && N < VQVAE_KMEANS_MAX_N, "vqvae_kmeans_update: a pool of N = %d rows; 1 <= N < 2^24", N);
  VQ_REQUIRE(k >= 1 && d >= 1, "vqvae_kmeans_update: k, d must be positive (got %d, %d)", k, d);
  VQ_REQUIRE(shapes_ok(N, d, k), "vqvae_kmeans_update: k = %d, d = %d beyond the kernels' range (d <= %d)", k, d,
             VQVAE_KMEANS_MAX_D);
  VQ_REQUIRE(iter >= 0, "vqvae_kmeans_update: iter = %d must not be negative", iter);
  hipStream_t st = (hipStream_t)s;
  VQ_CHECK_HIP(hipMemsetAsync(n_empty, 0, 4, st));
  hipLaunchKernelGGL(kmeans_update_kernel, dim3(grid_for((size_t)k * d, 256, 4096)), dim3(256), 0, st, pool, N, d, k, stats,
                     seed, iter, W, n_empty);
  VQ_LAUNCH_CHECK();
  return 0;
}

int vqvae_kmeans_inertia(const float* pool, const float* W, const int32_t* idx, int N, int d, int k, double* out, void* ws,
                         size_t ws_bytes, vqvae_kmeans_stream_t s) {
  VQ_REQUIRE(pool && W && idx && out && ws, "vqvae_kmeans_inertia: null pointer");
  VQ_REQUIRE(N >= 1 && N < VQVAE_KMEANS_MAX_N, "vqvae_kmeans_inertia: a pool of N = %d rows; 1 <= N < 2^24", N);
  VQ_REQUIRE(k >= 1 && d >= 1, "vqvae_kmeans_inertia: k, d must be positive (got %d, %d)", k, d);
  VQ_REQUIRE(shapes_ok(N, d, k), "vqvae_kmeans_inertia: k = %d, d = %d beyond the kernels' range (d <= %d)", k, d,
             VQVAE_KMEANS_MAX_D);
  const KmeansPlan p = kmeans_plan(N, d);
  VQ_REQUIRE(ws_bytes >= p.total, "vqvae_kmeans_inertia: workspace of %zu bytes, vqvae_kmeans_workspace_bytes asks for %zu",
             ws_bytes, p.total);
  hipStream_t st = (hipStream_t)s;
  double* bsum = (double*)((char*)ws + p.bsum);
  const int nblocks = (int)p.nblocks;
  hipLaunchKernelGGL(kmeans_inertia_kernel, dim3(nblocks), dim3(DIST_THREADS), 0, st, pool, W, idx, N, d, k, bsum);
  VQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(kmeans_total_kernel, dim3(1), dim3(PICK_THREADS), 0, st, (const double*)bsum, nblocks, out);
  VQ_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
