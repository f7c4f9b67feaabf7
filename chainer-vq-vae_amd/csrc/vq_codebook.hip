// Codebook usage statistics and dead-code re-seeding (include/vqvae_codebook.h).
//
// observe = three launches on the caller's stream:
//   codebook_draw_kernel      zeroes counts; reservoir[j,:] = z row n_j (one wave per code, the hash is wave-uniform)
//   codebook_hist_kernel      counts += histogram(idx): LDS-privatised int32 bins per workgroup, merged with one global
//                             INTEGER atomic add per non-empty bin (k <= VQVAE_CODEBOOK_LDS_MAX_K), or one global integer
//                             atomic add per index above that
//   codebook_finalize_kernel  ONE workgroup: usage blend, entropy / used-code reduction in a fixed order (float64, no
//                             atomics), interval sums, *steps_seen += 1 last
// Nothing here depends on arrival order except integer sums, so every output is bit-reproducible.
#include "common.h"
#include "../../include/vqvae_codebook.h"

namespace {

constexpr int HIST_THREADS = 256;
constexpr int HIST_ROWS_PER_WG = 4096;      // indices per workgroup before the grid stops growing
constexpr int HIST_MAX_WGS = 256;           // one per CU: every workgroup pays k LDS stores and up to k global atomics
constexpr int FIN_THREADS = 512;

__device__ __forceinline__ uint64_t codebook_hash(uint64_t seed, int32_t step, int j) {
  // the counter-based hash of include/vqvae_codebook.h (splitmix64 finaliser over seed + (ctr + 1) * golden ratio)
  uint64_t ctr = ((uint64_t)(uint32_t)step << 32) | (uint64_t)(uint32_t)j;
  uint64_t x = seed + (ctr + 1ull) * 0x9E3779B97F4A7C15ull;
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

__global__ __launch_bounds__(256) void codebook_draw_kernel(const float* __restrict__ z, int d, int T, int N, int k,
                                                            uint64_t seed, const int32_t* __restrict__ steps_seen,
                                                            int32_t* __restrict__ counts, float* __restrict__ reservoir) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g < k) counts[g] = 0;                       // (the grid has 64 threads per code)
  const int j = g >> 6, lane = g & 63;
  if (j >= k) return;
  const int32_t step = *steps_seen;
  const uint32_t n = (uint32_t)(codebook_hash(seed, step, j) % (uint64_t)N);      // < N: inside z
  const int b = n / (uint32_t)T, t = n % (uint32_t)T;
  const float* src = z + (size_t)b * d * T + t;
  float* dst = reservoir + (size_t)j * d;
  for (int c = lane; c < d; c += 64) dst[c] = src[(size_t)c * T];
}

template <bool LDS>
__device__ __forceinline__ void hist_add(int32_t j, int k, int32_t* bins, int32_t* counts) {
  if ((uint32_t)j >= (uint32_t)k) return;         // an index outside the codebook is not counted (and never addressed)
  if (LDS) atomicAdd(&bins[j], 1);                // ds_add_u32
  else atomicAdd(&counts[j], 1);
}

template <bool LDS>
__global__ __launch_bounds__(HIST_THREADS) void codebook_hist_kernel(const int32_t* __restrict__ idx, int N, int n4, int k,
                                                                     int32_t* __restrict__ counts) {
  extern __shared__ int32_t bins[];
  const int tid = threadIdx.x;
  if (LDS) {
    for (int j = tid; j < k; j += HIST_THREADS) bins[j] = 0;
    __syncthreads();
  }
  const int stride = gridDim.x * HIST_THREADS;
  const int g = blockIdx.x * HIST_THREADS + tid;
  const int4* idx4 = reinterpret_cast<const int4*>(idx);     // n4 > 0 only when idx is 16-byte aligned
  for (int i = g; i < n4; i += stride) {
    const int4 q = idx4[i];
    hist_add<LDS>(q.x, k, bins, counts);
    hist_add<LDS>(q.y, k, bins, counts);
    hist_add<LDS>(q.z, k, bins, counts);
    hist_add<LDS>(q.w, k, bins, counts);
  }
  for (int i = 4 * n4 + g; i < N; i += stride) hist_add<LDS>(idx[i], k, bins, counts);
  if (LDS) {
    __syncthreads();
    for (int j = tid; j < k; j += HIST_THREADS) {
      const int32_t c = bins[j];
      if (c) atomicAdd(&counts[j], c);
    }
  }
}

__global__ __launch_bounds__(FIN_THREADS) void codebook_finalize_kernel(const int32_t* __restrict__ counts, int k, int N,
                                                                        float decay, float* __restrict__ usage,
                                                                        int32_t* __restrict__ steps_seen,
                                                                        double* __restrict__ stats) {
  __shared__ double sh_h[FIN_THREADS / 64];
  __shared__ int sh_u[FIN_THREADS / 64];
  const int tid = threadIdx.x;
  const int32_t step = *steps_seen;
  const float omd = 1.0f - decay;
  double h = 0.0;
  int used = 0;
  for (int j = tid; j < k; j += FIN_THREADS) {
    const int32_t c = counts[j];
    const float cf = (float)c;
    usage[j] = step == 0 ? cf : decay * usage[j] + omd * cf;       // (-ffp-contract=off: three rounded operations)
    if (c > 0) {
      const double p = (double)c / (double)N;
      h += p * log(p);
      ++used;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {                          // fixed tree inside the wave
    h += __shfl_down(h, off, 64);
    used += __shfl_down(used, off, 64);
  }
  if ((tid & 63) == 0) { sh_h[tid >> 6] = h; sh_u[tid >> 6] = used; }
  __syncthreads();                                                   // (every thread has read *steps_seen by now)
  if (tid == 0) {
    double hs = 0.0;
    int us = 0;
    for (int w = 0; w < FIN_THREADS / 64; ++w) { hs += sh_h[w]; us += sh_u[w]; }   // waves in order
    const double perp = exp(-hs);
    stats[0] = perp;
    stats[1] = (double)us;
    stats[2] += perp;
    stats[3] += (double)us;
    stats[4] += 1.0;
    *steps_seen = step + 1;
  }
}

__global__ __launch_bounds__(256) void codebook_reseed_kernel(float* __restrict__ W, float* __restrict__ m,
                                                              float* __restrict__ v, int k, int d,
                                                              float* __restrict__ usage, const float* __restrict__ reservoir,
                                                              float threshold, float revived_usage,
                                                              int32_t* __restrict__ n_reseeded, int32_t* __restrict__ mask) {
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;     // one wave per code
  if (j >= k) return;
  const bool dead = usage[j] < threshold;          // wave-uniform; false for a NaN
  if (dead) {
    const size_t row = (size_t)j * d;
    for (int c = lane; c < d; c += 64) {
      W[row + c] = reservoir[row + c];
      if (m != nullptr) { m[row + c] = 0.0f; v[row + c] = 0.0f; }
    }
  }
  if (lane == 0) {
    mask[j] = dead ? 1 : 0;
    if (dead) {
      usage[j] = revived_usage;
      atomicAdd(n_reseeded, 1);                    // integer: order-independent
    }
  }
}

}  // namespace

extern "C" {

int vqvae_codebook_abi_version(void) { return 1; }

int vqvae_codebook_observe(const int32_t* idx, const float* z, int B, int d, int T, int k, float decay, uint64_t seed,
                           int32_t* counts, float* usage, float* reservoir, int32_t* steps_seen, double* stats,
                           vqvae_codebook_stream_t s) {
  VQ_REQUIRE(idx && z && counts && usage && reservoir && steps_seen && stats, "vqvae_codebook_observe: null pointer");
  VQ_REQUIRE(B > 0 && d > 0 && T > 0 && k > 0, "vqvae_codebook_observe: B, d, T, k must be positive (got %d, %d, %d, %d)",
             B, d, T, k);
  VQ_REQUIRE((long long)B * T < (1ll << 31) && (long long)k * 64 < (1ll << 31),
             "vqvae_codebook_observe: B*T = %lld rows / k = %d codes do not fit the kernels' 32-bit indices", (long long)B * T, k);
  VQ_REQUIRE(decay >= 0.0f && decay <= 1.0f, "vqvae_codebook_observe: decay %g outside [0, 1]", (double)decay);
  VQ_REQUIRE(((uintptr_t)stats & 7) == 0, "vqvae_codebook_observe: stats must be 8-byte aligned");
  hipStream_t st = (hipStream_t)s;
  const int N = B * T;
  hipLaunchKernelGGL(codebook_draw_kernel, dim3(vq::cdiv(k * 64, 256)), dim3(256), 0, st, z, d, T, N, k, seed,
                     (const int32_t*)steps_seen, counts, reservoir);
  VQ_LAUNCH_CHECK();
  const int n4 = ((uintptr_t)idx & 15) == 0 ? N / 4 : 0;
  if (k <= VQVAE_CODEBOOK_LDS_MAX_K) {
    int wgs = vq::cdiv(N, HIST_ROWS_PER_WG);
    wgs = wgs < 1 ? 1 : (wgs > HIST_MAX_WGS ? HIST_MAX_WGS : wgs);
    hipLaunchKernelGGL(codebook_hist_kernel<true>, dim3(wgs), dim3(HIST_THREADS), (size_t)k * sizeof(int32_t), st, idx, N,
                       n4, k, counts);
  } else {
    int wgs = vq::cdiv(N, 4 * HIST_THREADS);
    wgs = wgs < 1 ? 1 : (wgs > 1024 ? 1024 : wgs);
    hipLaunchKernelGGL(codebook_hist_kernel<false>, dim3(wgs), dim3(HIST_THREADS), 0, st, idx, N, n4, k, counts);
  }
  VQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(codebook_finalize_kernel, dim3(1), dim3(FIN_THREADS), 0, st, (const int32_t*)counts, k, N, decay, usage,
                     steps_seen, stats);
  VQ_LAUNCH_CHECK();
  return 0;
}

int vqvae_codebook_reseed(float* W, float* m, float* v, int k, int d, float* usage, const float* reservoir,
                          float threshold, float revived_usage, int32_t* n_reseeded, int32_t* mask,
                          vqvae_codebook_stream_t s) {
  VQ_REQUIRE(W && usage && reservoir && n_reseeded && mask, "vqvae_codebook_reseed: null pointer");
  VQ_REQUIRE((m == nullptr) == (v == nullptr), "vqvae_codebook_reseed: pass both Adam moments or neither");
  VQ_REQUIRE(k > 0 && d > 0, "vqvae_codebook_reseed: k, d must be positive (got %d, %d)", k, d);
  hipStream_t st = (hipStream_t)s;
  VQ_CHECK_HIP(hipMemsetAsync(n_reseeded, 0, sizeof(int32_t), st));
  hipLaunchKernelGGL(codebook_reseed_kernel, dim3(vq::cdiv(k, 4)), dim3(256), 0, st, W, m, v, k, d, usage, reservoir,
                     threshold, revived_usage, n_reseeded, mask);
  VQ_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
