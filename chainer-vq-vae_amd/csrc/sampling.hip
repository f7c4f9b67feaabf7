// Sampling controls for generation (include/vqvae_sampling.h): temperature, top-k, nucleus (top-p) and greedy decoding,
// per sequence, as the finish launch of a generation step and as an entry point of its own.
//
// One kernel serves the per-step path (n <= 4), the lockstep path (n <= 128) and vqvae_sample_logits: one workgroup
// per sequence, so a sequence's arithmetic does not depend on n or on its place in the batch.  Because every workgroup
// reads the step counter, the counter is advanced by a launch of its own behind it (as in generate_lockstep.hip).
//   1. rank: 64-bit keys {order-reversed logit bits, class index} in LDS, bitonic sort (<= 1024 keys, 8 KB); the keys
//      are distinct, so the order is total and the network's result does not depend on how the threads are scheduled;
//   2. top-k: keep flags scattered back to index order;
//   3. softmax over the kept classes in gen_finish_kernel's own order of operations (classes outside add +0);
//   4. top-p: one thread walks the ranks adding p in float64 until the mass reaches top_p;
//   5. gen_finish_kernel's index-order float64 cdf and count.
// Without top-k and top-p (temperature alone) steps 1, 2 and 4 are skipped.  No floating-point atomics.
#include "common.h"
#include "../../include/vqvae_sampling.h"

namespace vq {

constexpr int SMP_MAXOUT = VQVAE_SAMPLING_MAX_CLASSES;
constexpr int SMP_THREADS = 256;

int gen_step_impl(const vqvae_gen_desc* d, const vqvae_gen_sampling* s, hipStream_t st);   // generate.hip

struct SampledArgs {
  const float* logits;      // (n, out_dim)
  const double* uniforms;   // (T, n, n_uniform)
  const void* forced;       // (T, n) int32 / float or nullptr
  void* out;                // int32 index / float value at [b * out_bstride + t]
  long out_bstride;
  float* logits_out;        // (T, n, out_dim) or nullptr
  float* probs_out;         // (n, out_dim) or nullptr
  float* x_cur;             // (n, input_dim): next input, written in place; nullptr: no feedback
  const int* step;          // nullptr: t = 0 (the sampler alone)
  const float* temperature; // (n,) or nullptr
  const int* top_k;
  const float* top_p;
  int max_steps, n, out_dim, input_dim, mode, n_uniform;
  float log_scale_min;
};

// ascending order of the key = (logit descending, index ascending); -0 ranks with +0
__device__ __forceinline__ unsigned long long smp_key(float v, int i) {
  if (v == 0.f) v = 0.f;
  const uint32_t bits = __float_as_uint(v);
  const uint32_t asc = bits ^ ((bits & 0x80000000u) ? 0xffffffffu : 0x80000000u);
  return ((unsigned long long)(~asc) << 32) | (uint32_t)i;
}

__global__ __launch_bounds__(SMP_THREADS) void gen_sampled_finish_kernel(SampledArgs a) {
  __shared__ unsigned long long key_s[SMP_MAXOUT];
  __shared__ double cdf_s[SMP_MAXOUT];
  __shared__ float p_s[SMP_MAXOUT];
  __shared__ unsigned char keep_s[SMP_MAXOUT];
  __shared__ float red_s[4];
  __shared__ int cnt_s[4];
  __shared__ int nkeep_s;
  const int t = a.step ? *a.step : 0;
  if (a.step && t >= a.max_steps) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x, O = a.out_dim;
  const float* l = a.logits + (size_t)b * O;
  if (a.logits_out)
    for (int i = tid; i < O; i += SMP_THREADS) a.logits_out[((size_t)t * a.n + b) * O + i] = l[i];
  float T = a.temperature ? a.temperature[b] : 1.f;
  if (!(T >= 0.f) || isinf(T)) T = 1.f;                     // values the host should have rejected count as neutral
  if (a.mode == VQVAE_GEN_SOFTMAX) {
    if (O > SMP_MAXOUT) return;                             // rejected on the host; never index past the LDS arrays
    int k = a.top_k ? a.top_k[b] : 0;
    const float tp = a.top_p ? a.top_p[b] : 1.f;
    if (k <= 0 || k > O) k = O;
    if (T == 0.f) { T = 1.f; k = 1; }                       // greedy: the rank-0 class alone
    const bool nucleus = tp > 0.f && tp < 1.f && k > 1;
    const bool ranked = k < O || nucleus;
    if (ranked) {
      int N2 = 1;
      while (N2 < O) N2 <<= 1;
      for (int i = tid; i < N2; i += SMP_THREADS) key_s[i] = i < O ? smp_key(l[i], i) : ~0ull;
      __syncthreads();
      for (int kk = 2; kk <= N2; kk <<= 1)
        for (int j = kk >> 1; j > 0; j >>= 1) {
          for (int q = tid; q < (N2 >> 1); q += SMP_THREADS) {
            const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1)), p = i | j;
            const unsigned long long x = key_s[i], y = key_s[p];
            if ((x > y) == ((i & kk) == 0)) { key_s[i] = y; key_s[p] = x; }
          }
          __syncthreads();
        }
    }
    for (int i = tid; i < O; i += SMP_THREADS) keep_s[i] = ranked ? 0 : 1;
    __syncthreads();
    if (ranked) {
      for (int r = tid; r < k; r += SMP_THREADS) keep_s[(uint32_t)key_s[r]] = 1;
      __syncthreads();
    }
    // chainer.functions.softmax over the kept classes of l / T: exp(x - max) / sum, fp32, gen_finish_kernel's order
    const float inv = 1.0f / T;
    float m = -INFINITY;
    for (int i = tid; i < O; i += SMP_THREADS) if (keep_s[i]) m = fmaxf(m, l[i] * inv);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if (lane == 0) red_s[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red_s[0], red_s[1]), fmaxf(red_s[2], red_s[3]));
    __syncthreads();
    float s = 0.f;
    for (int i = tid; i < O; i += SMP_THREADS) { const float e = keep_s[i] ? expf(l[i] * inv - m) : 0.f; p_s[i] = e; s += e; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) red_s[wave] = s;
    __syncthreads();
    s = (red_s[0] + red_s[1]) + (red_s[2] + red_s[3]);
    for (int i = tid; i < O; i += SMP_THREADS) p_s[i] = p_s[i] / s;
    __syncthreads();
    if (nucleus) {
      // the shortest rank-order prefix whose float64 mass reaches top_p: one sequential sum, so membership has one answer
      if (tid == 0) {
        double c = 0.0;
        int nk = k;
        for (int r = 0; r < k; ++r) {
          c += (double)p_s[(uint32_t)key_s[r]];
          if (c >= (double)tp) { nk = r + 1; break; }
        }
        nkeep_s = nk;
      }
      __syncthreads();
      for (int r = nkeep_s + tid; r < k; r += SMP_THREADS) p_s[(uint32_t)key_s[r]] = 0.f;
      __syncthreads();
    }
    // numpy.random.choice: float64 cumsum, normalised by its last element,
    // searchsorted(u, side='right') == number of cdf entries <= u   (generate.py:136-138)
    if (tid == 0) {
      double c = 0.0;
      for (int i = 0; i < O; ++i) { c += (double)p_s[i]; cdf_s[i] = c; }
    }
    __syncthreads();
    const double total = cdf_s[O - 1];
    const double u = a.uniforms[((size_t)t * a.n + b) * a.n_uniform];
    int cnt = 0;
    for (int i = tid; i < O; i += SMP_THREADS) cnt += (cdf_s[i] / total <= u) ? 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if (lane == 0) cnt_s[wave] = cnt;
    __syncthreads();
    int idx = cnt_s[0] + cnt_s[1] + cnt_s[2] + cnt_s[3];
    idx = idx < O ? idx : O - 1;
    if (a.probs_out)
      for (int i = tid; i < O; i += SMP_THREADS) a.probs_out[(size_t)b * O + i] = (float)((double)p_s[i] / total);
    if (tid == 0 && a.out) reinterpret_cast<int32_t*>(a.out)[b * a.out_bstride + t] = idx;
    if (a.x_cur) {
      const int nxt = a.forced ? reinterpret_cast<const int32_t*>(a.forced)[(size_t)t * a.n + b] : idx;
      for (int i = tid; i < a.input_dim; i += SMP_THREADS) a.x_cur[(size_t)b * a.input_dim + i] = (i == nxt) ? 1.f : 0.f;  // generate.py:139-141
    }
  } else if (a.mode == VQVAE_GEN_MOL) {
    if (tid == 0) {
      if (T == 0.f) T = 1.f;
      const float inv = 1.0f / T;
      const int nr = O / 3;
      float m = -INFINITY;
      for (int j = 0; j < nr; ++j) m = fmaxf(m, l[j] * inv);
      float s = 0.f;
      for (int j = 0; j < nr; ++j) s += expf(l[j] * inv - m);
      double acc = 0.0;
      for (int j = 0; j < nr; ++j) {
        const float pj = expf(l[j] * inv - m) / s;
        const float sc = expf(fmaxf(l[2 * nr + j], a.log_scale_min)) * T;           // generate.py:111-112, tempered
        const double u = a.uniforms[((size_t)t * a.n + b) * a.n_uniform + j];
        double rv = (double)l[nr + j] + (double)sc * (log(u) - log(1.0 - u));       // generate.py:115-118
        acc += rv * (double)pj;                                                     // generate.py:121-122
      }
      float v = (float)acc;
      v = v / 127.5f;                                                               // generate.py:125
      v = fminf(fmaxf(v, -1.f), 1.f);
      if (a.out) reinterpret_cast<float*>(a.out)[b * a.out_bstride + t] = v;
      if (a.x_cur) {
        const float nxt = a.forced ? reinterpret_cast<const float*>(a.forced)[(size_t)t * a.n + b] : v;
        for (int i = 0; i < a.input_dim; ++i) a.x_cur[(size_t)b * a.input_dim + i] = nxt;   // generate.py:127
      }
    }
  }
}

__global__ __launch_bounds__(64) void gen_sampled_advance_kernel(int* step, int max_steps) {
  const int t = *step;
  if (threadIdx.x == 0 && t < max_steps) *step = t + 1;
}

static bool smp_neutral(const vqvae_gen_sampling* s) { return !s || (!s->temperature && !s->top_k && !s->top_p); }

// The last two launches of a step with controls (called by gen_step_impl and gen_step_lockstep in place of their own
// finish): the descriptor has been validated by then.
int gen_finish_sampled(const vqvae_gen_desc* d, const vqvae_gen_sampling* s, hipStream_t st) {
  VQ_REQUIRE(d->sample_mode != VQVAE_GEN_SOFTMAX || d->out_dim <= SMP_MAXOUT, "gen_step_sampled: at most %d classes", SMP_MAXOUT);
  SampledArgs f{};
  f.logits = d->logits; f.uniforms = d->uniforms; f.forced = d->forced_next; f.out = d->out; f.out_bstride = d->out_bstride;
  f.logits_out = d->logits_out; f.x_cur = d->x_cur; f.step = d->step; f.max_steps = d->max_steps; f.n = d->n;
  f.out_dim = d->out_dim; f.input_dim = d->input_dim; f.mode = d->sample_mode; f.n_uniform = d->n_uniform;
  f.log_scale_min = d->log_scale_min;
  f.temperature = s->temperature; f.top_k = s->top_k; f.top_p = s->top_p;
  hipLaunchKernelGGL(gen_sampled_finish_kernel, dim3(d->n), dim3(SMP_THREADS), 0, st, f);
  VQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(gen_sampled_advance_kernel, dim3(1), dim3(64), 0, st, d->step, d->max_steps);
  VQ_LAUNCH_CHECK();
  return 0;
}

}  // namespace vq

using namespace vq;

extern "C" int vqvae_sampling_abi_version(void) { return 1; }

extern "C" int vqvae_wavenet_gen_step_sampled(const vqvae_gen_desc* d, const vqvae_gen_sampling* s, vqvae_stream_t st) {
  if (smp_neutral(s)) return vqvae_wavenet_gen_step(d, st);
  VQ_REQUIRE(d, "gen_step_sampled: null descriptor");
  VQ_REQUIRE(d->sample_mode == VQVAE_GEN_SOFTMAX || d->sample_mode == VQVAE_GEN_MOL,
             "gen_step_sampled: sampling controls need sample_mode VQVAE_GEN_SOFTMAX or VQVAE_GEN_MOL");
  VQ_REQUIRE(d->sample_mode != VQVAE_GEN_MOL || (!s->top_k && !s->top_p),
             "gen_step_sampled: the mixture of logistics takes a temperature only (top_k and top_p must be NULL)");
  return gen_step_impl(d, s, (hipStream_t)st);
}

extern "C" int vqvae_sample_logits(const float* logits, int n, int out_dim, int mode, float log_scale_min,
                                   const double* uniforms, int n_uniform, const vqvae_gen_sampling* s,
                                   void* out, float* probs_out, vqvae_stream_t st) {
  VQ_REQUIRE(logits && uniforms && out, "sample_logits: null logits, uniforms or out");
  VQ_REQUIRE(n >= 1, "sample_logits: n must be at least 1 (got %d)", n);
  VQ_REQUIRE(out_dim >= 1 && out_dim <= SMP_MAXOUT, "sample_logits: out_dim must be 1..%d (got %d)", SMP_MAXOUT, out_dim);
  VQ_REQUIRE(mode == VQVAE_GEN_SOFTMAX || mode == VQVAE_GEN_MOL, "sample_logits: mode must be VQVAE_GEN_SOFTMAX or VQVAE_GEN_MOL");
  VQ_REQUIRE(n_uniform >= 1, "sample_logits: n_uniform must be at least 1");
  if (mode == VQVAE_GEN_MOL) {
    VQ_REQUIRE(out_dim % 3 == 0 && n_uniform >= out_dim / 3, "sample_logits: mixture sampling needs out_dim = 3*nr_mix and nr_mix uniforms");
    VQ_REQUIRE(!s || (!s->top_k && !s->top_p), "sample_logits: the mixture of logistics takes a temperature only (top_k and top_p must be NULL)");
    VQ_REQUIRE(!probs_out, "sample_logits: probs_out belongs to the softmax output");
  }
  SampledArgs f{};
  f.logits = logits; f.uniforms = uniforms; f.out = out; f.out_bstride = 1; f.probs_out = probs_out;
  f.n = n; f.out_dim = out_dim; f.mode = mode; f.n_uniform = n_uniform; f.log_scale_min = log_scale_min;
  if (s) { f.temperature = s->temperature; f.top_k = s->top_k; f.top_p = s->top_p; }
  hipLaunchKernelGGL(gen_sampled_finish_kernel, dim3(n), dim3(SMP_THREADS), 0, (hipStream_t)st, f);
  VQ_LAUNCH_CHECK();
  return 0;
}
