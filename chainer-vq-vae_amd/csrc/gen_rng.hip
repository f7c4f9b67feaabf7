// The uniforms of generation drawn on the device (include/vqvae_gen_rng.h): Philox4x32-10 keyed by a seed, counted by
// (step, j >> 1, stream id), so uniform (sequence, step, j) is a pure function of its name and no (T, N[, nr_mix]) array
// of doubles is drawn, uploaded or stored.
//
// The finishing kernels of lockstep generation are the bodies of gen_lockstep_body.h instantiated a second time with
// LsPhiloxUniforms as their source of uniforms: the one load `uniforms[(t * n_seq + sq) * n_uniform + j]` becomes one
// Philox block (gen_rng.h: ten rounds of two 32 x 32 -> 64 multiplies and three xors, about a hundred integer
// operations) on the threads that did the load; everything else of the kernels, their LDS, their launch shape and the
// order of their floating-point operations is the array form's, so a sequence's sample is the array form's sample for
// the same number.  The instantiations with the array stay in generate_lockstep.hip, sampling.hip and generate_slots.hip
// and are not touched.  The step's products are the GEMM launches of those files.
//
// vqvae_gen_rng_fill writes the same numbers as the dense array for the paths that keep reading one (n <= 4: the
// matrix-vector kernels and the persistent kernel): one thread per Philox block, that is per pair (j, j + 1) of one
// (step, sequence); a grid-stride loop over steps * n * ceil(n_uniform / 2) blocks; every store is to
// out[(s * n + q) * n_uniform + j] with s < steps, q < n, j < n_uniform.  No LDS, no atomics.
#include "gen_lockstep_body.h"
#include "gen_step.h"
#include "../../include/vqvae_gen_rng.h"

#include <limits.h>

namespace vq {

constexpr int RNG_FILL_THREADS = 256;
constexpr int RNG_FILL_MAX_BLOCKS = 4096;

struct RngFillArgs {
  LsPhiloxUniforms u;
  double* out;
  size_t blocks;          // steps * n * pairs
  int t0, n, n_uniform, pairs;
};

__global__ __launch_bounds__(RNG_FILL_THREADS) void gen_rng_fill_kernel(RngFillArgs a) {
  const size_t stride = (size_t)gridDim.x * RNG_FILL_THREADS;
  for (size_t i = (size_t)blockIdx.x * RNG_FILL_THREADS + threadIdx.x; i < a.blocks; i += stride) {
    const size_t row = i / a.pairs;                     // s * n + q
    const int jb = (int)(i - row * a.pairs);
    const int q = (int)(row % a.n);
    const int s = (int)(row / a.n);
    const unsigned long long id = a.u.ids ? a.u.ids[q] : (unsigned long long)q;
    const Philox4 p = philox4x32_10((uint32_t)(a.t0 + s), (uint32_t)jb, (uint32_t)id, (uint32_t)(id >> 32),
                                    (uint32_t)a.u.seed, (uint32_t)(a.u.seed >> 32));
    double* o = a.out + row * a.n_uniform;
    const int j = 2 * jb;
    o[j] = gen_rng_double(p.w[0], p.w[1]);
    if (j + 1 < a.n_uniform) o[j + 1] = gen_rng_double(p.w[2], p.w[3]);
  }
}

// ---- the finishing kernels with the uniform computed inside ----
__global__ __launch_bounds__(256) void gen_rng_lockstep_finish_kernel(LsFinishArgs a, LsPhiloxUniforms u) {
  ls_finish_body(a, LsIdentity{}, u);
}

__global__ __launch_bounds__(SMP_THREADS) void gen_rng_sampled_finish_kernel(SampledArgs a, LsPhiloxUniforms u) {
  smp_finish_body(a, LsIdentity{}, u);
}

__global__ __launch_bounds__(256) void gen_rng_slots_finish_kernel(LsFinishArgs a, LsSlots p, LsPhiloxUniforms u) {
  ls_finish_body(a, p, u);
}

__global__ __launch_bounds__(SMP_THREADS) void gen_rng_slots_sampled_finish_kernel(SampledArgs a, LsSlots p, LsPhiloxUniforms u) {
  smp_finish_body(a, p, u);
}

__global__ __launch_bounds__(64) void gen_rng_advance_kernel(int* step, int max_steps) { gen_advance(step, max_steps); }

static LsPhiloxUniforms philox_of(const vqvae_gen_rng* rng) {
  return LsPhiloxUniforms{(unsigned long long)rng->seed, reinterpret_cast<const unsigned long long*>(rng->ids), 0};
}

static int slots_finish_rng(const vqvae_gen_desc* d, const vqvae_gen_sampling* controls, const LsSlots& p, const void* ctx,
                            hipStream_t st) {
  const LsPhiloxUniforms u = philox_of(static_cast<const vqvae_gen_rng*>(ctx));
  if (controls) {
    VQ_REQUIRE(d->sample_mode != VQVAE_GEN_SOFTMAX || d->out_dim <= SMP_MAXOUT, "gen_step_slots_rng: at most %d classes", SMP_MAXOUT);
    hipLaunchKernelGGL(gen_rng_slots_sampled_finish_kernel, dim3(d->n), dim3(SMP_THREADS), 0, st, smp_finish_args(d, controls), p, u);
  } else {
    hipLaunchKernelGGL(gen_rng_slots_finish_kernel, dim3(d->n), dim3(256), 0, st, ls_finish_args(d), p, u);
  }
  VQ_LAUNCH_CHECK();
  return 0;
}

}  // namespace vq

using namespace vq;

extern "C" int vqvae_gen_rng_abi_version(void) { return 1; }

extern "C" int vqvae_gen_rng_fill(const vqvae_gen_rng* rng, int t0, int steps, int n, int n_uniform, double* out,
                                  vqvae_stream_t stream) {
  VQ_REQUIRE(rng && out, "gen_rng_fill: null rng or out");
  VQ_REQUIRE(n >= 1, "gen_rng_fill: n must be at least 1 (got %d)", n);
  VQ_REQUIRE(n_uniform >= 1, "gen_rng_fill: n_uniform must be at least 1 (got %d)", n_uniform);
  VQ_REQUIRE(t0 >= 0 && steps >= 0 && (long long)t0 + steps <= (long long)INT_MAX,
             "gen_rng_fill: steps t0 .. t0 + steps must be 0..2^31 - 1 (got t0 %d, steps %d)", t0, steps);
  if (steps == 0) return 0;
  RngFillArgs a{};
  a.u = philox_of(rng);
  a.out = out; a.t0 = t0; a.n = n; a.n_uniform = n_uniform; a.pairs = (n_uniform + 1) / 2;
  a.blocks = (size_t)steps * (size_t)n * (size_t)a.pairs;
  const size_t want = (a.blocks + RNG_FILL_THREADS - 1) / RNG_FILL_THREADS;
  const int grid = (int)(want < (size_t)RNG_FILL_MAX_BLOCKS ? want : (size_t)RNG_FILL_MAX_BLOCKS);
  hipLaunchKernelGGL(gen_rng_fill_kernel, dim3(grid), dim3(RNG_FILL_THREADS), 0, (hipStream_t)stream, a);
  VQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int vqvae_sample_logits_rng(const float* logits, int n, int out_dim, int mode, float log_scale_min,
                                       const vqvae_gen_rng* rng, int step, int n_uniform, const vqvae_gen_sampling* s,
                                       void* out, float* probs_out, vqvae_stream_t st) {
  VQ_REQUIRE(logits && rng && out, "sample_logits_rng: null logits, rng or out");
  VQ_REQUIRE(n >= 1, "sample_logits_rng: n must be at least 1 (got %d)", n);
  VQ_REQUIRE(step >= 0, "sample_logits_rng: step must not be negative (got %d)", step);
  VQ_REQUIRE(out_dim >= 1 && out_dim <= SMP_MAXOUT, "sample_logits_rng: out_dim must be 1..%d (got %d)", SMP_MAXOUT, out_dim);
  VQ_REQUIRE(mode == VQVAE_GEN_SOFTMAX || mode == VQVAE_GEN_MOL, "sample_logits_rng: mode must be VQVAE_GEN_SOFTMAX or VQVAE_GEN_MOL");
  VQ_REQUIRE(n_uniform >= 1, "sample_logits_rng: n_uniform must be at least 1");
  if (mode == VQVAE_GEN_MOL) {
    VQ_REQUIRE(out_dim % 3 == 0 && n_uniform >= out_dim / 3, "sample_logits_rng: mixture sampling needs out_dim = 3*nr_mix and nr_mix uniforms");
    VQ_REQUIRE(!s || (!s->top_k && !s->top_p), "sample_logits_rng: the mixture of logistics takes a temperature only (top_k and top_p must be NULL)");
    VQ_REQUIRE(!probs_out, "sample_logits_rng: probs_out belongs to the softmax output");
  }
  SampledArgs f{};      // step == nullptr: the kernel runs at t = 0 and the generator counts from `step`
  f.logits = logits; f.out = out; f.out_bstride = 1; f.probs_out = probs_out;
  f.n = n; f.out_dim = out_dim; f.mode = mode; f.n_uniform = n_uniform; f.log_scale_min = log_scale_min;
  if (s) { f.temperature = s->temperature; f.top_k = s->top_k; f.top_p = s->top_p; }
  LsPhiloxUniforms u = philox_of(rng);
  u.t0 = step;
  hipLaunchKernelGGL(gen_rng_sampled_finish_kernel, dim3(n), dim3(SMP_THREADS), 0, (hipStream_t)st, f, u);
  VQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int vqvae_wavenet_gen_step_rng(const vqvae_gen_desc* d, const vqvae_gen_sampling* s, const vqvae_gen_rng* rng,
                                          vqvae_stream_t stream) {
  VQ_REQUIRE(rng, "gen_step_rng: null rng");
  int bad = gen_validate_desc_rng(d);
  if (bad != 0) return bad;
  VQ_REQUIRE(d->n > VQVAE_GEN_MAX_N, "gen_step_rng: d->n must be %d..%d sequences (got %d); for fewer fill an array with "
             "vqvae_gen_rng_fill", VQVAE_GEN_MAX_N + 1, VQVAE_GEN_MAX_LOCKSTEP, d->n);
  VQ_REQUIRE(d->sample_mode != VQVAE_GEN_NONE, "gen_step_rng: sample_mode VQVAE_GEN_NONE draws nothing: use vqvae_wavenet_gen_step");
  const bool controls = gen_controls_set(s);
  VQ_REQUIRE(!controls || d->sample_mode != VQVAE_GEN_MOL || (!s->top_k && !s->top_p),
             "gen_step_rng: the mixture of logistics takes a temperature only (top_k and top_p must be NULL)");
  VQ_REQUIRE(d->sample_mode != VQVAE_GEN_SOFTMAX || d->out_dim <= (controls ? SMP_MAXOUT : LS_MAXOUT),
             "gen_step_rng: at most %d classes", controls ? SMP_MAXOUT : LS_MAXOUT);
  if ((bad = gen_validate_blocks(d, "gen_step_rng")) != 0) return bad;
  hipStream_t st = (hipStream_t)stream;
  const int rc = ls_step_products(d, ls_launch, st);
  if (rc != 0) return rc;
  const LsPhiloxUniforms u = philox_of(rng);
  if (controls) {
    hipLaunchKernelGGL(gen_rng_sampled_finish_kernel, dim3(d->n), dim3(SMP_THREADS), 0, st, smp_finish_args(d, s), u);
  } else {
    hipLaunchKernelGGL(gen_rng_lockstep_finish_kernel, dim3(d->n), dim3(256), 0, st, ls_finish_args(d), u);
  }
  VQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(gen_rng_advance_kernel, dim3(1), dim3(64), 0, st, d->step, d->max_steps);
  VQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int vqvae_wavenet_gen_step_slots_rng(const vqvae_gen_desc* d, const vqvae_gen_slots* slots,
                                                const vqvae_gen_sampling* s, const vqvae_gen_rng* rng, vqvae_stream_t stream) {
  VQ_REQUIRE(rng, "gen_step_slots_rng: null rng");
  VQ_REQUIRE(!d || d->sample_mode != VQVAE_GEN_NONE, "gen_step_slots_rng: sample_mode VQVAE_GEN_NONE draws nothing: use vqvae_wavenet_gen_step_slots");
  return gen_step_slots_impl(d, slots, s, "gen_step_slots_rng", slots_finish_rng, rng, (hipStream_t)stream);
}
