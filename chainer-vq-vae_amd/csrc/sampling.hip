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
// The kernel's body lives in gen_lockstep_body.h, shared with the slot-table form of generate_slots.hip; here it is
// instantiated with the identity policy (workgroup b is sequence b at the global step).
#include "gen_lockstep_body.h"
#include "gen_step.h"

namespace vq {

__global__ __launch_bounds__(SMP_THREADS) void gen_sampled_finish_kernel(SampledArgs a) { smp_finish_body(a, LsIdentity{}); }

__global__ __launch_bounds__(64) void gen_sampled_advance_kernel(int* step, int max_steps) { gen_advance(step, max_steps); }

// The last two launches of a step with controls (called by gen_step_impl and gen_step_lockstep in place of their own
// finish): the descriptor has been validated by then.
int gen_finish_sampled(const vqvae_gen_desc* d, const vqvae_gen_sampling* s, hipStream_t st) {
  VQ_REQUIRE(d->sample_mode != VQVAE_GEN_SOFTMAX || d->out_dim <= SMP_MAXOUT, "gen_step_sampled: at most %d classes", SMP_MAXOUT);
  const SampledArgs f = smp_finish_args(d, s);
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
  if (!gen_controls_set(s)) return vqvae_wavenet_gen_step(d, st);
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
