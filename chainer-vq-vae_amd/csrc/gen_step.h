// What the step entry points of generation share across generate.hip, generate_lockstep.hip, sampling.hip,
// generate_slots.hip and gen_rng.hip: the functions one file defines and another calls, declared once so that a changed
// signature fails to compile; the per-block check; "are any sampling controls set"; the advance kernels' body.
#ifndef VQ_GEN_STEP_H_
#define VQ_GEN_STEP_H_
#include "common.h"
#include "../../include/vqvae_gen_slots.h"

namespace vq {

struct LsGemmArgs;   // gen_lockstep_body.h
struct LsSlots;

// generate.hip: what every entry point rejects before it launches anything (_rng: d->uniforms may be null); one step
int gen_validate_desc(const vqvae_gen_desc* d);
int gen_validate_desc_rng(const vqvae_gen_desc* d);
int gen_step_impl(const vqvae_gen_desc* d, const vqvae_gen_sampling* smp, hipStream_t st);
// generate_lockstep.hip: the step for more than VQVAE_GEN_MAX_N sequences, and the launch of one of its products
int gen_step_lockstep(const vqvae_gen_desc* d, const vqvae_gen_sampling* smp, hipStream_t st);
int ls_launch(const LsGemmArgs& g, hipStream_t st);
// sampling.hip: the filtered finish and the advance, the last two launches of a step with controls
int gen_finish_sampled(const vqvae_gen_desc* d, const vqvae_gen_sampling* smp, hipStream_t st);
// generate_slots.hip: one tick; `finish` (or nullptr) launches the finishing kernel in place of the tick's own
typedef int (*SlotsFinish)(const vqvae_gen_desc* d, const vqvae_gen_sampling* controls, const LsSlots& p, const void* ctx,
                           hipStream_t st);
int gen_step_slots_impl(const vqvae_gen_desc* d, const vqvae_gen_slots* slots, const vqvae_gen_sampling* s, const char* who,
                        SlotsFinish finish, const void* ctx, hipStream_t st);

// Asked before the first launch of a step, so that nothing is enqueued for a rejected descriptor; `who` names the entry point.
inline int gen_validate_blocks(const vqvae_gen_desc* d, const char* who) {
  for (int l = 0; l < d->n_blocks; ++l) {
    const vqvae_gen_block& bk = d->blocks[l];
    VQ_REQUIRE(bk.conv_W && bk.conv_b && bk.res_W && bk.res_b && bk.skip_W && bk.skip_b && bk.ring && bk.dilation >= 1,
               "%s: block %d incomplete", who, l);
    VQ_REQUIRE(d->cond_dim == 0 || (bk.cond_W && bk.cond_b), "%s: block %d has no condition projection", who, l);
  }
  return 0;
}

inline bool gen_controls_set(const vqvae_gen_sampling* s) { return s && (s->temperature || s->top_k || s->top_p); }

// Every workgroup of a finishing launch reads the step counter, so a launch of its own advances it afterwards.
__device__ inline void gen_advance(int* step, int max_steps) {
  const int t = *step;
  if (threadIdx.x == 0 && t < max_steps) *step = t + 1;
}

}  // namespace vq
#endif  // VQ_GEN_STEP_H_
