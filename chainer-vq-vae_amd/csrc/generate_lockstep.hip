// Lockstep generation of 5..128 sequences per step on the matrix pipe: the per-step kernels of generate.hip with the
// batch in MFMA columns instead of registers.  Same step semantics (WaveNet/modules.py:58-74, 98-110, 232-255;
// generate.py:105-145): the step counter lives in device memory, every kernel reads it and the last one advances it,
// so one launch sequence serves every step and is captured once; rings of `dilation` slots per block; calls past
// max_steps are device no-ops; weights in their Chainer layout, no packing, no workspace.
//
// A step's cost is the weight stream (4 MiB per block of the reference's default decoder) and it does not depend on
// the number of sequences, so N sequences in lockstep turn each matrix-vector product into a GEMM
// [rows x K] . [K x N] on v_mfma_f32_16x16x4_f32 (fp32 in, fp32 accumulate: bit-for-bit a k-ordered fmaf chain).
//
// One kernel does every product of the step (embed, gate, res + skip, proj1, proj2):
//   * a workgroup owns a 16-row x 16-column tile of the result and ALL of K; its LS_WAVES waves take the 16-wide K chunks
//     round-robin (chunk c belongs to wave c % LS_WAVES) and their partial tiles are summed through LDS in wave order.
//     No atomics: an element's value is a fixed sequence of operations on its own row of W and its own column of the
//     batch, so it is the same from run to run and does not depend on n or on which other sequences are present.
//   * the gate's tile holds 8 tanh rows and the 8 sigmoid rows of the same channels, so tanh * sigmoid is the epilogue;
//     the res / skip launch stacks [res_W ; skip_W] into one row space (a tile may straddle the seam).
//   * columns >= n, rows past the matrix and k past K are predicated: never loaded, never stored (operands read as 0).
// Launch shape for the default decoder at n = 128: gate 32 x 8 = 256 workgroups, res + skip 48 x 8 = 384.
// The kernel bodies live in gen_lockstep_body.h, shared with the slot-table form of generate_slots.hip; here they are
// instantiated with the identity policy (column c is sequence c at the global step).
#include "gen_lockstep_body.h"
#include "gen_step.h"

namespace vq {

__global__ __launch_bounds__(LS_THREADS) void gen_lockstep_gemm_kernel(LsGemmArgs a) { ls_gemm_body(a, LsIdentity{}); }

// sampling + feedback (generate.py:109-145), one workgroup per sequence.  The step counter is read by every workgroup,
// so it is advanced by a launch of its own after this one.
__global__ __launch_bounds__(256) void gen_lockstep_finish_kernel(LsFinishArgs a) { ls_finish_body(a, LsIdentity{}); }

__global__ __launch_bounds__(64) void gen_lockstep_advance_kernel(int* step, int max_steps) { gen_advance(step, max_steps); }

int ls_launch(const LsGemmArgs& g, hipStream_t st) {   // also the products of gen_rng.hip's step
  hipLaunchKernelGGL(gen_lockstep_gemm_kernel, ls_gemm_grid(g), dim3(LS_THREADS), 0, st, g);
  VQ_LAUNCH_CHECK();
  return 0;
}

// One step for 5..VQVAE_GEN_MAX_LOCKSTEP sequences; vqvae_wavenet_gen_step (generate.hip) has validated the descriptor's
// dimensions, head weights, state buffers and sampling fields.  smp != nullptr (include/vqvae_sampling.h): the filtered
// sampler of sampling.hip takes the place of the finish and advance launches.
int gen_step_lockstep(const vqvae_gen_desc* d, const vqvae_gen_sampling* smp, hipStream_t st) {
  VQ_REQUIRE(d->n >= 1 && d->n <= VQVAE_GEN_MAX_LOCKSTEP, "gen_step: n must be 1..%d sequences (got %d)", VQVAE_GEN_MAX_LOCKSTEP, d->n);
  VQ_REQUIRE(d->sample_mode != VQVAE_GEN_SOFTMAX || d->out_dim <= LS_MAXOUT, "gen_step: at most %d classes", LS_MAXOUT);
  int rc = gen_validate_blocks(d, "gen_step");
  if (rc != 0 || (rc = ls_step_products(d, ls_launch, st)) != 0) return rc;

  if (smp) return gen_finish_sampled(d, smp, st);
  if (d->sample_mode != VQVAE_GEN_NONE || d->logits_out) {
    hipLaunchKernelGGL(gen_lockstep_finish_kernel, dim3(d->n), dim3(256), 0, st, ls_finish_args(d));
    VQ_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(gen_lockstep_advance_kernel, dim3(1), dim3(64), 0, st, d->step, d->max_steps);
  VQ_LAUNCH_CHECK();
  return 0;
}

}  // namespace vq
