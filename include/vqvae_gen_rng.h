/*
 * vqvae_gen_rng.h -- the uniforms of generation drawn on the device (csrc/gen_rng.hip, part of
 * libvqvae_hip.so): uniform number (sequence, step, j) is a pure function of a 64-bit seed, the
 * sequence's 64-bit stream id and two integers, computed by the kernel that consumes it.  Nothing
 * is stored or uploaded, and a sequence's draw is the same in any batch, group, slot or list
 * position.
 *
 * The entry points are additive and sit beside vqvae_hip.h, vqvae_sampling.h, vqvae_gen_slots.h
 * and vqvae_gen_cond.h (same conventions: raw device pointers, asynchronous on the given stream,
 * 0 / hipError_t / VQVAE_E_INVALID return codes with vqvae_last_error_string(), arguments
 * validated before anything is launched, writes only inside the outputs and the state); the other
 * ABIs, their versions, vqvae_gen_desc and their kernels are not touched.  The entry points that
 * take an array of uniforms launch what they launched before.
 *
 * The generator (normative).  Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers:
 * as easy as 1, 2, 3", SC'11).  Multipliers M0 = 0xD2511F53, M1 = 0xCD9E8D57; key increments
 * 0x9E3779B9 (k0) and 0xBB67AE85 (k1).  One round, on 32-bit words:
 *     (c0, c1, c2, c3), (k0, k1) -> (hi(M1*c2) ^ c1 ^ k0, lo(M1*c2), hi(M0*c0) ^ c3 ^ k1, lo(M0*c0))
 * Ten rounds; the key advances by its increments after every round.
 *   Key      (seed & 0xffffffff, seed >> 32).
 *   Counter  (t, j >> 1, id & 0xffffffff, id >> 32): t the sequence's own 0-based step (the index
 *            the kernels read the uniforms array with: the global step in a group launch, slot_t
 *            under refill), id the stream id of the sequence, j the index of the uniform within the
 *            step: 0 for the softmax output, 0..nr_mix-1 for the mixture of logistics.
 *   Double   one block is four words w0..w3; uniform j takes (a, b) = (w[2*(j&1)], w[2*(j&1)+1]) and
 *            is ((a >> 5) * 67108864.0 + (b >> 6)) / 9007199254740992.0: 53 bits in [0, 1), the
 *            construction and range of numpy.random.RandomState.random_sample, so the samplers
 *            meet no value they did not meet before.
 * Known answers (counter ; key -> words):
 *   00000000 00000000 00000000 00000000 ; 00000000 00000000 -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8
 *   243f6a88 85a308d3 13198a2e 03707344 ; a4093822 299f31d0 -> d16cfe09 94fdcceb 5001e420 24126ea1
 * vqvae_amd.DeviceUniforms.host and tests/gen_rng_ref.py restate it in NumPy.
 *
 * `ids` is a device array indexed like the sequence axis of the uniforms array it stands for: by
 * the column in vqvae_gen_rng_fill, vqvae_sample_logits_rng and vqvae_wavenet_gen_step_rng, by the
 * sequence number in vqvae_wavenet_gen_step_slots_rng.  NULL: the index itself is the id.
 */
#ifndef VQVAE_GEN_RNG_H_
#define VQVAE_GEN_RNG_H_

#include "vqvae_gen_slots.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1; independent of the other versions */
int vqvae_gen_rng_abi_version(void);

typedef struct {
  uint64_t        seed;  /* host */
  const uint64_t* ids;   /* device, one stream id per sequence; NULL = the identity */
} vqvae_gen_rng;

/* Writes the uniforms of steps t0 .. t0 + steps - 1 for n sequences as the dense array the other
 * entry points read: out[((s * n + q) * n_uniform) + j] = uniform (ids[q], t0 + s, j), doubles.
 * For the paths that run n <= VQVAE_GEN_MAX_N sequences (the matrix-vector kernels and the
 * persistent kernel), which keep reading an array.  steps == 0 launches nothing.
 * Rejected: a null rng or out, n < 1, n_uniform < 1, t0 < 0, steps < 0, t0 + steps > INT_MAX. */
int vqvae_gen_rng_fill(const vqvae_gen_rng* rng, int t0, int steps, int n, int n_uniform, double* out,
                       vqvae_stream_t stream);

/* vqvae_sample_logits with the uniforms of step `step` drawn on the device: sequence q draws
 * uniform (ids[q], step, j).  Every other argument, the outputs and what is rejected as there
 * (n_uniform: the mixture needs >= out_dim / 3; the softmax output reads j = 0); also rejected: a
 * null rng, step < 0. */
int vqvae_sample_logits_rng(const float* logits, int n, int out_dim, int mode, float log_scale_min,
                            const vqvae_gen_rng* rng, int step, int n_uniform, const vqvae_gen_sampling* s,
                            void* out, float* probs_out, vqvae_stream_t st);

/* vqvae_wavenet_gen_step[_sampled] for d->n = 5..VQVAE_GEN_MAX_LOCKSTEP with the uniforms drawn in
 * the finishing launch: d->uniforms is not read and may be NULL, d->n_uniform still says how many
 * the output takes (>= 1; the mixture needs >= out_dim / 3).  s == NULL or all three NULL: the
 * plain sampler, else the filtered sampler of vqvae_sampling.h.  Capturable into a hipGraph.
 * Rejected besides what those entry points reject: a null rng, d->n <= VQVAE_GEN_MAX_N (fill an
 * array with vqvae_gen_rng_fill and call the array entry points), sample_mode VQVAE_GEN_NONE. */
int vqvae_wavenet_gen_step_rng(const vqvae_gen_desc* d, const vqvae_gen_sampling* s, const vqvae_gen_rng* rng,
                               vqvae_stream_t stream);

/* vqvae_wavenet_gen_step_slots with the uniforms drawn in the finishing launch; ids has
 * slots->n_seq entries.  Rejected besides what it rejects: a null rng, sample_mode VQVAE_GEN_NONE. */
int vqvae_wavenet_gen_step_slots_rng(const vqvae_gen_desc* d, const vqvae_gen_slots* slots, const vqvae_gen_sampling* s,
                                     const vqvae_gen_rng* rng, vqvae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif  /* VQVAE_GEN_RNG_H_ */
