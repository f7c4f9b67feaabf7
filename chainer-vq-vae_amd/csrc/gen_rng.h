// The counter-based uniforms of generation (include/vqvae_gen_rng.h): Philox4x32-10 (Salmon et al., SC'11) and the
// 53-bit double made of two of its words.  Plain 32-bit integer arithmetic, the same on the host and on the device.
#ifndef VQ_GEN_RNG_H_
#define VQ_GEN_RNG_H_
#include <stdint.h>

namespace vq {

struct Philox4 { uint32_t w[4]; };

__host__ __device__ __forceinline__ uint32_t philox_mulhi(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umulhi(a, b);
#else
  return (uint32_t)(((uint64_t)a * b) >> 32);
#endif
}

// counter (c0, c1, c2, c3), key (k0, k1) -> four words; ten rounds, the key advances after every round
__host__ __device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                                          uint32_t k0, uint32_t k1) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = philox_mulhi(M0, c0), l0 = M0 * c0;
    const uint32_t h1 = philox_mulhi(M1, c2), l1 = M1 * c2;
    c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    k0 += W0; k1 += W1;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// two words -> 53 bits in [0, 1): RandomState.random_sample's construction
__host__ __device__ __forceinline__ double gen_rng_double(uint32_t a, uint32_t b) {
  return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) / 9007199254740992.0;
}

// uniform j of step t of the stream `id` under `seed`: key = seed, counter = (t, j >> 1, id), words 2 (j & 1) and + 1
__host__ __device__ __forceinline__ double gen_rng_uniform(uint64_t seed, uint64_t id, uint32_t t, uint32_t j) {
  const Philox4 p = philox4x32_10(t, j >> 1, (uint32_t)id, (uint32_t)(id >> 32), (uint32_t)seed, (uint32_t)(seed >> 32));
  return (j & 1u) ? gen_rng_double(p.w[2], p.w[3]) : gen_rng_double(p.w[0], p.w[1]);   // selects: no indexed registers
}

}  // namespace vq
#endif  // VQ_GEN_RNG_H_
