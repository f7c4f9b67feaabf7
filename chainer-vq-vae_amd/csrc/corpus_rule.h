// The draw rule of the device-resident corpus (include/vqvae_corpus.h): the shuffled position pi(seed, e, p) and the crop
// offset of draw d.  Plain integer arithmetic on top of gen_rng.h's Philox, the same on the host and on the device, so a
// stand-alone host program can compile these very functions (tests/test_host_resident_corpus.py).
#ifndef VQ_CORPUS_RULE_H_
#define VQ_CORPUS_RULE_H_
#include "gen_rng.h"

namespace vq {

constexpr uint32_t CORPUS_TAG_PERM = 0x50455231u;   // fourth counter word of the permutation's blocks
constexpr uint32_t CORPUS_TAG_CROP = 0x43524F31u;   // ... and of the crop offset's block

// w: max(2, bit_length(n - 1)) rounded up to even; n >= 2
__host__ __device__ __forceinline__ int corpus_width(uint32_t n) {
  int w = 0;
  for (uint32_t v = n - 1; v; v >>= 1) ++w;
  if (w < 2) w = 2;
  return w + (w & 1);
}

// position p of epoch e -> its place q in the epoch's order: a cycle-walking four-round Feistel bijection of [0, n)
__host__ __device__ __forceinline__ uint32_t corpus_pi(uint64_t seed, uint32_t e, uint32_t p, uint32_t n) {
  if (n <= 1) return 0;
  const int w = corpus_width(n), h = w / 2;
  const uint32_t mask = (1u << h) - 1u;
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  uint32_t x = p;
  for (uint64_t walk = 0; walk < (1ull << w); ++walk) {     // a cycle of a permutation of [0, 2^w) is no longer
    uint32_t l = x >> h, r = x & mask;
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
      const uint32_t f = philox4x32_10(r, i, e, CORPUS_TAG_PERM, k0, k1).w[0] & mask;
      const uint32_t nl = r;
      r = l ^ f;
      l = nl;
    }
    x = (l << h) | r;
    if (x < n) return x;
  }
  return p;                                                  // not reached: the cycle of p returns to p < n
}

__host__ __device__ __forceinline__ uint64_t corpus_mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// crop offset of draw d in an utterance of `length` samples: 0 on the padding branch, else uniform in [0, length - L1 - 1]
__host__ __device__ __forceinline__ int64_t corpus_start(uint64_t seed, uint64_t d, int64_t count) {
  if (count <= 0) return 0;
  const Philox4 b = philox4x32_10((uint32_t)d, (uint32_t)(d >> 32), 0u, CORPUS_TAG_CROP, (uint32_t)seed, (uint32_t)(seed >> 32));
  const uint64_t v = ((uint64_t)b.w[0] << 32) | b.w[1];
  return (int64_t)corpus_mulhi64(v, (uint64_t)count);
}

}  // namespace vq
#endif  // VQ_CORPUS_RULE_H_
