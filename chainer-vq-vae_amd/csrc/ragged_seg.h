// The one segment search of the ragged kernels (ragged_front.hip, audio_metrics.hip, audio_pitch.hip): N segments laid end to end along
// one axis, described by the prefix table off (off[0] = 0, ascending).
#ifndef VQ_RAGGED_SEG_H_
#define VQ_RAGGED_SEG_H_
#include <stdint.h>

namespace vq {

// the segment of position j: the largest i in [0, n) with off[i] <= j
__device__ __forceinline__ int ragged_find_segment(const int64_t* off, int n, long long j) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((long long)off[mid] <= j) lo = mid; else hi = mid - 1;
  }
  return lo;
}

}  // namespace vq

#endif  // VQ_RAGGED_SEG_H_
