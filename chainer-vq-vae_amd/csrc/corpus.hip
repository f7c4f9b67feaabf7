// Minibatches drawn on the device from a corpus that lives there (include/vqvae_corpus.h): one launch per draw writes
// x_enc, the decoder's bin indices, the targets and the speaker ids of a rank's rows of one global batch.
//
// Grid (ceil(L1 / 1024), rows), 256 threads: a workgroup owns 1024 consecutive samples of one row, thread k takes samples
// k, k + 256, k + 512, k + 768 of them, so every load and every store of a wave is to 64 consecutive dwords.
//
// The row's (utterance, start) is derived ONCE per workgroup by lane 0 (corpus_rule.h: at most a few dozen Philox blocks
// for the permutation's walks and one for the crop offset) and handed to the other lanes through LDS, behind the same
// barrier that publishes the thresholds there; the workgroups of a row derive the same pair.  The binning is the
// upper-bound search of mulaw_bins_kernel (misc.hip) over the same thresholds, so the bins are the streaming path's.
//
// offset[u] + start is arbitrary, so the gather is dword loads; every address is formed in 64 bits (a corpus passes 2^31
// elements at 37 hours of 16 kHz audio).  A sample is read only when start + i < length[u]; every store is to
// x_enc[row * L1 + i], x_dec[row * L + i] (i < L), t[row * L + i - 1] (i >= 1) with row < rows and i < L1, and workgroup 0 of
// a row writes speaker_out[row], utt_out[row], start_out[row].  Plain vector stores, no atomics.
#include "common.h"
#include "corpus_rule.h"
#include "../../include/vqvae_corpus.h"

#include <limits.h>

namespace vq {

constexpr int CORPUS_THREADS = 256;
constexpr int CORPUS_SPAN = 1024;            // samples of a row per workgroup
constexpr int CORPUS_MAX_THRESHOLDS = 8192;  // vqvae_mulaw_bins's limit: 32 KB of LDS
constexpr int CORPUS_MAX_L1 = 1 << 30;       // a workgroup's sample numbers stay below 2^31

struct CorpusDrawArgs {
  vqvae_corpus c;
  unsigned long long seed, d0;               // d0: draw number of global row 0 of this batch
  const float* thr;
  float* x_enc;
  int32_t *x_dec, *t, *speaker_out, *utt_out;
  int64_t* start_out;
  int shuffle, row0, row_stride, L1, nthr;
};

__global__ __launch_bounds__(CORPUS_THREADS) void corpus_draw_kernel(CorpusDrawArgs a) {
  extern __shared__ float sthr[];
  __shared__ long long s_base;               // offset[u] + start
  __shared__ int s_avail;                    // samples of the utterance from start on, capped at L1
  const int row = blockIdx.y;
  for (int i = threadIdx.x; i < a.nthr; i += CORPUS_THREADS) sthr[i] = a.thr[i];
  if (threadIdx.x == 0) {
    const uint64_t d = a.d0 + (uint64_t)a.row0 + (uint64_t)a.row_stride * (uint64_t)row;
    const uint32_t n = (uint32_t)a.c.n_view;
    const uint32_t e = (uint32_t)(d / n), p = (uint32_t)(d % n);
    const uint32_t q = a.shuffle ? corpus_pi(a.seed, e, p, n) : p;
    const int u = a.c.view ? a.c.view[q] : (int)q;
    const int len = a.c.length[u];
    const int64_t start = corpus_start(a.seed, d, (int64_t)len - (int64_t)a.L1);
    const int64_t left = (int64_t)len - start;
    s_base = (long long)(a.c.offset[u] + start);
    s_avail = (int)(left < (int64_t)a.L1 ? (left > 0 ? left : 0) : (int64_t)a.L1);
    if (blockIdx.x == 0) {
      a.speaker_out[row] = a.c.speaker[u];
      if (a.utt_out) a.utt_out[row] = u;
      if (a.start_out) a.start_out[row] = start;
    }
  }
  __syncthreads();
  const float* src = a.c.samples + s_base;
  const int avail = s_avail, L1 = a.L1, L = a.L1 - 1, nthr = a.nthr;
  float* xe = a.x_enc + (size_t)row * (size_t)L1;
  int32_t* xd = a.x_dec + (size_t)row * (size_t)L;
  int32_t* tt = a.t + (size_t)row * (size_t)L;
  const int i0 = blockIdx.x * CORPUS_SPAN + threadIdx.x;
#pragma unroll
  for (int k = 0; k < CORPUS_SPAN / CORPUS_THREADS; ++k) {
    const int i = i0 + k * CORPUS_THREADS;
    if (i < L1) {
      const float v = i < avail ? src[i] : 0.0f;
      int lo = 0, hi = nthr;                 // count of thresholds <= v  (upper bound search)
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sthr[mid] <= v) lo = mid + 1; else hi = mid;
      }
      xe[i] = v;
      if (i < L) xd[i] = lo;
      if (i >= 1) tt[i - 1] = lo;
    }
  }
}

}  // namespace vq

using namespace vq;

extern "C" int vqvae_corpus_abi_version(void) { return 1; }

extern "C" int vqvae_corpus_draw(const vqvae_corpus* corpus, uint64_t seed, int shuffle, uint64_t iteration, int global_batch,
                                 int row0, int row_stride, int rows, int L1, const float* thresholds, int n_thresholds,
                                 float* x_enc, int32_t* x_dec, int32_t* t, int32_t* speaker_out, int32_t* utt_out,
                                 int64_t* start_out, vqvae_stream_t stream) {
  VQ_REQUIRE(corpus, "corpus_draw: null corpus");
  VQ_REQUIRE(corpus->samples && corpus->offset && corpus->length && corpus->speaker,
             "corpus_draw: null samples, offset, length or speaker");
  VQ_REQUIRE(thresholds && x_enc && x_dec && t && speaker_out, "corpus_draw: null thresholds, x_enc, x_dec, t or speaker_out");
  VQ_REQUIRE(rows >= 1, "corpus_draw: rows must be at least 1 (got %d)", rows);
  VQ_REQUIRE(rows <= 65535, "corpus_draw: at most 65535 rows per call (got %d)", rows);
  VQ_REQUIRE(L1 >= 2 && L1 <= CORPUS_MAX_L1, "corpus_draw: L1 must be 2..2^30 (got %d)", L1);
  VQ_REQUIRE(corpus->n_view >= 1, "corpus_draw: n_view must be at least 1 (got %d)", (int)corpus->n_view);
  VQ_REQUIRE(global_batch >= 1 && row0 >= 0 && row_stride >= 1,
             "corpus_draw: global_batch >= 1, row0 >= 0, row_stride >= 1 (got %d, %d, %d)", global_batch, row0, row_stride);
  const long long last = (long long)row0 + (long long)row_stride * (long long)(rows - 1);
  VQ_REQUIRE(last < (long long)global_batch, "corpus_draw: row %lld is not a row of a global batch of %d (row0 %d, row_stride %d, rows %d)",
             last, global_batch, row0, row_stride, rows);
  VQ_REQUIRE(n_thresholds >= 1 && n_thresholds <= CORPUS_MAX_THRESHOLDS, "corpus_draw: n_thresholds must be 1..%d (got %d)",
             CORPUS_MAX_THRESHOLDS, n_thresholds);
  VQ_REQUIRE(iteration <= (UINT64_MAX - (uint64_t)last) / (uint64_t)global_batch,
             "corpus_draw: the draws of iteration %llu do not fit 64 bits", (unsigned long long)iteration);
  const uint64_t d_last = iteration * (uint64_t)global_batch + (uint64_t)last;
  VQ_REQUIRE(d_last / (uint64_t)corpus->n_view <= 0xFFFFFFFFull, "corpus_draw: epoch %llu does not fit 32 bits",
             (unsigned long long)(d_last / (uint64_t)corpus->n_view));
  CorpusDrawArgs a{};
  a.c = *corpus;
  a.seed = seed; a.d0 = iteration * (uint64_t)global_batch;
  a.thr = thresholds; a.x_enc = x_enc; a.x_dec = x_dec; a.t = t; a.speaker_out = speaker_out; a.utt_out = utt_out;
  a.start_out = start_out;
  a.shuffle = shuffle ? 1 : 0; a.row0 = row0; a.row_stride = row_stride; a.L1 = L1; a.nthr = n_thresholds;
  const dim3 grid((unsigned)((L1 + CORPUS_SPAN - 1) / CORPUS_SPAN), (unsigned)rows);
  hipLaunchKernelGGL(corpus_draw_kernel, grid, dim3(CORPUS_THREADS), (size_t)n_thresholds * sizeof(float), (hipStream_t)stream, a);
  VQ_LAUNCH_CHECK();
  return 0;
}
