/*
 * vqvae_corpus.h -- minibatches drawn on the device from a corpus that lives there (csrc/corpus.hip,
 * part of libvqvae_hip.so): the preprocessed (loaded, silence-trimmed, peak-normalised) waveforms
 * of a training set lie end to end in one float32 buffer, and one launch writes a whole minibatch
 * from it: utterance choice (a new shuffled order per epoch), crop offset, zero padding of short
 * utterances (utils.py:67-81 of the reference), mu-law bins and speaker ids.  Row r of batch i is a
 * pure function of (seed, i, r): it resumes exactly, is the same whatever the number of ranks, and
 * a rank draws its rows batch[rank::size] without communication.  Nothing is stored between calls.
 *
 * The entry point is additive and sits beside vqvae_hip.h and the other add-on headers (same
 * conventions as vqvae_gen_rng.h: raw device pointers, asynchronous on the given stream, 0 /
 * hipError_t / VQVAE_E_INVALID return codes with vqvae_last_error_string(), arguments validated
 * before anything is launched, writes only inside the outputs); the other ABIs, their versions and
 * their kernels are not touched.
 *
 * The draw rule (normative).
 * Philox is Philox4x32-10 as vqvae_gen_rng.h defines it (philox4x32_10 of csrc/gen_rng.h).  The key
 * is (seed & 0xffffffff, seed >> 32).  Take n = n_view.
 *   d = iteration * global_batch + global_row (unsigned 64-bit).
 *   e = d div n, p = d mod n.
 *   q = p without `shuffle`, else q = pi(seed, e, p):
 *     n == 1 gives 0.
 *     Else w = max(2, bit_length(n - 1)) rounded up to even, h = w / 2, mask = 2^h - 1.
 *     Starting from x = p, repeat:
 *       (l, r) = (x >> h, x & mask).
 *       Four rounds i = 0..3 of
 *         f = word0(Philox(counter = (r, i, e, 0x50455231))) & mask; (l, r) = (r, l ^ f).
 *       x = (l << h) | r.
 *     Stop when x < n.
 *     This is a cycle-walking Feistel bijection of [0, n).  It stores nothing.  It terminates within
 *     2^w walks because x moves along a cycle of a permutation that contains p < n; the device loop
 *     is bounded by that.
 *   u = view[q], or q when `view` is NULL.
 *   count = length[u] - L1.
 *   start = 0 if count <= 0.  This is the padding branch, utils.py:67-75.
 *   Otherwise start = (v * count) >> 64, with v = (w0 << 32) | w1 of
 *     Philox(counter = (d & 0xffffffff, d >> 32, 0, 0x43524F31)).
 *     That is an integer in [0, len - L1 - 1], the range of utils.py:78.
 *   For i in [0, L1):
 *     x = samples[offset[u] + start + i] if start + i < length[u], else 0.0f.
 *     x_enc[row, i] = x.
 *     bin = #{j : thr[j] <= x}.
 *     x_dec[row, i] = bin for i < L.
 *     t[row, i - 1] = bin for i >= 1.
 *   speaker_out[row] = speaker[u].
 * Here L = L1 - 1, `row` is the local row j of the call and global_row = row0 + row_stride * j.
 *
 * Known answers (computed on the CPU from the Philox restatement, tests/gen_rng_ref.py):
 *   pi, seed 71, n = 5: e = 0 gives [2, 4, 0, 1, 3]; e = 1 gives [1, 0, 3, 2, 4].
 *   pi, seed 71, e = 0, n = 2 gives [1, 0].
 *   pi, seed 2^40 + 3, e = 7, n = 1000, p = 0..5 gives [923, 47, 656, 221, 117, 678].
 *   start, seed 71, count 1000, d = 0..3 gives [555, 6, 920, 140].
 *   start, seed 71, d = 2^32 + 1, count = 2^31 + 5 gives 123133830.
 *   A full plan: lengths [1, 129, 130, 131, 1000], L1 = 130, global batch 4, seed 71, shuffle on.
 *   The (u, start) rows are
 *     iteration 0: (2,0) (4,6) (0,0) (1,0)
 *     iteration 1: (3,0) (1,0) (0,0) (3,0)
 *     iteration 2: (2,0) (4,857) (2,0) (0,0)
 *   Batch 1 of that plan straddles the epoch boundary: its second row is draw 5, which is epoch 1,
 *   position 0.
 * vqvae_amd.corpus.plan_rows and tests/resident_corpus_ref.py restate the rule in Python.
 */
#ifndef VQVAE_CORPUS_H_
#define VQVAE_CORPUS_H_

#include "vqvae_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1; independent of the other versions */
int vqvae_corpus_abi_version(void);

/* The corpus (or a subset of it): every pointer is a device pointer. */
typedef struct {
  const float*   samples;  /* the utterances end to end (ragged), peak-normalised float32 */
  const int64_t* offset;   /* per utterance: its first element in `samples` */
  const int32_t* length;   /* per utterance: its number of samples, >= 1 */
  const int32_t* speaker;  /* per utterance: its speaker id */
  const int32_t* view;     /* n_view utterance numbers (a train or validation subset); NULL = the identity */
  int32_t        n_view;   /* utterances drawn from: entries of `view`, or of the three arrays above when view == NULL */
} vqvae_corpus;

/* Writes local rows 0 .. rows - 1 of global batch `iteration` by the rule above; local row j is
 * global row row0 + row_stride * j (the shard of rank row0 among row_stride ranks).  L = L1 - 1.
 *   x_enc       float32 (rows, L1)
 *   x_dec       int32   (rows, L)
 *   t           int32   (rows, L)
 *   speaker_out int32   (rows,)
 *   utt_out     int32   (rows,)   the utterance u of every row; may be NULL
 *   start_out   int64   (rows,)   its crop offset; may be NULL
 * thresholds: the n_thresholds ascending float32 values vqvae_mulaw_bins takes (1..8192 of them).
 * One launch.  The entries of `view` must be utterance numbers and offset / length must lie inside
 * `samples`: they are device data and are not checked.
 * Rejected: a null corpus, samples, offset, length, speaker, thresholds, x_enc, x_dec, t or
 * speaker_out; rows < 1 or > 65535, L1 < 2 or > 2^30, n_view < 1; global_batch < 1, row0 < 0, row_stride < 1;
 * row0 + row_stride * (rows - 1) >= global_batch; n_thresholds outside 1..8192; an iteration whose
 * draws do not fit 64 bits or whose epoch number does not fit 32 bits. */
int vqvae_corpus_draw(const vqvae_corpus* corpus, uint64_t seed, int shuffle, uint64_t iteration, int global_batch,
                      int row0, int row_stride, int rows, int L1, const float* thresholds, int n_thresholds,
                      float* x_enc, int32_t* x_dec, int32_t* t, int32_t* speaker_out, int32_t* utt_out,
                      int64_t* start_out, vqvae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif  /* VQVAE_CORPUS_H_ */
