/*
 * vqvae_codes.h -- statistics of the discrete codes of a RAGGED list of utterances (csrc/code_stats.hip, part of
 * libvqvae_hip.so): the device side of vqvae_amd.codestats (code_stats, collapse_many, compare_codes_many): runs of equal
 * codes, unigram counts per speaker and bigram counts, and per pair of utterances the frame agreement and the edit
 * distance of the two code strings.
 *
 * The entry points are additive and follow the conventions of include/vqvae_hip.h and the add-on headers: raw
 * device pointers, asynchronous on the given stream, 0 / hipError_t / VQVAE_E_INVALID return codes with
 * vqvae_last_error_string(), arguments validated before anything is launched, writes only inside the outputs
 * and the queried workspace, every address formed in 64 bits.  The header is an entry of the header table of
 * vqvae_amd/_lib.py like every other.
 *
 * The rule (normative).  Everything is integer arithmetic: integer atomics are exact and order-free, so every launch
 * shape gives the same tables, and a pair's or an utterance's results are the same bits alone, in any list and at any
 * position.  A list is described by the device tables start (n,) int64 and len (n,) int32: utterance i is the len[i]
 * int32 codes at codes[start[i]] .. ; the utterances need not touch (the outputs of vqvae_codes_runs are read in place
 * this way).  `total` is the number of elements of the code buffer.
 *   1. Runs.  In utterance i with codes c[0 .. len), a run starts at t = 0 and wherever c[t] != c[t-1]; m[i] is the number
 *      of runs, run r has the code u[r] and the duration dur[r] (the durations of an utterance add up to len).  A run never
 *      continues across an utterance boundary.  The outputs lie at the input's offsets: u and dur of utterance i occupy
 *      [start[i], start[i] + m[i]) of two int32 buffers of `total` elements; the slots behind them are not written.
 *      run_hist (max_run,) int64, nullable, is cleared on the stream and a run of length L adds 1 to bucket
 *      min(L, max_run) - 1.
 *   2. Counts.  Utterance i belongs to group[i] in [0, groups).  uni (groups, k) int64: uni[g, c] counts the positions of
 *      group g that hold code c.  big (k, k) int64, nullable: big[c, c'] counts the transitions c[t] -> c[t+1] inside one
 *      utterance, never across a boundary.  invalid: one int64 counter.  A code outside [0, k) adds 1 to invalid and to
 *      nothing else, and the two transitions it is part of are dropped.  A group outside [0, groups) makes every position
 *      of the utterance add to invalid and to nothing else.  accumulate = 0: the three outputs are cleared on the stream
 *      first; accumulate = 1: the counts are added to what the outputs hold.
 *   3. Frame agreement.  Per pair, overlap = min(len_a, len_b) and agree = #{t < overlap : a[t] == b[t]}.
 *   4. Edit distance, unit costs, on the (La + 1) x (Lb + 1) matrix.  D(i, 0) = i, D(0, j) = j, S = 0 on both borders.
 *      Inside, with ne = (a[i-1] != b[j-1]), the candidates are taken in the order
 *          D(i-1, j-1) + ne   [diagonal],   D(i-1, j) + 1   [step along a],   D(i, j-1) + 1   [step along b];
 *      a later candidate replaces an earlier one only when it is strictly smaller (<): the tie order of vqvae_align.h.
 *      Every cell carries S, the substitutions on its chosen path: the diagonal gives S_prev + ne, the other two steps
 *      S_prev.  dist = D(La, Lb), subs = S(La, Lb).  The host derives dels = (dist - subs + La - Lb) / 2,
 *      ins = (dist - subs - La + Lb) / 2 and matches = La - dels - subs.
 *
 * An utterance or a pair whose table entries contradict the descriptor (a length below 1, codes outside [0, total), a
 * shorter side above max_short) is skipped on the device: m = 0 and nothing else (runs), no count at all (counts),
 * agree = -1 (agreement), dist = -1 and subs = 0 (edit distance).
 *
 * VQVAE_CODES_MAX_SHORT.  vqvae_codes_edit walks the anti-diagonals of the matrix's inside with one workgroup per pair
 * and keeps the current diagonal and the two before it in LDS: (D, S) as two int32, 24 bytes per cell over the three; the
 * borders are closed forms and are not stored.  A diagonal has at most min(La, Lb) cells.  6143 cells take 147432 bytes,
 * within the 144 KiB (147456 bytes) that VQVAE_ALIGN_MAX_SHORT asks of the 160 KiB of a compute unit: 24 s of audio at
 * the default stride of 64 samples per code at 16 kHz on the SHORTER side.  The longer side is free (below 2^30).
 */
#ifndef VQVAE_CODES_H_
#define VQVAE_CODES_H_

#include "vqvae_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VQVAE_CODES_MAX_SHORT 6143     /* min(La, Lb) of a pair: three diagonals of 8-byte cells within 144 KiB of LDS */
#define VQVAE_CODES_THREADS 256        /* every kernel's workgroup: a longer diagonal or utterance is looped over */
#define VQVAE_CODES_MAX_BIGRAM_K 4096  /* k of a call that counts bigrams: the table is 8 k^2 bytes, 128 MiB here */

/* 1; independent of the other versions */
int vqvae_codes_abi_version(void);

typedef struct {
  int32_t n;            /* utterances of this call, >= 1 */
  int32_t max_run;      /* buckets of run_hist, >= 1 */
  int64_t total;        /* elements of codes, u and dur, >= n */
} vqvae_codes_runs_desc;

typedef struct {
  int32_t n;            /* utterances of this call, >= 1 */
  int32_t k;            /* codebook size, >= 1; at most VQVAE_CODES_MAX_BIGRAM_K with bigrams */
  int32_t groups;       /* rows of uni, >= 1 */
  int32_t bigrams;      /* 1: big is counted (and must be given), 0: big must be NULL */
  int32_t accumulate;   /* 0: uni, big and invalid are cleared on the stream first, 1: added to */
  int32_t reserved;     /* 0 */
  int64_t total;        /* elements of codes, >= n */
} vqvae_codes_hist_desc;

typedef struct {
  int32_t n;            /* pairs of this call, >= 1 */
  int32_t max_short;    /* an upper bound of min(La, Lb) over the pairs, 1 .. VQVAE_CODES_MAX_SHORT: sizes the LDS */
  int64_t total_a;      /* elements of side a's code buffer, >= n */
  int64_t total_b;      /* the same for side b */
} vqvae_codes_pair_desc;

typedef struct {        /* device arrays */
  const int64_t* start_a;   /* (n,) first code of every pair on side a */
  const int32_t* len_a;     /* (n,) codes of every pair on side a, >= 1 */
  const int64_t* start_b;   /* (n,) the same on side b */
  const int32_t* len_b;     /* (n,) */
} vqvae_codes_pair_tables;

/* Bytes of workspace of each entry point: none of them keeps anything outside its outputs, so 0; (size_t)-1 for a
 * description the entry point would refuse. */
size_t vqvae_codes_runs_workspace_bytes(const vqvae_codes_runs_desc* d);
size_t vqvae_codes_hist_workspace_bytes(const vqvae_codes_hist_desc* d);
size_t vqvae_codes_agree_workspace_bytes(const vqvae_codes_pair_desc* d);
size_t vqvae_codes_edit_workspace_bytes(const vqvae_codes_pair_desc* d);

/* Step 1, one workgroup per utterance: codes (total,) int32, start (n,) int64, len (n,) int32; u and dur (total,) int32,
 * m (n,) int32, run_hist (max_run,) int64 or NULL (no histogram is kept). */
int vqvae_codes_runs(const vqvae_codes_runs_desc* d, const int32_t* codes, const int64_t* start, const int32_t* len,
                     int32_t* u, int32_t* dur, int32_t* m, int64_t* run_hist, void* ws, size_t ws_bytes,
                     vqvae_stream_t stream);

/* Step 2, one workgroup per utterance: group (n,) int32; uni (groups, k), big (k, k) or NULL, invalid (1,), all int64. */
int vqvae_codes_hist(const vqvae_codes_hist_desc* d, const int32_t* codes, const int64_t* start, const int32_t* len,
                     const int32_t* group, int64_t* uni, int64_t* big, int64_t* invalid, void* ws, size_t ws_bytes,
                     vqvae_stream_t stream);

/* Step 3, one workgroup per pair: agree (n,) int32.  max_short is not looked at beyond the descriptor's own check. */
int vqvae_codes_agree(const vqvae_codes_pair_desc* d, const vqvae_codes_pair_tables* t, const int32_t* a, const int32_t* b,
                      int32_t* agree, void* ws, size_t ws_bytes, vqvae_stream_t stream);

/* Step 4, one workgroup per pair, all pairs in one launch: dist (n,) and subs (n,) int32. */
int vqvae_codes_edit(const vqvae_codes_pair_desc* d, const vqvae_codes_pair_tables* t, const int32_t* a, const int32_t* b,
                     int32_t* dist, int32_t* subs, void* ws, size_t ws_bytes, vqvae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif  /* VQVAE_CODES_H_ */
