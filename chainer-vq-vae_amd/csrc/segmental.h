/*
 * segmental.h -- duration-penalised quantisation of a RAGGED list of utterances (csrc/segmental.hip, part of
 * libvqvae_hip.so): the device side of vqvae_amd.segmental (segment_latents, segment_many, ResidentCorpus.segment).  The
 * whole code sequence of an utterance is chosen at once: it minimises the squared distance to the chosen codes plus a
 * penalty for every change of code (the penalised dynamic-programming segmentation of VQ-VAE speech units).
 *
 * The entry points are additive and follow the conventions of include/vqvae_hip.h and the add-on headers: raw device
 * pointers, asynchronous on the given stream, 0 / hipError_t / VQVAE_E_INVALID return codes with
 * vqvae_last_error_string(), arguments validated before anything is launched, a *_workspace_bytes query, writes only
 * inside the outputs and the queried workspace, every address formed in 64 bits.  This header is not under include/ and
 * is in no table of vqvae_amd/_lib.py: vqvae_amd/segmental.py binds it itself and checks vqvae_seg_revision() there.
 *
 * The rule (normative).  Utterance i owns the frames [frame_off[i], frame_off[i + 1]) = T >= 1 frames.  z is (d, stride)
 * float32, channel-major, as the ragged encoder leaves it; W is (k, d) float32; lam is one of n_pen penalties, each a
 * finite double >= 0.  Everything is float64, one rounding per operation, no contraction.
 *   1. Distances.  D[t, c] = sum_j ((double)z[j, t] - (double)W[c, j])^2, j ascending, started from 0.0; each term is one
 *      subtraction, one product and one addition.  A cell's value does not depend on how the table is tiled.
 *   2. Forward.  V[0, c] = D[0, c].  For t >= 1:  m = min_c V[t - 1, c] and a[t - 1] its lowest index;  sw = m + lam;
 *      b[t, c] = (V[t - 1, c] <= sw)  (a tie stays);  V[t, c] = D[t, c] + (b[t, c] ? V[t - 1, c] : sw).
 *      min is the smallest value, then the lowest index: exact in any reduction order, so no tree is prescribed.  The
 *      argmin starts at index 0, so every a lies in [0, k) whatever the inputs.
 *   3. Backward.  c[T - 1] is the lowest argmin of V[T - 1, .] and cost = V[T - 1, c[T - 1]];
 *      c[t - 1] = b[t, c[t]] ? c[t] : a[t - 1];  n_seg = 1 + #{t >= 1 : c[t] != c[t - 1]}.
 * The codes, n_seg and cost of an utterance under a penalty are pure functions of that utterance, W and lam: the same bits
 * alone, in any list, at any position, beside any neighbour, for any split of a list into calls and for any set of other
 * penalties in the call.  Inputs must be finite; with non-finite inputs the codes are unspecified but stay in [0, k), and
 * nothing outside the outputs is written.  No floating-point atomics, no matrix instructions.
 *
 * An utterance whose table entries contradict the descriptor -- frame_off[0] other than 0, frame_off[n] other than ttot,
 * frame_off[i + 1] <= frame_off[i], an end above ttot -- is skipped and marked: n_seg 0, cost NaN, and codes -1 on the
 * frames of [frame_off[i], frame_off[i + 1]) that lie inside [0, ttot).
 */
#ifndef VQVAE_SEGMENTAL_H_
#define VQVAE_SEGMENTAL_H_

#include "../../include/vqvae_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VQVAE_SEG_MAX_K 8192    /* k: 32 codes a lane of the 256-lane DP workgroup keeps in registers */
#define VQVAE_SEG_MAX_PEN 16    /* penalties of one call */
#define VQVAE_SEG_WAVE_K 512    /* k up to here: one wavefront per (utterance, penalty), no barrier; above: 256 lanes */
#define VQVAE_SEG_LANES 256     /* the DP workgroup above VQVAE_SEG_WAVE_K, and the distance kernel's */
#define VQVAE_SEG_TILE 64       /* the distance kernel's tile: 64 frames x 64 codes, 4 x 4 cells a lane */

/* 1 */
int vqvae_seg_revision(void);

typedef struct {
  int32_t n;            /* utterances of this call, >= 1 */
  int32_t d;            /* channels of z and columns of W, >= 1 */
  int32_t k;            /* codes, 1 .. VQVAE_SEG_MAX_K */
  int32_t n_pen;        /* P, 1 .. VQVAE_SEG_MAX_PEN */
  int64_t ttot;         /* frames of this call = frame_off[n], >= n */
  int64_t stride;       /* elements between the channel rows of z, >= ttot */
  int64_t code_stride;  /* elements between the penalties' rows of codes, >= ttot */
  int64_t utt_stride;   /* elements between the penalties' rows of n_seg and cost, >= n */
  double lam[VQVAE_SEG_MAX_PEN];   /* the first n_pen: finite, >= 0; the others are not read */
} vqvae_seg_desc;

/* Bytes of workspace vqvae_seg_segment needs: the table (ttot, k) float64, the stay-words b as the wavefronts' ballots,
 * (n_pen, ttot, ceil(k / 64)) uint64 with code c at bit c % 64 of word c / 64, and a (n_pen, ttot) int32; each of the
 * three pieces starts on a 256-byte boundary and is padded to the next.  (size_t)-1 for a descriptor the entry point
 * would refuse. */
size_t vqvae_seg_workspace_bytes(const vqvae_seg_desc* d);

/* Step 1 alone: z (d, stride) float32 with this call's first frame at z[0], W (k, d) float32; table (ttot, k) float64.
 * n, n_pen, lam, code_stride and utt_stride are validated and otherwise not used.  No workspace. */
int vqvae_seg_distances(const vqvae_seg_desc* d, const float* z, const float* W, double* table, vqvae_stream_t stream);

/* Steps 1 to 3, two launches (the table; then forward and backward, one workgroup per (utterance, penalty)):
 * frame_off (n + 1,) int64 on the device; codes int32, penalty p's frame t at codes[p * code_stride + t]; n_seg int32 and
 * cost float64, penalty p's utterance i at [p * utt_stride + i]. */
int vqvae_seg_segment(const vqvae_seg_desc* d, const float* z, const float* W, const int64_t* frame_off, int32_t* codes,
                      int32_t* n_seg, double* cost, void* workspace, size_t workspace_bytes, vqvae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif  /* VQVAE_SEGMENTAL_H_ */
