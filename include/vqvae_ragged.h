/*
 * vqvae_ragged.h -- the encoder's and ConditionEmbed's convolutions over a RAGGED batch
 * (csrc/ragged_front.hip, part of libvqvae_hip.so): many utterances of different lengths lie end to
 * end along time with no padding, and one launch per conv stage runs all of them.  With the two small
 * gathers below this is the device side of vqvae_amd.frontend (encode_many, condition_many,
 * frontend_many): waveforms -> latents -> codes -> the latent-rate condition of lockstep generation.
 *
 * The entry points are additive and sit beside vqvae_hip.h and the other add-on headers (raw device
 * pointers, asynchronous on the given stream, 0 / hipError_t / VQVAE_E_INVALID return codes with
 * vqvae_last_error_string(), arguments validated before anything is launched, writes only inside the
 * outputs); the other ABIs, their versions and their kernels are not touched.  Forward only.
 *
 * Layout.  A ragged activation is ONE channel-major (C, Ttot) float32 tensor: channel c of column j at
 * x[c * x_cstride + j].  Segment (utterance) i owns columns [off[i], off[i] + len[i]).  Every stage has
 * its own tables; a stage's lengths follow from the previous stage's by the conv's length rule, for the
 * encoder Tout = (Tin - 2) / 2 + 1 (K = 4, stride 2, pad 1), for the condition convs Tout = Tin.  At the
 * latent rate the tensor is exactly the (B = 1, d, T = Ttot) tensor vqvae_vq_nearest_fwd takes, so the
 * nearest-code search and the gathered e run through that entry point unchanged.
 *
 * The rule (normative).  With jl = j - off_out[i] for output column j of segment i,
 *   y[m, j] = act(bias[m] + sum_{c, k} W[m, c, k] * X(c, stride * jl - pad + k * dil)),
 *   X(c, p) = x[c * x_cstride + off_in[i] + p] if 0 <= p < len_in[i], else 0 -- whatever lies there in
 *   memory: a tap outside its own utterance is never loaded.  The bound is checked per column, so a
 *   column tile may span several segments and a segment many tiles.  act = ReLU when `relu`.
 *
 * Arithmetic (per vqvae_set_matmul_dtype):
 *   0        fp32 operands on v_mfma_f32_32x32x2_f32.
 *   2 and 3  the exact three-way bf16 split of both operands, six products per K step (what the generic
 *            conv runs in mode 2, and in mode 3 below its GFLOP threshold).  Mode 3's float32x2 kernels
 *            are NOT used here on purpose: they scale an operand by a power of two taken from the whole
 *            tensor's absolute maximum, which would make an utterance's result depend on its neighbours.
 *   1        refused (VQVAE_E_INVALID, the message names it).
 *   Cin == 1 (the encoder's first stage) is a memory-bound VALU kernel in every mode: fp32 multiplies
 *            and adds, taps in order k = 0 .. K - 1, then the bias.
 * The result is data-independent and composition-independent: no per-tensor scale, no split-K, one
 * fixed K order per output element (channel groups of 16 ascending, taps ascending inside a group),
 * no floating-point atomics, and out-of-segment taps enter as exact zeros.  An output element is a
 * pure function of its utterance's samples and the weights: the same bits alone, in any list, at any
 * position, in any chunking.
 */
#ifndef VQVAE_RAGGED_H_
#define VQVAE_RAGGED_H_

#include "vqvae_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1; independent of the other versions */
int vqvae_ragged_abi_version(void);

typedef struct {
  int32_t n;            /* segments (utterances), >= 1 */
  int32_t cin, cout;    /* channels in / out, >= 1 */
  int32_t K, stride, pad, dil;   /* (4, 2, 1, 1), or (3, 1, d, d) with d in {1, 2, 4, 8, 16} */
  int32_t relu;         /* != 0: ReLU in the epilogue */
  int32_t blocked_out;  /* 0: y is the ragged (cout, ttot_out) tensor.  != 0: segment i is a row-major
                           (cout, len_out[i]) block at y + cout * off_out[i]: the layout of
                           LatentCondition.local (vqvae_gen_cond.h), written directly */
  int64_t ttot_out;     /* columns of the output, = off_out[n], >= 1 */
  int64_t x_cstride;    /* elements between the channels of x (its Ttot); unused when cin == 1 */
} vqvae_ragged_conv_desc;

/* Bytes of workspace vqvae_ragged_conv_fwd needs for this description: 0 today (a column finds its
 * segment by a search in off_out), queried like every other entry point's so that a later planning
 * pass changes no caller.  (size_t)-1 for a description the entry point would refuse. */
size_t vqvae_ragged_conv_workspace_bytes(const vqvae_ragged_conv_desc* d);

/* One conv stage over all segments, one launch.
 *   x        float32, read at c * x_cstride + off_in[i] + p only for 0 <= p < len_in[i]
 *   off_in   int64 (n,)      first input column of every segment (any order, gaps allowed: a corpus
 *                            buffer is read in place)
 *   len_in   int32 (n,)      input columns of every segment, >= 1
 *   off_out  int64 (n + 1,)  first output column of every segment, ascending from 0, no gaps;
 *                            off_out[n] = ttot_out.  len_out[i] = off_out[i + 1] - off_out[i]
 *   W        float32 (cout, cin, K) (Chainer's (cout, cin, K, 1)),  bias (cout,) or NULL
 *   y        float32, cout * ttot_out elements in either layout
 *   ws       ws_bytes >= the query above (may be NULL when that is 0)
 * The tables are device data and are not checked: off_out must be as described and the input ranges
 * must lie inside x.  Rejected: a null descriptor, x, off_in, len_in, off_out, W or y; n, cin, cout or
 * ttot_out < 1; a (K, stride, pad, dil) outside the two families above; x_cstride < 0; more than
 * 2^31 - 1 column tiles of 64; matmul mode 1; a workspace smaller than the query. */
int vqvae_ragged_conv_fwd(const vqvae_ragged_conv_desc* d, const float* x, const int64_t* off_in,
                          const int32_t* len_in, const int64_t* off_out, const float* W, const float* bias,
                          float* y, void* ws, size_t ws_bytes, vqvae_stream_t stream);

/* The way back from stored codes: e[c, j] = W[idx[j], c] for the ragged (d, ttot) tensor e, W (k, d).
 * An index outside [0, k) gives a column of zeros (the host layer refuses such codes before it calls).
 * Rejected: null idx, W or e; ttot, d or k < 1. */
int vqvae_ragged_code_gather(const int32_t* idx, const float* W, int64_t ttot, int d, int k, float* e,
                             vqvae_stream_t stream);

/* global_vec[i, g] = E[speaker[i], g] for i < n: the speaker embedding rows of LatentCondition.global_vec
 * (n, G), E (n_speaker, G).  A speaker id outside [0, n_speaker) gives a row of zeros.
 * Rejected: null speaker, E or global_vec; n, G or n_speaker < 1. */
int vqvae_ragged_speaker_gather(const int32_t* speaker, const float* E, int n, int G, int n_speaker,
                                float* global_vec, vqvae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif  /* VQVAE_RAGGED_H_ */
