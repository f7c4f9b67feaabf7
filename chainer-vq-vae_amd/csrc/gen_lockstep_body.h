// The arithmetic of lockstep generation, shared by its two addressings: the bodies of the GEMM kernel, the finish
// kernel (generate_lockstep.hip) and the filtered sampler (sampling.hip) as device functions, and the launch sequence
// of one step, all templated on a small indexing policy.
//
// A policy answers, for an MFMA column c of a launch: is a sequence there, which one, and at which of ITS steps.
//   LsIdentity (generate_lockstep.hip, sampling.hip): column c < n is sequence c at the global step; the policy's
//     answers are compile-time constants, so these kernels keep their names, their LDS and their instruction mix.
//   LsSlots (generate_slots.hip): column c is a slot of the table of include/vqvae_gen_slots.h; slot_seq[c] < 0 is an
//     idle slot and is treated like a column >= n; the step is the sequence's own slot_t[c]; the global counter is
//     only a tick that indexes the rings.
// What belongs to a sequence (condition, uniforms, forced values, outputs, sampling controls) is addressed by
// (seq, t); what belongs to the machine (state vectors, rings) by the column.  The per-element sequence of
// floating-point operations is the same under both policies, so a sequence's bits do not depend on the policy.
#ifndef VQ_GEN_LOCKSTEP_BODY_H_
#define VQ_GEN_LOCKSTEP_BODY_H_
#include "common.h"
#include "gen_rng.h"
#include "../../include/vqvae_sampling.h"

namespace vq {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int LS_WAVES = 8;                  // K split inside a workgroup
constexpr int LS_THREADS = 64 * LS_WAVES;
constexpr int LS_MAXOUT = 1024;              // categorical sampler: classes held in LDS (generate.hip: GEN_MAXOUT)
constexpr int SMP_MAXOUT = VQVAE_SAMPLING_MAX_CLASSES;
constexpr int SMP_THREADS = 256;

enum { LS_EPI_STACK = 0, LS_EPI_GATE = 1 };

struct LsGemmArgs {
  // A operand.  STACK: virtual row v < rows0 is row v of W0, rows0 <= v < rows0 + rows1 is row v - rows0 of W1.
  // GATE: W0 (2 * rows0, K): tile g holds rows 8g..8g+7 (tanh) and rows0 + 8g.. (sigmoid); rows0 = dilated / 2.
  const float* W0; const float* b0;
  const float* W1; const float* b1;
  const float* Wc; const float* bc;   // condition projection (rows of W0, Cc) or nullptr
  int rows0, rows1, K, Cc;
  // B operand, (n, ldx) row per sequence.  taps == 2: k = 2c + tap meets xa[c] (tap 0, the OLD sample) / xb[c];
  // taps == 1: k meets xa[k].  ring_len > 0: xa is slot t % ring_len of a (ring_len, n, ldx) ring.
  const float* xa; const float* xb;
  int ldx, taps, ring_len, relu_in;
  const float* cond; long cond_bstride, cond_cstride; int cond_step;
  // epilogue
  int epi, relu_out, accum1, n;
  float* out0; const float* add0;     // (n, rows0): out0 = (acc + b0) [relu] + add0; GATE: (n, rows0) gated
  float* out1;                        // (n, rows1): out1 (+)= acc + b1
  const int* step; int max_steps;
  // side duties of the res + skip launch: queue push (modules.py:71-74) and embed-queue shift (247)
  const float* push_src; float* ring; int push_ring_len, push_elems;
  const float* shift_src; float* shift_dst; int shift_elems;
};

// ---- the two policies ----
struct LsCol { bool live; int seq, t; };     // a column of a launch: is a sequence there, which, at which of its steps

struct LsIdentity {
  static constexpr bool kSlots = false;
  __device__ __forceinline__ bool done(int t, int max_steps) const { return t >= max_steps; }
  __device__ __forceinline__ LsCol column(int c, int n) const { return LsCol{c < n, c, 0}; }
  __device__ __forceinline__ int seq_step(const LsCol&, int tick) const { return tick; }
  __device__ __forceinline__ bool aged(const LsCol&, int) const { return true; }      // the rings start as zeros
  __device__ __forceinline__ int n_seq(int n) const { return n; }
  __device__ __forceinline__ bool last(const LsCol&) const { return false; }
  __device__ __forceinline__ float* x_prev_row(int, int) const { return nullptr; }
};

struct LsSlots {
  static constexpr bool kSlots = true;
  const int* slot_seq; const int* slot_t; const int* live_count; const int* steps;
  float* x_prev;
  int nseq;
  __device__ __forceinline__ bool done(int t, int max_steps) const { return t >= max_steps || *live_count == 0; }
  // Two loads that depend on nothing but the column: the kernels ask for them before they test done(), so that the
  // tick, the live count and the table entry are in flight together (loaded one after the other in front of every
  // one of a tick's 62 short launches they cost 5.0 % of the tick, together 2.2 %: profiles/r12_generation_refill.txt).
  __device__ __forceinline__ LsCol column(int c, int n) const {
    LsCol r{false, -1, 0};
    if (c < n) { r.seq = slot_seq[c]; r.t = slot_t[c]; r.live = r.seq >= 0; }
    return r;
  }
  __device__ __forceinline__ int seq_step(const LsCol& c, int) const { return c.t; }
  // ring-age predicate: the entry under tick % ring_len was pushed ring_len ticks ago, by this tenant only if it
  // has run that long; otherwise by the slot's previous tenant (or never) and reads as the 0 of a fresh queue
  __device__ __forceinline__ bool aged(const LsCol& c, int ring_len) const { return c.t >= ring_len; }
  __device__ __forceinline__ int n_seq(int) const { return nseq; }
  __device__ __forceinline__ bool last(const LsCol& c) const { return c.t + 1 >= steps[c.seq]; }   // live columns only
  __device__ __forceinline__ float* x_prev_row(int c, int input_dim) const { return x_prev + (size_t)c * input_dim; }
};

// ---- where the uniform for (t, sq, j) comes from: a second template argument of the two finishing bodies ----
// LsArrayUniforms: the descriptor's (T, n_seq, n_uniform) array; the bodies keep their own load expression for it, so the
//   kernels of generate_lockstep.hip, sampling.hip and generate_slots.hip compile to what they compiled to without it.
// LsPhiloxUniforms (gen_rng.hip): computed by the threads that did the load (include/vqvae_gen_rng.h); ids[sq].
struct LsArrayUniforms { static constexpr bool kArray = true; };

struct LsPhiloxUniforms {
  static constexpr bool kArray = false;
  unsigned long long seed; const unsigned long long* ids;
  int t0;                  // added to t: 0 in a step; the step of vqvae_sample_logits_rng, whose kernel runs at t = 0
  __device__ __forceinline__ double operator()(int t, int sq, int j) const {
    const unsigned long long id = ids ? ids[sq] : (unsigned long long)sq;
    return gen_rng_uniform(seed, id, (uint32_t)(t0 + t), (uint32_t)j);
  }
};

// elements k..k+3 of a row (nullptr: a row / column outside the problem), zero past `lim`
__device__ __forceinline__ float4 ls_load4(const float* p, int k, int lim, bool vec) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (!p) return v;
  if (vec && k + 3 < lim) return *reinterpret_cast<const float4*>(p + k);
  if (k < lim) v.x = p[k];
  if (k + 1 < lim) v.y = p[k + 1];
  if (k + 2 < lim) v.z = p[k + 2];
  if (k + 3 < lim) v.w = p[k + 3];
  return v;
}

__device__ __forceinline__ bool ls_aligned(const void* p, int bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

// One product of a step: a workgroup of LS_THREADS owns a 16-row x 16-column tile and all of K (see generate_lockstep.hip).
template <class P>
__device__ __forceinline__ void ls_gemm_body(const LsGemmArgs& a, const P& pol) {
  __shared__ float part_s[LS_WAVES][256];
  __shared__ float tile_s[16][17];
  const int t = *a.step;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = blockIdx.y * 16 + (lane & 15);               // this lane's column of B
  const int eb = blockIdx.y * 16 + ((tid & 255) >> 4);         // ... and of the epilogue
  const LsCol cs = pol.column(col, a.n), es = pol.column(eb, a.n);
  if (pol.done(t, a.max_steps)) return;
  {
    // side duties, spread over the whole grid (n * residual floats: 256 KiB for the default decoder at n = 128; as one
    // workgroup's loop this was 30 us of a 34 us launch).  Nothing in this launch reads the ring or the older embed slot.
    const int wg = blockIdx.y * gridDim.x + blockIdx.x, stride = gridDim.x * gridDim.y * LS_THREADS;
    if (a.ring) {
      float* dst = a.ring + (size_t)(t % a.push_ring_len) * a.push_elems;
      const int per = P::kSlots ? a.push_elems / a.n : 1;                // an idle slot pushes nothing
      for (int i = wg * LS_THREADS + tid; i < a.push_elems; i += stride)
        if (!P::kSlots || pol.column(i / per, a.n).live) dst[i] = a.push_src[i];
    }
    if (a.shift_dst) {
      const int per = P::kSlots ? a.shift_elems / a.n : 1;
      for (int i = wg * LS_THREADS + tid; i < a.shift_elems; i += stride)
        if (!P::kSlots || pol.column(i / per, a.n).live) a.shift_dst[i] = a.shift_src[i];
    }
  }
  // ---- this lane's row of A and column of B ----
  const int r = lane & 15, kq = 4 * (lane >> 4);
  int wrow = -1;                               // row of W0 (or of W1 when in_w1), -1: outside
  bool in_w1 = false;
  if (a.epi == LS_EPI_GATE) {
    const int j = blockIdx.x * 8 + (r & 7);
    if (j < a.rows0) wrow = j + (r >> 3) * a.rows0;
  } else {
    const int v = blockIdx.x * 16 + r;
    if (v < a.rows0) wrow = v;
    else if (v < a.rows0 + a.rows1) { wrow = v - a.rows0; in_w1 = true; }
  }
  const float* wbase = in_w1 ? a.W1 : a.W0;
  const float* wp = wrow >= 0 ? wbase + (size_t)wrow * a.K : nullptr;
  const float* wcp = (wrow >= 0 && a.Wc) ? a.Wc + (size_t)wrow * a.Cc : nullptr;
  const bool vec_w = (a.K & 3) == 0 && ls_aligned(a.W0, 16) && (!a.W1 || ls_aligned(a.W1, 16));
  const bool vec_wc = (a.Cc & 3) == 0 && ls_aligned(a.Wc, 16);
  const bool col_ok = cs.live;
  // the OLD operand: a ring entry younger than its tenant reads as 0 (always old enough under LsIdentity)
  const bool old_ok = col_ok && (a.ring_len == 0 || pol.aged(cs, a.ring_len));
  const float* xa = a.xa + (a.ring_len > 0 ? (size_t)(t % a.ring_len) * a.n * a.ldx : 0);
  const float* xap = (P::kSlots ? old_ok : col_ok) ? xa + (size_t)col * a.ldx : nullptr;
  const float* xbp = (col_ok && a.taps == 2) ? a.xb + (size_t)col * a.ldx : nullptr;
  const bool vec_x = (a.ldx & 3) == 0 && ls_aligned(xa, 16);
  const float* cp = (col_ok && a.Wc) ? a.cond + (size_t)cs.seq * a.cond_bstride + (a.cond_step ? pol.seq_step(cs, t) : 0) : nullptr;

  const int nch_main = (a.K + 15) >> 4;
  const int nch = nch_main + (a.Wc ? (a.Cc + 15) >> 4 : 0);

  // chunk c: A[row][16c + kq + j], B[16c + kq + j][col] for MFMA step j = 0..3 (lane group kq/4 supplies k = kq + j)
  auto load = [&](int c, float4& av, float4& bv) {
    if (c < nch_main) {
      const int k = 16 * c + kq;
      av = ls_load4(wp, k, a.K, vec_w);
      if (a.taps == 2) {
        const int ch = k >> 1;                 // k is a multiple of 4: channels ch, ch + 1, both taps
        bv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (P::kSlots) {
          if (xbp) {
            if (ch < a.ldx) { if (xap) bv.x = xap[ch]; bv.y = xbp[ch]; }
            if (ch + 1 < a.ldx) { if (xap) bv.z = xap[ch + 1]; bv.w = xbp[ch + 1]; }
          }
        } else if (xap) {
          if (ch < a.ldx) { bv.x = xap[ch]; bv.y = xbp[ch]; }
          if (ch + 1 < a.ldx) { bv.z = xap[ch + 1]; bv.w = xbp[ch + 1]; }
        }
      } else {
        bv = ls_load4(xap, k, a.K, vec_x);
      }
      if (a.relu_in) { bv.x = fmaxf(bv.x, 0.f); bv.y = fmaxf(bv.y, 0.f); bv.z = fmaxf(bv.z, 0.f); bv.w = fmaxf(bv.w, 0.f); }
    } else {
      const int k = 16 * (c - nch_main) + kq;
      av = ls_load4(wcp, k, a.Cc, vec_wc);
      bv = make_float4(0.f, 0.f, 0.f, 0.f);
      if (cp) {
        if (k < a.Cc) bv.x = cp[(size_t)k * a.cond_cstride];
        if (k + 1 < a.Cc) bv.y = cp[(size_t)(k + 1) * a.cond_cstride];
        if (k + 2 < a.Cc) bv.z = cp[(size_t)(k + 2) * a.cond_cstride];
        if (k + 3 < a.Cc) bv.w = cp[(size_t)(k + 3) * a.cond_cstride];
      }
    }
  };

  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  float4 av = make_float4(0.f, 0.f, 0.f, 0.f), bv = av;
  int c = wave;
  if (c < nch) load(c, av, bv);
  for (; c < nch; c += LS_WAVES) {
    float4 an = make_float4(0.f, 0.f, 0.f, 0.f), bn = an;
    if (c + LS_WAVES < nch) load(c + LS_WAVES, an, bn);       // next chunk's loads fly under this chunk's MFMAs
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bv.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bv.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bv.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bv.w, acc, 0, 0, 0);
    av = an; bv = bn;
  }
  // ---- K reduction across the waves, in wave order.  C/D map: col = lane & 15, row = 4 * (lane >> 4) + reg ----
  part_s[wave][lane] = acc[0];
  part_s[wave][64 + lane] = acc[1];
  part_s[wave][128 + lane] = acc[2];
  part_s[wave][192 + lane] = acc[3];
  __syncthreads();
  if (tid < 256) {
    float s = part_s[0][tid];
#pragma unroll
    for (int w = 1; w < LS_WAVES; ++w) s += part_s[w][tid];
    const int reg = tid >> 6, l = tid & 63;
    tile_s[4 * (l >> 4) + reg][l & 15] = s;
  }
  __syncthreads();
  // ---- epilogue: consecutive threads take consecutive rows (contiguous in the (n, rows) state buffers) ----
  if (tid >= 256) return;
  const int er = tid & 15, ec = tid >> 4;
  if (!es.live) return;
  if (a.epi == LS_EPI_GATE) {
    if (er >= 8) return;
    const int j = blockIdx.x * 8 + er;
    if (j >= a.rows0) return;
    float h0 = tile_s[er][ec] + a.b0[j];
    float h1 = tile_s[er + 8][ec] + a.b0[j + a.rows0];
    if (a.Wc) { h0 += a.bc[j]; h1 += a.bc[j + a.rows0]; }
    a.out0[(size_t)eb * a.rows0 + j] = tanhf(h0) * (1.f / (1.f + expf(-h1)));      // modules.py:47-48
  } else {
    const int v = blockIdx.x * 16 + er;
    if (v < a.rows0) {
      float val = tile_s[er][ec] + a.b0[v];
      if (a.relu_out) val = fmaxf(val, 0.f);
      if (a.add0) val += a.add0[(size_t)eb * a.rows0 + v];
      a.out0[(size_t)eb * a.rows0 + v] = val;
    } else if (v < a.rows0 + a.rows1) {
      const int s = v - a.rows0;
      float val = tile_s[er][ec] + a.b1[s];
      if (a.accum1) val = a.out1[(size_t)eb * a.rows1 + s] + val;                  // modules.py:105-109 order
      a.out1[(size_t)eb * a.rows1 + s] = val;
    }
  }
}

// ---- sampling + feedback (generate.py:109-145): gen_finish_kernel's arithmetic, one workgroup per column.
// The step counter is read by every workgroup, so it is advanced by a launch of its own after this one. ----
struct LsFinishArgs {
  const float* logits;      // (n, out_dim)
  const double* uniforms;   // (T, n_seq, n_uniform)
  const void* forced;       // (T, n_seq) int32 / float or nullptr
  void* out;                // int32 index / float value at [seq * out_bstride + t]
  long out_bstride;
  float* logits_out;        // (T, n_seq, out_dim) or nullptr
  float* x_cur;             // (n, input_dim): next input, written in place
  const int* step;
  int max_steps, n, out_dim, input_dim, mode, n_uniform;
  float log_scale_min;
};

// The feedback of a sequence's last step under LsSlots is the fresh embed queue of the slot's next tenant: zeros in
// x_cur and in x_prev (this step's x_prev <- x_cur shift has run in block 0's launch).
template <class P, class U = LsArrayUniforms>
__device__ __forceinline__ void ls_finish_body(const LsFinishArgs& a, const P& pol, const U& uni = U{}) {
  __shared__ float p_s[LS_MAXOUT];
  __shared__ double cdf_s[LS_MAXOUT];
  __shared__ float red_s[4];
  __shared__ int cnt_s[4];
  const int tick = *a.step;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
  const LsCol cs = pol.column(b, a.n);
  if (pol.done(tick, a.max_steps)) return;
  if (P::kSlots && !cs.live) return;
  const int sq = cs.seq, t = pol.seq_step(cs, tick), ns = pol.n_seq(a.n);
  const bool last = pol.last(cs);
  const float* l = a.logits + (size_t)b * a.out_dim;
  if (a.logits_out)
    for (int i = tid; i < a.out_dim; i += 256) a.logits_out[((size_t)t * ns + sq) * a.out_dim + i] = l[i];
  if (a.mode == VQVAE_GEN_SOFTMAX) {
    // chainer.functions.softmax: exp(l - max) / sum, fp32 (generate.py:138)
    float m = -INFINITY;
    for (int i = tid; i < a.out_dim; i += 256) m = fmaxf(m, l[i]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if (lane == 0) red_s[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red_s[0], red_s[1]), fmaxf(red_s[2], red_s[3]));
    __syncthreads();
    float s = 0.f;
    for (int i = tid; i < a.out_dim; i += 256) { const float e = expf(l[i] - m); p_s[i] = e; s += e; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) red_s[wave] = s;
    __syncthreads();
    s = (red_s[0] + red_s[1]) + (red_s[2] + red_s[3]);
    for (int i = tid; i < a.out_dim; i += 256) p_s[i] = p_s[i] / s;
    __syncthreads();
    // numpy.random.choice: float64 cumsum, normalised by its last element,
    // searchsorted(u, side='right') == number of cdf entries <= u   (generate.py:136-138)
    if (tid == 0) {
      double c = 0.0;
      for (int i = 0; i < a.out_dim; ++i) { c += (double)p_s[i]; cdf_s[i] = c; }
    }
    __syncthreads();
    const double total = cdf_s[a.out_dim - 1];
    double u;
    if constexpr (U::kArray) u = a.uniforms[((size_t)t * ns + sq) * a.n_uniform];
    else u = uni(t, sq, 0);
    int cnt = 0;
    for (int i = tid; i < a.out_dim; i += 256) cnt += (cdf_s[i] / total <= u) ? 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if (lane == 0) cnt_s[wave] = cnt;
    __syncthreads();
    int idx = cnt_s[0] + cnt_s[1] + cnt_s[2] + cnt_s[3];
    idx = idx < a.out_dim ? idx : a.out_dim - 1;
    if (tid == 0 && a.out) reinterpret_cast<int32_t*>(a.out)[sq * a.out_bstride + t] = idx;
    const int nxt = a.forced ? reinterpret_cast<const int32_t*>(a.forced)[(size_t)t * ns + sq] : idx;
    if (P::kSlots && last) {
      float* xp = pol.x_prev_row(b, a.input_dim);
      for (int i = tid; i < a.input_dim; i += 256) { a.x_cur[(size_t)b * a.input_dim + i] = 0.f; xp[i] = 0.f; }
    } else {
      for (int i = tid; i < a.input_dim; i += 256) a.x_cur[(size_t)b * a.input_dim + i] = (i == nxt) ? 1.f : 0.f;  // generate.py:139-141
    }
  } else if (a.mode == VQVAE_GEN_MOL) {
    if (tid == 0) {
      const int nr = a.out_dim / 3;
      float m = -INFINITY;
      for (int j = 0; j < nr; ++j) m = fmaxf(m, l[j]);
      float s = 0.f;
      for (int j = 0; j < nr; ++j) s += expf(l[j] - m);
      double acc = 0.0;
      for (int j = 0; j < nr; ++j) {
        const float pj = expf(l[j] - m) / s;
        const float sc = expf(fmaxf(l[2 * nr + j], a.log_scale_min));               // generate.py:111-112
        double u;
        if constexpr (U::kArray) u = a.uniforms[((size_t)t * ns + sq) * a.n_uniform + j];
        else u = uni(t, sq, j);
        double rv = (double)l[nr + j] + (double)sc * (log(u) - log(1.0 - u));       // generate.py:115-118
        acc += rv * (double)pj;                                                     // generate.py:121-122
      }
      float v = (float)acc;
      v = v / 127.5f;                                                               // generate.py:125
      v = fminf(fmaxf(v, -1.f), 1.f);
      if (a.out) reinterpret_cast<float*>(a.out)[sq * a.out_bstride + t] = v;
      const float nxt = a.forced ? reinterpret_cast<const float*>(a.forced)[(size_t)t * ns + sq] : v;
      if (P::kSlots && last) {
        float* xp = pol.x_prev_row(b, a.input_dim);
        for (int i = 0; i < a.input_dim; ++i) { a.x_cur[(size_t)b * a.input_dim + i] = 0.f; xp[i] = 0.f; }
      } else {
        for (int i = 0; i < a.input_dim; ++i) a.x_cur[(size_t)b * a.input_dim + i] = nxt;   // generate.py:127
      }
    }
  }
}

// ---- the filtered sampler (include/vqvae_sampling.h; the steps are listed at the top of sampling.hip) ----
struct SampledArgs {
  const float* logits;      // (n, out_dim)
  const double* uniforms;   // (T, n_seq, n_uniform)
  const void* forced;       // (T, n_seq) int32 / float or nullptr
  void* out;                // int32 index / float value at [seq * out_bstride + t]
  long out_bstride;
  float* logits_out;        // (T, n_seq, out_dim) or nullptr
  float* probs_out;         // (n, out_dim) or nullptr
  float* x_cur;             // (n, input_dim): next input, written in place; nullptr: no feedback
  const int* step;          // nullptr: t = 0 (the sampler alone)
  const float* temperature; // (n_seq,) or nullptr
  const int* top_k;
  const float* top_p;
  int max_steps, n, out_dim, input_dim, mode, n_uniform;
  float log_scale_min;
};

// ascending order of the key = (logit descending, index ascending); -0 ranks with +0
__device__ __forceinline__ unsigned long long smp_key(float v, int i) {
  if (v == 0.f) v = 0.f;
  const uint32_t bits = __float_as_uint(v);
  const uint32_t asc = bits ^ ((bits & 0x80000000u) ? 0xffffffffu : 0x80000000u);
  return ((unsigned long long)(~asc) << 32) | (uint32_t)i;
}

template <class P, class U = LsArrayUniforms>
__device__ __forceinline__ void smp_finish_body(const SampledArgs& a, const P& pol, const U& uni = U{}) {
  __shared__ unsigned long long key_s[SMP_MAXOUT];
  __shared__ double cdf_s[SMP_MAXOUT];
  __shared__ float p_s[SMP_MAXOUT];
  __shared__ unsigned char keep_s[SMP_MAXOUT];
  __shared__ float red_s[4];
  __shared__ int cnt_s[4];
  __shared__ int nkeep_s;
  const int tick = a.step ? *a.step : 0;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x, O = a.out_dim;
  const LsCol cs = pol.column(b, a.n);
  if (a.step && pol.done(tick, a.max_steps)) return;
  if (P::kSlots && !cs.live) return;
  const int sq = cs.seq, t = pol.seq_step(cs, tick), ns = pol.n_seq(a.n);
  const bool last = pol.last(cs);
  const float* l = a.logits + (size_t)b * O;
  if (a.logits_out)
    for (int i = tid; i < O; i += SMP_THREADS) a.logits_out[((size_t)t * ns + sq) * O + i] = l[i];
  float T = a.temperature ? a.temperature[sq] : 1.f;
  if (!(T >= 0.f) || isinf(T)) T = 1.f;                     // values the host should have rejected count as neutral
  if (a.mode == VQVAE_GEN_SOFTMAX) {
    if (O > SMP_MAXOUT) return;                             // rejected on the host; never index past the LDS arrays
    int k = a.top_k ? a.top_k[sq] : 0;
    const float tp = a.top_p ? a.top_p[sq] : 1.f;
    if (k <= 0 || k > O) k = O;
    if (T == 0.f) { T = 1.f; k = 1; }                       // greedy: the rank-0 class alone
    const bool nucleus = tp > 0.f && tp < 1.f && k > 1;
    const bool ranked = k < O || nucleus;
    if (ranked) {
      int N2 = 1;
      while (N2 < O) N2 <<= 1;
      for (int i = tid; i < N2; i += SMP_THREADS) key_s[i] = i < O ? smp_key(l[i], i) : ~0ull;
      __syncthreads();
      for (int kk = 2; kk <= N2; kk <<= 1)
        for (int j = kk >> 1; j > 0; j >>= 1) {
          for (int q = tid; q < (N2 >> 1); q += SMP_THREADS) {
            const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1)), p = i | j;
            const unsigned long long x = key_s[i], y = key_s[p];
            if ((x > y) == ((i & kk) == 0)) { key_s[i] = y; key_s[p] = x; }
          }
          __syncthreads();
        }
    }
    for (int i = tid; i < O; i += SMP_THREADS) keep_s[i] = ranked ? 0 : 1;
    __syncthreads();
    if (ranked) {
      for (int r = tid; r < k; r += SMP_THREADS) keep_s[(uint32_t)key_s[r]] = 1;
      __syncthreads();
    }
    // chainer.functions.softmax over the kept classes of l / T: exp(x - max) / sum, fp32, gen_finish_kernel's order
    const float inv = 1.0f / T;
    float m = -INFINITY;
    for (int i = tid; i < O; i += SMP_THREADS) if (keep_s[i]) m = fmaxf(m, l[i] * inv);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if (lane == 0) red_s[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red_s[0], red_s[1]), fmaxf(red_s[2], red_s[3]));
    __syncthreads();
    float s = 0.f;
    for (int i = tid; i < O; i += SMP_THREADS) { const float e = keep_s[i] ? expf(l[i] * inv - m) : 0.f; p_s[i] = e; s += e; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) red_s[wave] = s;
    __syncthreads();
    s = (red_s[0] + red_s[1]) + (red_s[2] + red_s[3]);
    for (int i = tid; i < O; i += SMP_THREADS) p_s[i] = p_s[i] / s;
    __syncthreads();
    if (nucleus) {
      // the shortest rank-order prefix whose float64 mass reaches top_p: one sequential sum, so membership has one answer
      if (tid == 0) {
        double c = 0.0;
        int nk = k;
        for (int r = 0; r < k; ++r) {
          c += (double)p_s[(uint32_t)key_s[r]];
          if (c >= (double)tp) { nk = r + 1; break; }
        }
        nkeep_s = nk;
      }
      __syncthreads();
      for (int r = nkeep_s + tid; r < k; r += SMP_THREADS) p_s[(uint32_t)key_s[r]] = 0.f;
      __syncthreads();
    }
    // numpy.random.choice: float64 cumsum, normalised by its last element,
    // searchsorted(u, side='right') == number of cdf entries <= u   (generate.py:136-138)
    if (tid == 0) {
      double c = 0.0;
      for (int i = 0; i < O; ++i) { c += (double)p_s[i]; cdf_s[i] = c; }
    }
    __syncthreads();
    const double total = cdf_s[O - 1];
    double u;
    if constexpr (U::kArray) u = a.uniforms[((size_t)t * ns + sq) * a.n_uniform];
    else u = uni(t, sq, 0);
    int cnt = 0;
    for (int i = tid; i < O; i += SMP_THREADS) cnt += (cdf_s[i] / total <= u) ? 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if (lane == 0) cnt_s[wave] = cnt;
    __syncthreads();
    int idx = cnt_s[0] + cnt_s[1] + cnt_s[2] + cnt_s[3];
    idx = idx < O ? idx : O - 1;
    if (a.probs_out)
      for (int i = tid; i < O; i += SMP_THREADS) a.probs_out[(size_t)b * O + i] = (float)((double)p_s[i] / total);
    if (tid == 0 && a.out) reinterpret_cast<int32_t*>(a.out)[sq * a.out_bstride + t] = idx;
    if (a.x_cur) {
      const int nxt = a.forced ? reinterpret_cast<const int32_t*>(a.forced)[(size_t)t * ns + sq] : idx;
      if (P::kSlots && last) {
        float* xp = pol.x_prev_row(b, a.input_dim);
        for (int i = tid; i < a.input_dim; i += SMP_THREADS) { a.x_cur[(size_t)b * a.input_dim + i] = 0.f; xp[i] = 0.f; }
      } else {
        for (int i = tid; i < a.input_dim; i += SMP_THREADS) a.x_cur[(size_t)b * a.input_dim + i] = (i == nxt) ? 1.f : 0.f;  // generate.py:139-141
      }
    }
  } else if (a.mode == VQVAE_GEN_MOL) {
    if (tid == 0) {
      if (T == 0.f) T = 1.f;
      const float inv = 1.0f / T;
      const int nr = O / 3;
      float m = -INFINITY;
      for (int j = 0; j < nr; ++j) m = fmaxf(m, l[j] * inv);
      float s = 0.f;
      for (int j = 0; j < nr; ++j) s += expf(l[j] * inv - m);
      double acc = 0.0;
      for (int j = 0; j < nr; ++j) {
        const float pj = expf(l[j] * inv - m) / s;
        const float sc = expf(fmaxf(l[2 * nr + j], a.log_scale_min)) * T;           // generate.py:111-112, tempered
        double u;
        if constexpr (U::kArray) u = a.uniforms[((size_t)t * ns + sq) * a.n_uniform + j];
        else u = uni(t, sq, j);
        double rv = (double)l[nr + j] + (double)sc * (log(u) - log(1.0 - u));       // generate.py:115-118
        acc += rv * (double)pj;                                                     // generate.py:121-122
      }
      float v = (float)acc;
      v = v / 127.5f;                                                               // generate.py:125
      v = fminf(fmaxf(v, -1.f), 1.f);
      if (a.out) reinterpret_cast<float*>(a.out)[sq * a.out_bstride + t] = v;
      if (a.x_cur) {
        const float nxt = a.forced ? reinterpret_cast<const float*>(a.forced)[(size_t)t * ns + sq] : v;
        if (P::kSlots && last) {
          float* xp = pol.x_prev_row(b, a.input_dim);
          for (int i = 0; i < a.input_dim; ++i) { a.x_cur[(size_t)b * a.input_dim + i] = 0.f; xp[i] = 0.f; }
        } else {
          for (int i = 0; i < a.input_dim; ++i) a.x_cur[(size_t)b * a.input_dim + i] = nxt;   // generate.py:127
        }
      }
    }
  }
}

// ---- host: what is common to the finish launches, and the GEMM launches of one step ----
inline LsFinishArgs ls_finish_args(const vqvae_gen_desc* d) {
  LsFinishArgs f{};
  f.logits = d->logits; f.logits_out = d->logits_out; f.step = d->step; f.max_steps = d->max_steps; f.n = d->n;
  f.out_dim = d->out_dim; f.mode = VQVAE_GEN_NONE;
  if (d->sample_mode != VQVAE_GEN_NONE) {
    f.uniforms = d->uniforms; f.forced = d->forced_next; f.out = d->out; f.out_bstride = d->out_bstride;
    f.x_cur = d->x_cur; f.input_dim = d->input_dim; f.mode = d->sample_mode; f.n_uniform = d->n_uniform;
    f.log_scale_min = d->log_scale_min;
  }
  return f;
}

inline SampledArgs smp_finish_args(const vqvae_gen_desc* d, const vqvae_gen_sampling* s) {
  SampledArgs f{};
  f.logits = d->logits; f.uniforms = d->uniforms; f.forced = d->forced_next; f.out = d->out; f.out_bstride = d->out_bstride;
  f.logits_out = d->logits_out; f.x_cur = d->x_cur; f.step = d->step; f.max_steps = d->max_steps; f.n = d->n;
  f.out_dim = d->out_dim; f.input_dim = d->input_dim; f.mode = d->sample_mode; f.n_uniform = d->n_uniform;
  f.log_scale_min = d->log_scale_min;
  f.temperature = s->temperature; f.top_k = s->top_k; f.top_p = s->top_p;
  return f;
}

// Embed, the residual blocks, proj1, proj2 of one step for 5..VQVAE_GEN_MAX_LOCKSTEP columns, each product launched
// by `launch(args, stream)` (returns 0 or an error code): the logits of the step are in d->logits afterwards.  The
// caller has asked gen_validate_blocks (gen_step.h) about the blocks.
template <class Launch>
int ls_step_products(const vqvae_gen_desc* d, Launch launch, hipStream_t st) {
  const int n = d->n, R = d->residual, half = d->dilated / 2;
  int rc;
  auto base = [&]() {
    LsGemmArgs g{};
    g.n = d->n; g.step = d->step; g.max_steps = d->max_steps; g.taps = 1; g.epi = LS_EPI_STACK;
    return g;
  };

  LsGemmArgs e = base();   // embed: pad-free 2-tap conv on [previous input, current input] (modules.py:234, 247-248)
  e.W0 = d->embed_W; e.b0 = d->embed_b; e.rows0 = R; e.K = 2 * d->input_dim;
  e.xa = d->x_prev; e.xb = d->x_cur; e.ldx = d->input_dim; e.taps = 2; e.out0 = d->h0;
  if ((rc = launch(e, st)) != 0) return rc;

  float* h_in = d->h0;
  float* h_out = d->h1;
  for (int l = 0; l < d->n_blocks; ++l) {
    const vqvae_gen_block& bk = d->blocks[l];
    LsGemmArgs c = base();
    c.epi = LS_EPI_GATE; c.W0 = bk.conv_W; c.b0 = bk.conv_b; c.rows0 = half; c.K = 2 * R;
    if (d->cond_dim) {
      c.Wc = bk.cond_W; c.bc = bk.cond_b; c.Cc = d->cond_dim; c.cond = d->cond;
      c.cond_bstride = d->cond_bstride; c.cond_cstride = d->cond_cstride; c.cond_step = d->cond_follows_step;
    }
    c.xa = bk.ring; c.ring_len = bk.dilation; c.xb = h_in; c.ldx = R; c.taps = 2; c.out0 = d->z;
    if ((rc = launch(c, st)) != 0) return rc;

    LsGemmArgs g = base();
    g.W0 = bk.res_W; g.b0 = bk.res_b; g.rows0 = R; g.add0 = h_in; g.out0 = h_out;                    // modules.py:54
    g.W1 = bk.skip_W; g.b1 = bk.skip_b; g.rows1 = d->skip; g.out1 = d->skip_acc; g.accum1 = l ? 1 : 0;
    g.K = half; g.xa = d->z; g.ldx = half;
    g.push_src = h_in; g.ring = bk.ring; g.push_ring_len = bk.dilation; g.push_elems = n * R;
    if (l == 0) { g.shift_src = d->x_cur; g.shift_dst = d->x_prev; g.shift_elems = n * d->input_dim; }
    if ((rc = launch(g, st)) != 0) return rc;
    float* tmp = h_in; h_in = h_out; h_out = tmp;
  }
  LsGemmArgs p1 = base();
  p1.W0 = d->proj1_W; p1.b0 = d->proj1_b; p1.rows0 = d->skip; p1.K = d->skip; p1.xa = d->skip_acc; p1.ldx = d->skip;
  p1.relu_in = 1; p1.relu_out = 1; p1.out0 = d->s1;
  if ((rc = launch(p1, st)) != 0) return rc;
  LsGemmArgs p2 = base();
  p2.W0 = d->proj2_W; p2.b0 = d->proj2_b; p2.rows0 = d->out_dim; p2.K = d->skip; p2.xa = d->s1; p2.ldx = d->skip;
  p2.out0 = d->logits;
  return launch(p2, st);
}

inline dim3 ls_gemm_grid(const LsGemmArgs& g) {
  return dim3(g.epi == LS_EPI_GATE ? cdiv(g.rows0, 8) : cdiv(g.rows0 + g.rows1, 16), cdiv(g.n, 16));
}

}  // namespace vq
#endif  // VQ_GEN_LOCKSTEP_BODY_H_
