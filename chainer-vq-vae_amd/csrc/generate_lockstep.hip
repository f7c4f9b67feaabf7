// Lockstep generation of 5..128 sequences per step on the matrix pipe: the per-step kernels of generate.hip with the
// batch in MFMA columns instead of registers.  Same step semantics (WaveNet/modules.py:58-74, 98-110, 232-255;
// generate.py:105-145): the step counter lives in device memory, every kernel reads it and the last one advances it,
// so one launch sequence serves every step and is captured once; rings of `dilation` slots per block; calls past
// max_steps are device no-ops; weights in their Chainer layout, no packing, no workspace.
//
// A step's cost is the weight stream (4 MiB per block of the reference's default decoder) and it does not depend on
// the number of sequences, so N sequences in lockstep turn each matrix-vector product into a GEMM
// [rows x K] . [K x N] on v_mfma_f32_16x16x4_f32 (fp32 in, fp32 accumulate: bit-for-bit a k-ordered fmaf chain).
//
// One kernel does every product of the step (embed, gate, res + skip, proj1, proj2):
//   * a workgroup owns a 16-row x 16-column tile of the result and ALL of K; its LS_WAVES waves take the 16-wide K chunks
//     round-robin (chunk c belongs to wave c % LS_WAVES) and their partial tiles are summed through LDS in wave order.
//     No atomics: an element's value is a fixed sequence of operations on its own row of W and its own column of the
//     batch, so it is the same from run to run and does not depend on n or on which other sequences are present.
//   * the gate's tile holds 8 tanh rows and the 8 sigmoid rows of the same channels, so tanh * sigmoid is the epilogue;
//     the res / skip launch stacks [res_W ; skip_W] into one row space (a tile may straddle the seam).
//   * columns >= n, rows past the matrix and k past K are predicated: never loaded, never stored (operands read as 0).
// Launch shape for the default decoder at n = 128: gate 32 x 8 = 256 workgroups, res + skip 48 x 8 = 384.
#include "common.h"
#include "../../include/vqvae_sampling.h"

namespace vq {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int LS_WAVES = 8;                  // K split inside a workgroup
constexpr int LS_THREADS = 64 * LS_WAVES;
constexpr int LS_MAXOUT = 1024;              // categorical sampler: classes held in LDS (generate.hip: GEN_MAXOUT)

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

__global__ __launch_bounds__(LS_THREADS) void gen_lockstep_gemm_kernel(LsGemmArgs a) {
  __shared__ float part_s[LS_WAVES][256];
  __shared__ float tile_s[16][17];
  const int t = *a.step;
  if (t >= a.max_steps) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  {
    // side duties, spread over the whole grid (n * residual floats: 256 KiB for the default decoder at n = 128; as one
    // workgroup's loop this was 30 us of a 34 us launch).  Nothing in this launch reads the ring or the older embed slot.
    const int wg = blockIdx.y * gridDim.x + blockIdx.x, stride = gridDim.x * gridDim.y * LS_THREADS;
    if (a.ring) {
      float* dst = a.ring + (size_t)(t % a.push_ring_len) * a.push_elems;
      for (int i = wg * LS_THREADS + tid; i < a.push_elems; i += stride) dst[i] = a.push_src[i];
    }
    if (a.shift_dst)
      for (int i = wg * LS_THREADS + tid; i < a.shift_elems; i += stride) a.shift_dst[i] = a.shift_src[i];
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
  const int col = blockIdx.y * 16 + r;
  const bool col_ok = col < a.n;
  const float* xa = a.xa + (a.ring_len > 0 ? (size_t)(t % a.ring_len) * a.n * a.ldx : 0);
  const float* xap = col_ok ? xa + (size_t)col * a.ldx : nullptr;
  const float* xbp = (col_ok && a.taps == 2) ? a.xb + (size_t)col * a.ldx : nullptr;
  const bool vec_x = (a.ldx & 3) == 0 && ls_aligned(xa, 16);
  const float* cp = (col_ok && a.Wc) ? a.cond + (size_t)col * a.cond_bstride + (a.cond_step ? t : 0) : nullptr;

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
        if (xap) {
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
  const int er = tid & 15, eb = blockIdx.y * 16 + (tid >> 4), ec = tid >> 4;
  if (eb >= a.n) return;
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

// ---- sampling + feedback (generate.py:109-145): gen_finish_kernel's arithmetic, one workgroup per sequence.
// The step counter is read by every workgroup, so it is advanced by a launch of its own after this one. ----
struct LsFinishArgs {
  const float* logits;      // (n, out_dim)
  const double* uniforms;   // (T, n, n_uniform)
  const void* forced;       // (T, n) int32 / float or nullptr
  void* out;                // int32 index / float value at [b * out_bstride + t]
  long out_bstride;
  float* logits_out;        // (T, n, out_dim) or nullptr
  float* x_cur;             // (n, input_dim): next input, written in place
  const int* step;
  int max_steps, n, out_dim, input_dim, mode, n_uniform;
  float log_scale_min;
};

__global__ __launch_bounds__(256) void gen_lockstep_finish_kernel(LsFinishArgs a) {
  __shared__ float p_s[LS_MAXOUT];
  __shared__ double cdf_s[LS_MAXOUT];
  __shared__ float red_s[4];
  __shared__ int cnt_s[4];
  const int t = *a.step;
  if (t >= a.max_steps) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
  const float* l = a.logits + (size_t)b * a.out_dim;
  if (a.logits_out)
    for (int i = tid; i < a.out_dim; i += 256) a.logits_out[((size_t)t * a.n + b) * a.out_dim + i] = l[i];
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
    const double u = a.uniforms[((size_t)t * a.n + b) * a.n_uniform];
    int cnt = 0;
    for (int i = tid; i < a.out_dim; i += 256) cnt += (cdf_s[i] / total <= u) ? 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if (lane == 0) cnt_s[wave] = cnt;
    __syncthreads();
    int idx = cnt_s[0] + cnt_s[1] + cnt_s[2] + cnt_s[3];
    idx = idx < a.out_dim ? idx : a.out_dim - 1;
    if (tid == 0 && a.out) reinterpret_cast<int32_t*>(a.out)[b * a.out_bstride + t] = idx;
    const int nxt = a.forced ? reinterpret_cast<const int32_t*>(a.forced)[(size_t)t * a.n + b] : idx;
    for (int i = tid; i < a.input_dim; i += 256) a.x_cur[(size_t)b * a.input_dim + i] = (i == nxt) ? 1.f : 0.f;  // generate.py:139-141
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
        const double u = a.uniforms[((size_t)t * a.n + b) * a.n_uniform + j];
        double rv = (double)l[nr + j] + (double)sc * (log(u) - log(1.0 - u));       // generate.py:115-118
        acc += rv * (double)pj;                                                     // generate.py:121-122
      }
      float v = (float)acc;
      v = v / 127.5f;                                                               // generate.py:125
      v = fminf(fmaxf(v, -1.f), 1.f);
      if (a.out) reinterpret_cast<float*>(a.out)[b * a.out_bstride + t] = v;
      const float nxt = a.forced ? reinterpret_cast<const float*>(a.forced)[(size_t)t * a.n + b] : v;
      for (int i = 0; i < a.input_dim; ++i) a.x_cur[(size_t)b * a.input_dim + i] = nxt;   // generate.py:127
    }
  }
}

__global__ __launch_bounds__(64) void gen_lockstep_advance_kernel(int* step, int max_steps) {
  const int t = *step;
  if (threadIdx.x == 0 && t < max_steps) *step = t + 1;
}

static LsGemmArgs ls_base(const vqvae_gen_desc* d) {
  LsGemmArgs g{};
  g.n = d->n; g.step = d->step; g.max_steps = d->max_steps; g.taps = 1; g.epi = LS_EPI_STACK;
  return g;
}

static int ls_launch(const LsGemmArgs& g, hipStream_t st) {
  const int row_tiles = g.epi == LS_EPI_GATE ? cdiv(g.rows0, 8) : cdiv(g.rows0 + g.rows1, 16);
  hipLaunchKernelGGL(gen_lockstep_gemm_kernel, dim3(row_tiles, cdiv(g.n, 16)), dim3(LS_THREADS), 0, st, g);
  VQ_LAUNCH_CHECK();
  return 0;
}

// One step for 5..VQVAE_GEN_MAX_LOCKSTEP sequences; vqvae_wavenet_gen_step (generate.hip) has validated the descriptor's
// dimensions, head weights, state buffers and sampling fields.  smp != nullptr (include/vqvae_sampling.h): the filtered
// sampler of sampling.hip takes the place of the finish and advance launches.
int gen_finish_sampled(const vqvae_gen_desc* d, const vqvae_gen_sampling* smp, hipStream_t st);
int gen_step_lockstep(const vqvae_gen_desc* d, const vqvae_gen_sampling* smp, hipStream_t st) {
  VQ_REQUIRE(d->n >= 1 && d->n <= VQVAE_GEN_MAX_LOCKSTEP, "gen_step: n must be 1..%d sequences (got %d)", VQVAE_GEN_MAX_LOCKSTEP, d->n);
  VQ_REQUIRE(d->sample_mode != VQVAE_GEN_SOFTMAX || d->out_dim <= LS_MAXOUT, "gen_step: at most %d classes", LS_MAXOUT);
  const int n = d->n, R = d->residual, half = d->dilated / 2;
  int rc;

  LsGemmArgs e = ls_base(d);   // embed: pad-free 2-tap conv on [previous input, current input] (modules.py:234, 247-248)
  e.W0 = d->embed_W; e.b0 = d->embed_b; e.rows0 = R; e.K = 2 * d->input_dim;
  e.xa = d->x_prev; e.xb = d->x_cur; e.ldx = d->input_dim; e.taps = 2; e.out0 = d->h0;
  if ((rc = ls_launch(e, st)) != 0) return rc;

  float* h_in = d->h0;
  float* h_out = d->h1;
  for (int l = 0; l < d->n_blocks; ++l) {
    const vqvae_gen_block& bk = d->blocks[l];
    VQ_REQUIRE(bk.conv_W && bk.conv_b && bk.res_W && bk.res_b && bk.skip_W && bk.skip_b && bk.ring && bk.dilation >= 1,
               "gen_step: block %d incomplete", l);
    VQ_REQUIRE(d->cond_dim == 0 || (bk.cond_W && bk.cond_b), "gen_step: block %d has no condition projection", l);
    LsGemmArgs c = ls_base(d);
    c.epi = LS_EPI_GATE; c.W0 = bk.conv_W; c.b0 = bk.conv_b; c.rows0 = half; c.K = 2 * R;
    if (d->cond_dim) {
      c.Wc = bk.cond_W; c.bc = bk.cond_b; c.Cc = d->cond_dim; c.cond = d->cond;
      c.cond_bstride = d->cond_bstride; c.cond_cstride = d->cond_cstride; c.cond_step = d->cond_follows_step;
    }
    c.xa = bk.ring; c.ring_len = bk.dilation; c.xb = h_in; c.ldx = R; c.taps = 2; c.out0 = d->z;
    if ((rc = ls_launch(c, st)) != 0) return rc;

    LsGemmArgs g = ls_base(d);
    g.W0 = bk.res_W; g.b0 = bk.res_b; g.rows0 = R; g.add0 = h_in; g.out0 = h_out;                    // modules.py:54
    g.W1 = bk.skip_W; g.b1 = bk.skip_b; g.rows1 = d->skip; g.out1 = d->skip_acc; g.accum1 = l ? 1 : 0;
    g.K = half; g.xa = d->z; g.ldx = half;
    g.push_src = h_in; g.ring = bk.ring; g.push_ring_len = bk.dilation; g.push_elems = n * R;
    if (l == 0) { g.shift_src = d->x_cur; g.shift_dst = d->x_prev; g.shift_elems = n * d->input_dim; }
    if ((rc = ls_launch(g, st)) != 0) return rc;
    float* tmp = h_in; h_in = h_out; h_out = tmp;
  }
  LsGemmArgs p1 = ls_base(d);
  p1.W0 = d->proj1_W; p1.b0 = d->proj1_b; p1.rows0 = d->skip; p1.K = d->skip; p1.xa = d->skip_acc; p1.ldx = d->skip;
  p1.relu_in = 1; p1.relu_out = 1; p1.out0 = d->s1;
  if ((rc = ls_launch(p1, st)) != 0) return rc;
  LsGemmArgs p2 = ls_base(d);
  p2.W0 = d->proj2_W; p2.b0 = d->proj2_b; p2.rows0 = d->out_dim; p2.K = d->skip; p2.xa = d->s1; p2.ldx = d->skip;
  p2.out0 = d->logits;
  if ((rc = ls_launch(p2, st)) != 0) return rc;

  if (smp) return gen_finish_sampled(d, smp, st);
  if (d->sample_mode != VQVAE_GEN_NONE) {
    LsFinishArgs f{};
    f.logits = d->logits; f.uniforms = d->uniforms; f.forced = d->forced_next; f.out = d->out; f.out_bstride = d->out_bstride;
    f.logits_out = d->logits_out; f.x_cur = d->x_cur; f.step = d->step; f.max_steps = d->max_steps; f.n = n;
    f.out_dim = d->out_dim; f.input_dim = d->input_dim; f.mode = d->sample_mode; f.n_uniform = d->n_uniform;
    f.log_scale_min = d->log_scale_min;
    hipLaunchKernelGGL(gen_lockstep_finish_kernel, dim3(n), dim3(256), 0, st, f);
    VQ_LAUNCH_CHECK();
  } else if (d->logits_out) {
    LsFinishArgs f{};
    f.logits = d->logits; f.logits_out = d->logits_out; f.step = d->step; f.max_steps = d->max_steps; f.n = n;
    f.out_dim = d->out_dim; f.mode = VQVAE_GEN_NONE;
    hipLaunchKernelGGL(gen_lockstep_finish_kernel, dim3(n), dim3(256), 0, st, f);
    VQ_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(gen_lockstep_advance_kernel, dim3(1), dim3(64), 0, st, d->step, d->max_steps);
  VQ_LAUNCH_CHECK();
  return 0;
}

}  // namespace vq
