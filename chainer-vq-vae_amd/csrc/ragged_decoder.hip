// The teacher-forced decoder pass over a ragged list of utterances (include/vqvae_ragged_decoder.h, which states the rule):
// embed by index, the condition projected at the latent rate, per block a gate launch and a res / skip launch, the head
// with the per-column log-sum-exp, and the per-utterance float64 reduce.
//
// rd_gemm_kernel<MODE, T2, EPI> is ragged_conv_kernel's K loop (ragged_front.hip: a workgroup of four waves owns a
//   64 T2 x 64 T2 output tile, a wave a T2 x T2 block of 32 x 32 accumulators; channel groups of 16 ascending, the taps
//   in order inside a group; the NEXT group's words travel in registers while the matrix pipe works on this one's; MODE 0
//   fp32 MFMA, MODE 3 split3 and the six bf16 products of mfma_chain<3>) with one or two taps and four epilogues:
//     RDE_PLAIN    y = act(W f(x) + b), f = ReLU on request; x ragged or LatentCondition.local's blocks: the latent-rate
//                  condition projection of all blocks, and proj1
//     RDE_GATE     two taps (j - d, j), always the 128-row tile: tile rows [0, 64) are tanh rows ch = 64 blockIdx.y + r,
//                  tile rows [64, 128) the sigmoid rows D/2 + ch, so a lane's mi = 0 and mi = 1 accumulators sit at the same
//                  (r, column) and the gate needs no exchange.  The epilogue adds lerp(P)[j] + g[i] and stores z only.
//     RDE_RESSKIP  rows [0, R) from Wr (x' = . + br + x), rows [R, R + S) from Ws (skip = [skip +] . + bs): z is read once
//     RDE_HEAD     always the 64-column tile: the workgroup walks the row tiles of proj2, leaves the column tile's Q logits
//                  in LDS (Q <= 512: 130 KB), then a thread per column runs the two-pass log-sum-exp in ascending class
//                  order, the target gather and the arg-max
//   A thread per column finds the column's segment once (ragged_seg.h) and leaves what the K loop and the epilogue need in
//   LDS.  A tap outside [0, n_i) of its own utterance is a SELECTED zero, never a load.  The order per output element is
//   fixed and the same in every tile position and tile size; there is no split-K, no scale and no atomic.
//   LDS (dynamic): 48 bytes per column + 16 taps x (2 TILE + 1) floats [+ the head's logits]; registers and scratch are
//   held by tests/test_host_ragged_decoder_budget.py.
// rd_embed_kernel, rd_gvec_kernel, rd_reduce_kernel: memory-bound VALU; plain fp32 / fp64 adds in the written order
//   (-ffp-contract=off).
//
// Every address is formed in 64 bits.  Stores go to (row < rows of the output, column < ttot) only; plain vector stores.
#include "gemm_common.h"
#include "ragged_seg.h"
#include "../../include/vqvae_ragged_decoder.h"

namespace vq {

constexpr int RD_TILE = 64;
constexpr int RD_KC = 16;
constexpr int RD_THREADS = 256;
constexpr int RD_WIDE_ROWS = 128;      // from this many output rows on: 128 x 128 tiles (PLAIN, RESSKIP)
enum { RDE_PLAIN = 0, RDE_GATE = 1, RDE_RESSKIP = 2, RDE_HEAD = 3 };

struct RdArgs {
  const float* x;            // the activation the K loop reads
  const int64_t* off;        // (n + 1) column prefix; NULL: the columns are one segment of ttot
  const float *w0, *w1;      // weights, (rows, cin, taps) with w_rs elements between rows; w1: the rows from m_split on
  const float *b0, *b1;
  float *y0, *y1;
  const float* xres;         // RESSKIP: the residual input
  const float *P, *g;        // GATE: this block's rows of P (., tltot) and of g (n, g_stride)
  const int64_t *latoff, *qoff;
  const int32_t *tl, *q;
  float* nll; int32_t* hit; float* logits;
  long long ttot, x_cs, tltot, w_rs, g_stride;
  int n, cin, cout, m_split, dil, upscale, relu_in, relu_out, blocked_in, accumulate;
};

template <int T2, int K>
constexpr size_t rd_lds_bytes(int q_rows) {
  constexpr size_t T = RD_TILE * T2;
  return T * (3 * sizeof(long long) + 6 * sizeof(int)) + (size_t)K * RD_KC * ((T + 1) + T) * sizeof(float) +
         (size_t)q_rows * (T + 1) * sizeof(float);
}

template <int MODE, int T2, int EPI>
__global__ __launch_bounds__(RD_THREADS) void rd_gemm_kernel(RdArgs a) {
  constexpr int K = EPI == RDE_GATE ? 2 : 1;
  constexpr int TILE = RD_TILE * T2;
  constexpr int ROWS = K * RD_KC;
  constexpr int RL = RD_KC * K;                           // floats of one weight row per channel group, contiguous
  constexpr int RP = RD_THREADS / RL;                     // weight rows per pass of the workgroup
  constexpr int NPA = (TILE + RP - 1) / RP;
  constexpr int BSTEP = RD_THREADS / TILE;
  constexpr int NPB = K * RD_KC / BSTEP;
  static_assert(EPI != RDE_GATE || T2 == 2, "the gate pairs tile rows r and 64 + r");
  static_assert(EPI != RDE_HEAD || T2 == 1, "the head keeps 64 columns of logits in LDS");
  extern __shared__ __attribute__((aligned(16))) unsigned char rd_lds[];
  long long* s_base = reinterpret_cast<long long*>(rd_lds);   // [TILE] element of channel 0, position 0 of the column's segment
  long long* s_cs = s_base + TILE;                        // [TILE] elements between the channels
  long long* s_auxl = s_cs + TILE;                        // [TILE] GATE: latoff[i] + v0
  int* s_pos0 = reinterpret_cast<int*>(s_auxl + TILE);    // [TILE] position of tap 0
  int* s_len = s_pos0 + TILE;                             // [TILE] length of the segment; 0 for a column past the end
  int* s_i0 = s_len + TILE;                               // [TILE] GATE: v1 - v0; HEAD: the target class
  int* s_i1 = s_i0 + TILE;                                // [TILE] GATE: the segment
  float* s_f0 = reinterpret_cast<float*>(s_i1 + TILE);    // [TILE] GATE: w0
  float* s_f1 = s_f0 + TILE;                              // [TILE] GATE: w1
  float (*sA)[TILE + 1] = reinterpret_cast<float (*)[TILE + 1]>(s_f1 + TILE);       // [tap * 16 + channel][row]
  float (*sB)[TILE] = reinterpret_cast<float (*)[TILE]>(&sA[ROWS][0]);              // [tap * 16 + channel][column]
  float (*s_out)[TILE + 1] = reinterpret_cast<float (*)[TILE + 1]>(&sB[ROWS][0]);   // HEAD: [class][column]

  const int tid = threadIdx.x;
  const long long t0 = (long long)blockIdx.x * TILE;

  if (tid < TILE) {
    const long long j = t0 + tid;
    long long base = 0, cs = 0, auxl = 0;
    int pos0 = 0, len = 0, i0 = 0, i1 = 0;
    float f0 = 0.f, f1 = 0.f;
    if (j < a.ttot) {
      int i = 0;
      long long o = 0, ln = a.ttot;
      if (a.off) {
        i = ragged_find_segment(a.off, a.n, j);
        o = (long long)a.off[i];
        ln = (long long)a.off[i + 1] - o;
      }
      const long long jl = j - o;
      len = (int)ln;
      pos0 = (int)jl - (K - 1) * a.dil;
      if (a.blocked_in) { base = (long long)a.cin * o; cs = ln; }
      else { base = o; cs = a.x_cs; }
      if constexpr (EPI == RDE_GATE) {
        const int tl = a.tl[i];
        const long long Tq = (long long)a.upscale * tl;
        int v0 = 0, step = 0;
        f0 = 0.f; f1 = 1.f;
        if (tl > 1) {                                      // (v0, w0, w1) of include/vqvae_gen_cond.h
          double v = (double)jl * ((double)(tl - 1) / (double)(Tq - 1));
          if (jl == Tq - 1) v = (double)(tl - 1);
          int f = (int)floor(v);
          f = f < 0 ? 0 : (f > tl - 2 ? tl - 2 : f);
          v0 = f; step = 1;
          f0 = (float)((double)(f + 1) - v);
          f1 = (float)(v - (double)f);
        }
        auxl = (long long)a.latoff[i] + v0;
        i0 = step; i1 = i;
      }
      if constexpr (EPI == RDE_HEAD) i0 = a.q[(long long)a.qoff[i] + jl + 1];
    }
    s_base[tid] = base; s_cs[tid] = cs; s_auxl[tid] = auxl; s_pos0[tid] = pos0; s_len[tid] = len;
    s_i0[tid] = i0; s_i1[tid] = i1; s_f0[tid] = f0; s_f1[tid] = f1;
  }
  __syncthreads();

  const bool a_act = tid < RP * RL;
  const int a_row = tid / RL, a_r = tid - a_row * RL;
  const int a_c = a_r / K, a_k = a_r - a_c * K;
  const int b_col = tid & (TILE - 1), b_kc0 = tid / TILE;
  const int b_pos0 = s_pos0[b_col], b_len = s_len[b_col];
  const long long b_cs = s_cs[b_col];
  const float* b_src = a.x + s_base[b_col];
  const int wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1;
  const int lr = lane & 31, lh = lane >> 5;
  const int Ch = a.cout >> 1;                              // GATE: rows of one half

  const int n_mt = EPI == RDE_HEAD ? (a.cout + TILE - 1) / TILE : 1;
  for (int mt = 0; mt < n_mt; ++mt) {
    const int m0 = EPI == RDE_HEAD ? mt * TILE : (EPI == RDE_GATE ? (int)blockIdx.y * RD_TILE : (int)blockIdx.y * TILE);
    // where the weight rows this thread stages start (elements from w0 / w1; -1: a row outside the output)
    int wofs[NPA];
    unsigned wsel = 0;
#pragma unroll
    for (int p = 0; p < NPA; ++p) {
      const int m = p * RP + a_row;
      int ofs = -1;
      if (a_act && m < TILE) {
        if constexpr (EPI == RDE_GATE) {
          const int ch = m0 + (m & (RD_TILE - 1));
          if (ch < Ch) ofs = (int)(((m >> 6) * Ch + ch) * a.w_rs);
        } else if constexpr (EPI == RDE_RESSKIP) {
          const int gm = m0 + m;
          if (gm < a.m_split) ofs = (int)(gm * a.w_rs);
          else if (gm < a.cout) { ofs = (int)((gm - a.m_split) * a.w_rs); wsel |= 1u << p; }
        } else {
          if (m0 + m < a.cout) ofs = (int)((m0 + m) * a.w_rs);
        }
      }
      wofs[p] = ofs;
    }
    float ra[NPA], rb[NPB];
    auto fetch = [&](const int c0) {
#pragma unroll
      for (int p = 0; p < NPA; ++p) {
        const bool ok = wofs[p] >= 0 && c0 + a_c < a.cin;
        const float* wb = (EPI == RDE_RESSKIP && ((wsel >> p) & 1u)) ? a.w1 : a.w0;
        ra[p] = ok ? wb[(long long)wofs[p] + c0 * K + a_r] : 0.f;
      }
#pragma unroll
      for (int p = 0; p < NPB; ++p) {
        const int kc = b_kc0 + p * BSTEP;                  // tap * 16 + channel
        const int k = kc >> 4, ch = c0 + (kc & (RD_KC - 1));
        const int pos = b_pos0 + k * a.dil;
        const bool ok = pos >= 0 && pos < b_len && ch < a.cin;      // a tap outside its own utterance is a selected zero, never a load
        float v = ok ? b_src[(long long)ch * b_cs + pos] : 0.f;
        if (a.relu_in) v = fmaxf(v, 0.f);
        rb[p] = v;
      }
    };
    fetch(0);

    f32x16 acc[T2][T2];
#pragma unroll
    for (int mi = 0; mi < T2; ++mi)
#pragma unroll
      for (int ni = 0; ni < T2; ++ni)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

    for (int c0 = 0; c0 < a.cin; c0 += RD_KC) {
      if (c0 || mt) __syncthreads();                       // the previous group's fragments are read
#pragma unroll
      for (int p = 0; p < NPA; ++p) {
        const int m = p * RP + a_row;
        if (a_act && m < TILE) sA[a_k * RD_KC + a_c][m] = ra[p];
      }
#pragma unroll
      for (int p = 0; p < NPB; ++p) sB[b_kc0 + p * BSTEP][b_col] = rb[p];
      __syncthreads();
      if (c0 + RD_KC < a.cin) fetch(c0 + RD_KC);
#pragma unroll
      for (int k = 0; k < K; ++k) {
        if constexpr (MODE == 0) {
#pragma unroll
          for (int s = 0; s < RD_KC / 2; ++s) {
            float av[T2], bv[T2];
#pragma unroll
            for (int q = 0; q < T2; ++q) {
              av[q] = sA[k * RD_KC + 2 * s + lh][wm * 32 + q * 64 + lr];
              bv[q] = sB[k * RD_KC + 2 * s + lh][wn * 32 + q * 64 + lr];
            }
#pragma unroll
            for (int mi = 0; mi < T2; ++mi)
#pragma unroll
              for (int ni = 0; ni < T2; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[mi], bv[ni], acc[mi][ni], 0, 0, 0);
          }
        } else {
          uint4 af[T2][3], bf[T2][3];
#pragma unroll
          for (int t = 0; t < T2; ++t) {
            float av[8], bv[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
              av[q] = sA[k * RD_KC + 8 * lh + q][wm * 32 + t * 64 + lr];
              bv[q] = sB[k * RD_KC + 8 * lh + q][wn * 32 + t * 64 + lr];
            }
            unsigned ap[3][4], bp[3][4];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
              split3(av[2 * p], av[2 * p + 1], ap[0][p], ap[1][p], ap[2][p]);
              split3(bv[2 * p], bv[2 * p + 1], bp[0][p], bp[1][p], bp[2][p]);
            }
#pragma unroll
            for (int q = 0; q < 3; ++q) {
              af[t][q] = make_uint4(ap[q][0], ap[q][1], ap[q][2], ap[q][3]);
              bf[t][q] = make_uint4(bp[q][0], bp[q][1], bp[q][2], bp[q][3]);
            }
          }
#pragma unroll
          for (int mi = 0; mi < T2; ++mi)
#pragma unroll
            for (int ni = 0; ni < T2; ++ni) acc[mi][ni] = mfma_chain<3>(af[mi], bf[ni], acc[mi][ni]);
        }
      }
    }

    // epilogue.  C/D layout of the 32 x 32 tiles: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    if constexpr (EPI == RDE_GATE) {
#pragma unroll
      for (int ni = 0; ni < T2; ++ni) {
        const int cl = wn * 32 + ni * 64 + lr;
        const long long j = t0 + cl;
        if (j >= a.ttot) continue;
        const long long pv = s_auxl[cl];
        const int step = s_i0[cl];
        const float w0 = s_f0[cl], w1 = s_f1[cl];
        const float* gi = a.g + (long long)s_i1[cl] * a.g_stride;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ch = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
          if (ch < Ch) {
            float h[2];
#pragma unroll
            for (int half = 0; half < 2; ++half) {
              const int m = half * Ch + ch;
              const float* pr = a.P + (long long)m * a.tltot + pv;
              const float c = (w0 * pr[0] + w1 * pr[step]) + gi[m];
              h[half] = acc[half][ni][r] + c;
            }
            a.y0[(long long)ch * a.ttot + j] = tanhf(h[0]) * (1.f / (1.f + expf(-h[1])));
          }
        }
      }
    } else {
#pragma unroll
      for (int ni = 0; ni < T2; ++ni) {
        const int cl = wn * 32 + ni * 64 + lr;
        const long long j = t0 + cl;
        const bool col_ok = j < a.ttot;
#pragma unroll
        for (int mi = 0; mi < T2; ++mi)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int row = wm * 32 + mi * 64 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            const int gm = m0 + row;
            float v = acc[mi][ni][r];
            if constexpr (EPI == RDE_PLAIN) {
              if (col_ok && gm < a.cout) {
                if (a.b0) v += a.b0[gm];
                if (a.relu_out) v = fmaxf(v, 0.f);
                a.y0[(long long)gm * a.ttot + j] = v;
              }
            } else if constexpr (EPI == RDE_RESSKIP) {
              if (col_ok && gm < a.m_split) {
                v = (v + a.b0[gm]) + a.xres[(long long)gm * a.ttot + j];
                a.y0[(long long)gm * a.ttot + j] = v;
              } else if (col_ok && gm < a.cout) {
                const int s = gm - a.m_split;
                v += a.b1[s];
                if (a.accumulate) v = a.y1[(long long)s * a.ttot + j] + v;
                a.y1[(long long)s * a.ttot + j] = v;
              }
            } else {                                         // RDE_HEAD: the logits stay in LDS
              if (gm < a.cout) {
                if (a.b0) v += a.b0[gm];
                s_out[gm][cl] = v;
                if (a.logits && col_ok) a.logits[(long long)gm * a.ttot + j] = v;
              }
            }
          }
      }
    }
  }

  if constexpr (EPI == RDE_HEAD) {
    __syncthreads();
    const long long j = t0 + tid;
    if (tid < TILE && j < a.ttot) {
      const int Q = a.cout, tgt = s_i0[tid];
      float mx = s_out[0][tid];
      int arg = 0;
      for (int c = 1; c < Q; ++c) {
        const float v = s_out[c][tid];
        if (v > mx) { mx = v; arg = c; }                   // ties stay with the lowest index
      }
      float sum = 0.f;
      for (int c = 0; c < Q; ++c) sum += expf(s_out[c][tid] - mx);
      const bool ok = tgt >= 0 && tgt < Q;
      const float lse = logf(sum) + mx;
      a.nll[j] = ok ? lse - s_out[tgt][tid] : lse;
      a.hit[j] = (ok && arg == tgt) ? 1 : 0;
    }
  }
}

// x[c, j] = (jl > 0 ? W[c, q[jl - 1], 0] : 0) + W[c, q[jl], 1] + b[c]; grid (column blocks of 256, channel groups of 64)
__global__ __launch_bounds__(RD_THREADS) void rd_embed_kernel(const int64_t* off, const int64_t* qoff, const int32_t* q,
                                                              const float* W, const float* b, float* x, long long ttot,
                                                              int n, int R, int Q) {
  const long long j = (long long)blockIdx.x * RD_THREADS + threadIdx.x;
  if (j >= ttot) return;
  const int i = ragged_find_segment(off, n, j);
  const long long jl = j - (long long)off[i];
  const int32_t* qi = q + (long long)qoff[i];
  const int c1 = qi[jl], c0 = jl > 0 ? qi[jl - 1] : -1;
  const bool ok0 = c0 >= 0 && c0 < Q, ok1 = c1 >= 0 && c1 < Q;
  const int r0 = blockIdx.y * RD_TILE, r1 = min(r0 + RD_TILE, R);
  for (int c = r0; c < r1; ++c) {
    const float* wc = W + (long long)c * Q * 2;
    float v = (ok0 ? wc[2 * c0] : 0.f) + (ok1 ? wc[2 * c1 + 1] : 0.f);
    if (b) v += b[c];
    x[(long long)c * ttot + j] = v;
  }
}

// g[i, m] = (sum_c Wc_all[m, Cl + c] global_vec[i, c]) + bias_all[m], c ascending
__global__ __launch_bounds__(RD_THREADS) void rd_gvec_kernel(const float* gv, const float* Wc, const float* bias, float* g,
                                                             int n, int M, int Cl, int G) {
  const long long e = (long long)blockIdx.x * RD_THREADS + threadIdx.x;
  if (e >= (long long)n * M) return;
  const int i = (int)(e / M), m = (int)(e - (long long)i * M);
  const float* w = Wc + (long long)m * (Cl + G) + Cl;
  const float* v = gv + (long long)i * G;
  float s = 0.f;
  for (int c = 0; c < G; ++c) s += w[c] * v[c];
  g[e] = s + bias[m];
}

// one workgroup per utterance: lane t adds elements t, t + 256, ... in ascending order, then s[k] += s[k + h], h = 128 .. 1
__global__ __launch_bounds__(VQVAE_RAGGED_DECODER_REDUCE_LANES) void rd_reduce_kernel(const int64_t* off, const float* nll,
                                                                            const int32_t* hit, double* nll_sum,
                                                                            int64_t* hits) {
  __shared__ double sd[VQVAE_RAGGED_DECODER_REDUCE_LANES];
  __shared__ long long sh[VQVAE_RAGGED_DECODER_REDUCE_LANES];
  const int i = blockIdx.x, t = threadIdx.x;
  const long long lo = (long long)off[i], hi = (long long)off[i + 1];
  double s = 0.0;
  long long h = 0;
  for (long long j = lo + t; j < hi; j += VQVAE_RAGGED_DECODER_REDUCE_LANES) { s += (double)nll[j]; h += hit[j]; }
  sd[t] = s; sh[t] = h;
  __syncthreads();
  for (int w = VQVAE_RAGGED_DECODER_REDUCE_LANES / 2; w >= 1; w >>= 1) {
    if (t < w) { sd[t] += sd[t + w]; sh[t] += sh[t + w]; }
    __syncthreads();
  }
  if (t == 0) { nll_sum[i] = sd[0]; hits[i] = (int64_t)sh[0]; }
}

template <int MODE, int T2, int EPI>
static int launch_rd_gemm(const RdArgs& a, int row_tiles, hipStream_t st) {
  constexpr int K = EPI == RDE_GATE ? 2 : 1;
  constexpr int TILE = RD_TILE * T2;
  const size_t lds = rd_lds_bytes<T2, K>(EPI == RDE_HEAD ? cdiv(a.cout, TILE) * TILE : 0);
  if (int e = lds_opt_in<rd_gemm_kernel<MODE, T2, EPI>>(lds)) return e;
  const dim3 grid((unsigned)((a.ttot + TILE - 1) / TILE), (unsigned)row_tiles);
  hipLaunchKernelGGL((rd_gemm_kernel<MODE, T2, EPI>), grid, dim3(RD_THREADS), lds, st, a);
  return 0;
}

// PLAIN and RESSKIP pick the tile by the rows alone (never by the data), as ragged_conv_kernel does
template <int EPI>
static int launch_rd_by_rows(const RdArgs& a, hipStream_t st) {
  const bool fp32 = g_matmul_dtype == 0;
  if (a.cout >= RD_WIDE_ROWS)
    return fp32 ? launch_rd_gemm<0, 2, EPI>(a, cdiv(a.cout, 2 * RD_TILE), st) : launch_rd_gemm<3, 2, EPI>(a, cdiv(a.cout, 2 * RD_TILE), st);
  return fp32 ? launch_rd_gemm<0, 1, EPI>(a, cdiv(a.cout, RD_TILE), st) : launch_rd_gemm<3, 1, EPI>(a, cdiv(a.cout, RD_TILE), st);
}

static bool rd_desc_ok(const vqvae_rdec_desc* d) {
  return d && d->n >= 1 && d->R >= 1 && d->D >= 2 && d->D % 2 == 0 && d->S >= 1 && d->Q >= 1 && d->Q <= VQVAE_RAGGED_DECODER_MAX_CLASSES &&
         d->Cl >= 1 && d->G >= 0 && d->n_blocks >= 1 && d->upscale >= 1 && d->ttot >= 1 && d->tltot >= 1 &&
         d->ttot <= 0x7fffffffLL && d->tltot <= 0x7fffffffLL && (long long)d->n_blocks * d->D <= 0x7fffffffLL / (d->Cl + d->G) &&
         (long long)d->R * d->Q * 2 <= 0x7fffffffLL && (long long)d->D * d->R * 2 <= 0x7fffffffLL &&
         (long long)(d->R + d->S) * d->D <= 0x7fffffffLL && (long long)(d->S + d->Q) * d->S <= 0x7fffffffLL;
}

// the one workspace plan: the (S, ttot) activation between proj1 and proj2
struct RdPlan { size_t s1, total; };
static RdPlan plan_rd(const vqvae_rdec_desc* d) {
  WsPlan p;
  RdPlan r;
  r.s1 = p.take((size_t)d->S * (size_t)d->ttot * sizeof(float));
  r.total = p.total;
  return r;
}

}  // namespace vq

using namespace vq;

#define RD_COMMON(who)                                                                                                          \
  VQ_REQUIRE(d, who ": null descriptor");                                                                                       \
  VQ_REQUIRE(rd_desc_ok(d), who ": needs n, R, S, Cl, n_blocks, upscale, ttot, tltot >= 1, an even D >= 2, G >= 0, "             \
             "1 <= Q <= %d, ttot and tltot below 2^31 and weight tensors below 2^31 elements (got n %d, R %d, D %d, S %d, Q %d, Cl %d, G %d, n_blocks %d, " \
             "upscale %d, ttot %lld, tltot %lld)", VQVAE_RAGGED_DECODER_MAX_CLASSES, (int)d->n, (int)d->R, (int)d->D, (int)d->S, (int)d->Q, \
             (int)d->Cl, (int)d->G, (int)d->n_blocks, (int)d->upscale, (long long)d->ttot, (long long)d->tltot);                 \
  VQ_REQUIRE(g_matmul_dtype != 1, who ": matmul mode 1 (bf16 operands) is not supported by the ragged decoder; use mode 0, 2 or 3")

extern "C" int vqvae_ragged_decoder_abi_version(void) { return 1; }

extern "C" size_t vqvae_rdec_workspace_bytes(const vqvae_rdec_desc* d) {
  if (!rd_desc_ok(d)) return (size_t)-1;
  return plan_rd(d).total;
}

extern "C" int vqvae_rdec_embed(const vqvae_rdec_desc* d, const vqvae_rdec_tables* t, const int32_t* q, const float* W,
                                const float* b, float* x, vqvae_stream_t stream) {
  RD_COMMON("rdec_embed");
  VQ_REQUIRE(t && t->off && t->qoff, "rdec_embed: null tables, off or qoff");
  VQ_REQUIRE(q && W && x, "rdec_embed: null q, W or x");
  const long long blocks = (d->ttot + RD_THREADS - 1) / RD_THREADS;
  hipLaunchKernelGGL(rd_embed_kernel, dim3((unsigned)blocks, (unsigned)cdiv(d->R, RD_TILE)), dim3(RD_THREADS), 0,
                     (hipStream_t)stream, t->off, t->qoff, q, W, b, x, (long long)d->ttot, (int)d->n, (int)d->R, (int)d->Q);
  VQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int vqvae_rdec_cond_project(const vqvae_rdec_desc* d, const vqvae_rdec_tables* t, const float* local,
                                       const float* Wc_all, float* P, vqvae_stream_t stream) {
  RD_COMMON("rdec_cond_project");
  VQ_REQUIRE(t && t->latoff, "rdec_cond_project: null tables or latoff");
  VQ_REQUIRE(local && Wc_all && P, "rdec_cond_project: null local, Wc_all or P");
  RdArgs a{};
  a.x = local; a.off = t->latoff; a.w0 = Wc_all; a.y0 = P;
  a.ttot = d->tltot; a.w_rs = d->Cl + d->G;
  a.n = d->n; a.cin = d->Cl; a.cout = d->n_blocks * d->D; a.blocked_in = 1;
  if (int rc = launch_rd_by_rows<RDE_PLAIN>(a, (hipStream_t)stream)) return rc;
  VQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int vqvae_rdec_cond_global(const vqvae_rdec_desc* d, const float* global_vec, const float* Wc_all,
                                      const float* bias_all, float* g, vqvae_stream_t stream) {
  RD_COMMON("rdec_cond_global");
  VQ_REQUIRE(Wc_all && bias_all && g && (global_vec || d->G == 0), "rdec_cond_global: null global_vec, Wc_all, bias_all or g");
  const int M = d->n_blocks * d->D;
  const long long blocks = ((long long)d->n * M + RD_THREADS - 1) / RD_THREADS;
  VQ_REQUIRE(blocks <= 0x7fffffffLL, "rdec_cond_global: %d utterances of %d rows are too many for one launch", (int)d->n, M);
  hipLaunchKernelGGL(rd_gvec_kernel, dim3((unsigned)blocks), dim3(RD_THREADS), 0, (hipStream_t)stream, global_vec, Wc_all,
                     bias_all, g, (int)d->n, M, (int)d->Cl, (int)d->G);
  VQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int vqvae_rdec_gate(const vqvae_rdec_desc* d, const vqvae_rdec_tables* t, int block, int dilation, const float* x,
                               const float* Wd, const float* P, const float* g, float* z, vqvae_stream_t stream) {
  RD_COMMON("rdec_gate");
  VQ_REQUIRE(t && t->off && t->latoff && t->tl, "rdec_gate: null tables, off, latoff or tl");
  VQ_REQUIRE(x && Wd && P && g && z, "rdec_gate: null x, Wd, P, g or z");
  VQ_REQUIRE(block >= 0 && block < d->n_blocks, "rdec_gate: block %d of %d", block, (int)d->n_blocks);
  VQ_REQUIRE(dilation >= 1 && dilation <= VQVAE_RAGGED_DECODER_MAX_DILATION, "rdec_gate: dilation must be in 1 .. %d (got %d)",
             VQVAE_RAGGED_DECODER_MAX_DILATION, dilation);
  RdArgs a{};
  a.x = x; a.off = t->off; a.w0 = Wd; a.y0 = z;
  a.P = P + (long long)block * d->D * d->tltot;
  a.g = g + (long long)block * d->D;
  a.g_stride = (long long)d->n_blocks * d->D;
  a.latoff = t->latoff; a.tl = t->tl;
  a.ttot = d->ttot; a.x_cs = d->ttot; a.tltot = d->tltot; a.w_rs = (long long)d->R * 2;
  a.n = d->n; a.cin = d->R; a.cout = d->D; a.dil = dilation; a.upscale = d->upscale;
  const int rc = g_matmul_dtype == 0 ? launch_rd_gemm<0, 2, RDE_GATE>(a, cdiv(d->D / 2, RD_TILE), (hipStream_t)stream)
                                     : launch_rd_gemm<3, 2, RDE_GATE>(a, cdiv(d->D / 2, RD_TILE), (hipStream_t)stream);
  if (rc) return rc;
  VQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int vqvae_rdec_res_skip(const vqvae_rdec_desc* d, const float* z, const float* Wr, const float* br, const float* Ws,
                                   const float* bs, const float* x_in, float* x_out, float* skip, int accumulate,
                                   vqvae_stream_t stream) {
  RD_COMMON("rdec_res_skip");
  VQ_REQUIRE(z && Ws && bs && skip, "rdec_res_skip: null z, Ws, bs or skip");
  VQ_REQUIRE(!Wr || (br && x_in && x_out), "rdec_res_skip: Wr without br, x_in or x_out");
  RdArgs a{};
  a.x = z; a.w0 = Wr; a.w1 = Ws; a.b0 = br; a.b1 = bs; a.xres = x_in; a.y0 = x_out; a.y1 = skip;
  a.ttot = d->ttot; a.x_cs = d->ttot; a.w_rs = d->D / 2;
  a.n = 1; a.cin = d->D / 2; a.m_split = Wr ? d->R : 0; a.cout = a.m_split + d->S; a.accumulate = accumulate ? 1 : 0;
  if (int rc = launch_rd_by_rows<RDE_RESSKIP>(a, (hipStream_t)stream)) return rc;
  VQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int vqvae_rdec_head(const vqvae_rdec_desc* d, const vqvae_rdec_tables* t, const int32_t* q, const float* skip,
                               const float* W1, const float* b1, const float* W2, const float* b2, float* nll, int32_t* hit,
                               float* logits, void* ws, size_t ws_bytes, vqvae_stream_t stream) {
  RD_COMMON("rdec_head");
  VQ_REQUIRE(t && t->off && t->qoff, "rdec_head: null tables, off or qoff");
  VQ_REQUIRE(q && skip && W1 && W2 && nll && hit, "rdec_head: null q, skip, W1, W2, nll or hit");
  const RdPlan plan = plan_rd(d);
  VQ_REQUIRE(ws && ws_bytes >= plan.total, "rdec_head: workspace of %zu bytes, %zu needed", ws_bytes, plan.total);
  float* s1 = reinterpret_cast<float*>(static_cast<char*>(ws) + plan.s1);
  RdArgs a{};
  a.x = skip; a.w0 = W1; a.b0 = b1; a.y0 = s1;
  a.ttot = d->ttot; a.x_cs = d->ttot; a.w_rs = d->S;
  a.n = 1; a.cin = d->S; a.cout = d->S; a.relu_in = 1; a.relu_out = 1;
  if (int rc = launch_rd_by_rows<RDE_PLAIN>(a, (hipStream_t)stream)) return rc;
  RdArgs h{};
  h.x = s1; h.off = t->off; h.qoff = t->qoff; h.q = q; h.w0 = W2; h.b0 = b2; h.nll = nll; h.hit = hit; h.logits = logits;
  h.ttot = d->ttot; h.x_cs = d->ttot; h.w_rs = d->S;
  h.n = d->n; h.cin = d->S; h.cout = d->Q;
  const int rc = g_matmul_dtype == 0 ? launch_rd_gemm<0, 1, RDE_HEAD>(h, 1, (hipStream_t)stream)
                                     : launch_rd_gemm<3, 1, RDE_HEAD>(h, 1, (hipStream_t)stream);
  if (rc) return rc;
  VQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int vqvae_rdec_reduce(const vqvae_rdec_desc* d, const vqvae_rdec_tables* t, const float* nll, const int32_t* hit,
                                 double* nll_sum, int64_t* hits, vqvae_stream_t stream) {
  RD_COMMON("rdec_reduce");
  VQ_REQUIRE(t && t->off, "rdec_reduce: null tables or off");
  VQ_REQUIRE(nll && hit && nll_sum && hits, "rdec_reduce: null nll, hit, nll_sum or hits");
  hipLaunchKernelGGL(rd_reduce_kernel, dim3((unsigned)d->n), dim3(VQVAE_RAGGED_DECODER_REDUCE_LANES), 0, (hipStream_t)stream, t->off, nll,
                     hit, nll_sum, hits);
  VQ_LAUNCH_CHECK();
  return 0;
}
