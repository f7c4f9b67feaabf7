// The encoder's and ConditionEmbed's forward convolutions over a ragged batch (include/vqvae_ragged.h): the utterances lie
// end to end along time with no padding, one launch per conv stage runs all of them, and every tap checks the bounds of
// its OWN utterance, so no edge sample ever sees a neighbour or padding.
//
// ragged_conv_kernel<MODE, T2, K>  (cin > 1): a workgroup of four waves owns a 64 T2-row x 64 T2-column output tile, a wave a
//   T2 x T2 block of 32 x 32 accumulators; T2 = 2 from 128 output channels on -- by the model's width alone, never by the
//   data.  The columns are plain output columns of the ragged tensor: a column tile may span several segments and a segment
//   many tiles.  A thread per column finds the column's segment once (a search in the off_out prefix table) and leaves its
//   input base, first tap position, input length and output address in LDS.
//   K loop: channel groups of 16 ascending; per group the weights of all K taps (16 K contiguous floats per row: W is read
//   as Chainer stores it, no packed slab -- a slab would cost one more launch per stage for weights that stay in L2) and the
//   K shifted activation windows (16 channels per tap; a tap outside [0, len_in) is a SELECTED zero, never a load) are
//   staged as fp32.  What a thread stages is fixed for the whole loop (one (channel, tap) of every RP-th weight row, one
//   column of the windows), so the addresses advance by constants and the NEXT group's words travel in registers while the
//   matrix pipe works on this one's.  Every wave then runs the taps in order on its fragments:
//     MODE 0  eight v_mfma_f32_32x32x2_f32 per tap and accumulator
//     MODE 3  split3 (gemm_common.h) of its fragments and the six bf16 products of mfma_chain<3> per tap and accumulator
//   The order per output element is fixed and the same in every tile position and tile size, there is no split-K, no scale
//   and no atomic: the result is a pure function of the utterance's samples and the weights.
//   LDS (dynamic): 64 x (TILE + 1) + 64 x TILE floats of operands + 32 bytes per column = 34.3 KB (T2 = 1) / 68.3 KB
//   (T2 = 2, opted in once per kernel), two barriers per channel group.  Registers, accumulators included: 132 - 160
//   (T2 = 1: three waves per SIMD), 244 - 312 (T2 = 2: up to 64 staged words beside 64 accumulators; one wave per SIMD
//   in three of the four instantiations).  Capped at 256 (amdgpu_waves_per_eu(2)) they spill 48 - 184 bytes per lane to
//   scratch, so the cap is not set; no instantiation uses scratch (tests/test_host_ragged_budget.py).
// ragged_conv1_kernel  (cin == 1, the encoder's first stage): memory-bound VALU, a thread per output column, 64 output
//   channels per workgroup row; fp32 multiplies and adds in tap order (-ffp-contract=off), coalesced stores.
// ragged_code_gather_kernel / ragged_speaker_gather_kernel: the two gathers of the way back from stored codes.
//
// Every address is formed in 64 bits.  Stores: y[m * ttot_out + j] (ragged) or y[cout * off_out[i] + m * len_out[i] + jl]
// (blocked) for m < cout and j < ttot_out only; plain vector stores.
#include "gemm_common.h"
#include "ragged_seg.h"
#include "../../include/vqvae_ragged.h"

namespace vq {

constexpr int RG_TILE = 64;      // rows and columns of a workgroup's output tile
constexpr int RG_KC = 16;        // channels per K step
constexpr int RG_MAXK = 4;       // taps
constexpr int RG_THREADS = 256;
constexpr int RG_WIDE_COUT = 128;  // from this many output channels on: 128 x 128 tiles

struct RaggedArgs {
  const float* x; const int64_t* off_in; const int32_t* len_in; const int64_t* off_out;
  const float* w; const float* bias; float* y;
  long long ttot_out, x_cstride;
  int n, cin, cout, K, stride, pad, dil, relu, blocked;
};

// T2 = 1: 64 x 64 tiles, a wave one 32 x 32 accumulator; T2 = 2: 128 x 128 tiles, a wave a 2 x 2 block of them (rows
// wm * 32 + 64 mi, columns wn * 32 + 64 ni), so that a fragment split once serves two products and a staged word twice the
// outputs.  The choice depends on cout alone (never on the data or the batch), and an output element's arithmetic is the
// same in both: the same K order, the same products.
template <int T2>
constexpr size_t ragged_lds_bytes() {
  constexpr size_t T = RG_TILE * T2;
  return T * (3 * sizeof(long long) + 2 * sizeof(int)) + (size_t)RG_MAXK * RG_KC * ((T + 1) + T) * sizeof(float);
}

template <int MODE, int T2, int K>
__global__ __launch_bounds__(RG_THREADS) void ragged_conv_kernel(RaggedArgs a) {
  constexpr int TILE = RG_TILE * T2;
  constexpr int ROWS = RG_MAXK * RG_KC;                   // staged (tap, channel) rows per K step
  constexpr int RL = RG_KC * K;                           // floats of one weight row per channel group: W[m][c0 .. c0 + 15][0 .. K - 1], contiguous
  constexpr int RP = RG_THREADS / RL;                     // weight rows per pass of the workgroup (4 or 5)
  constexpr int NPA = (TILE + RP - 1) / RP;               // passes over the tile's weight rows
  constexpr int BSTEP = RG_THREADS / TILE;                // (tap, channel) rows of activations per pass
  constexpr int NPB = K * RG_KC / BSTEP;                  // passes over the K 16-channel windows
  extern __shared__ __attribute__((aligned(16))) unsigned char rg_lds[];
  long long* s_base = reinterpret_cast<long long*>(rg_lds);   // [TILE] off_in of the column's segment
  long long* s_yoff = s_base + TILE;                      // [TILE] where row 0 of the column is stored
  long long* s_ycs = s_yoff + TILE;                       // [TILE] elements between the rows of the column in y
  int* s_pos0 = reinterpret_cast<int*>(s_ycs + TILE);     // [TILE] input position of tap 0: stride * jl - pad
  int* s_len = s_pos0 + TILE;                             // [TILE] input length of the segment; 0 for a column past the end
  float (*sA)[TILE + 1] = reinterpret_cast<float (*)[TILE + 1]>(s_len + TILE);      // [tap * 16 + channel][row]
  float (*sB)[TILE] = reinterpret_cast<float (*)[TILE]>(&sA[ROWS][0]);              // [tap * 16 + channel][column]

  const int tid = threadIdx.x;
  const long long t0 = (long long)blockIdx.x * TILE;
  const int m0 = blockIdx.y * TILE;

  if (tid < TILE) {
    const long long j = t0 + tid;
    if (j < a.ttot_out) {
      const int i = ragged_find_segment(a.off_out, a.n, j);
      const long long o = (long long)a.off_out[i];
      const long long jl = j - o;
      s_base[tid] = (long long)a.off_in[i];
      s_pos0[tid] = (int)(jl * a.stride - a.pad);
      s_len[tid] = a.len_in[i];
      if (a.blocked) {
        const long long lo = (long long)a.off_out[i + 1] - o;
        s_yoff[tid] = (long long)a.cout * o + jl;
        s_ycs[tid] = lo;
      } else {
        s_yoff[tid] = j;
        s_ycs[tid] = a.ttot_out;
      }
    } else {
      s_base[tid] = 0; s_pos0[tid] = 0; s_len[tid] = 0; s_yoff[tid] = 0; s_ycs[tid] = 0;
    }
  }
  __syncthreads();

  // What a thread stages is fixed for the whole K loop: one (channel, tap) of the weight rows a_row, a_row + RP, ... and one
  // column of the activation windows, whose segment it reads ONCE.  The next channel group's words travel in registers while
  // the matrix pipe works on this one's.
  const bool a_act = tid < RP * RL;
  const int a_row = tid / RL, a_r = tid - a_row * RL;
  const int a_c = a_r / K, a_k = a_r - a_c * K;
  const int b_col = tid & (TILE - 1), b_kc0 = tid / TILE;
  const int b_pos0 = s_pos0[b_col], b_len = s_len[b_col];
  const float* b_src = a.x + s_base[b_col];
  float ra[NPA], rb[NPB];
  auto fetch = [&](const int c0) {
#pragma unroll
    for (int p = 0; p < NPA; ++p) {
      const int m = p * RP + a_row;
      const bool ok = a_act && m < TILE && m0 + m < a.cout && c0 + a_c < a.cin;
      ra[p] = ok ? a.w[((long long)(m0 + m) * a.cin + c0) * K + a_r] : 0.f;
    }
#pragma unroll
    for (int p = 0; p < NPB; ++p) {
      const int kc = b_kc0 + p * BSTEP;                    // tap * 16 + channel
      const int k = kc >> 4, ch = c0 + (kc & (RG_KC - 1));
      const int pos = b_pos0 + k * a.dil;
      const bool ok = pos >= 0 && pos < b_len && ch < a.cin;      // a tap outside its own utterance is a selected zero, never a load
      rb[p] = ok ? b_src[(long long)ch * a.x_cstride + pos] : 0.f;
    }
  };
  fetch(0);

  const int wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1;
  const int lr = lane & 31, lh = lane >> 5;
  f32x16 acc[T2][T2];
#pragma unroll
  for (int mi = 0; mi < T2; ++mi)
#pragma unroll
    for (int ni = 0; ni < T2; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

  for (int c0 = 0; c0 < a.cin; c0 += RG_KC) {
    if (c0) __syncthreads();                               // the previous group's fragments are read
#pragma unroll
    for (int p = 0; p < NPA; ++p) {
      const int m = p * RP + a_row;
      if (a_act && m < TILE) sA[a_k * RG_KC + a_c][m] = ra[p];
    }
#pragma unroll
    for (int p = 0; p < NPB; ++p) sB[b_kc0 + p * BSTEP][b_col] = rb[p];
    __syncthreads();
    if (c0 + RG_KC < a.cin) fetch(c0 + RG_KC);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if constexpr (MODE == 0) {
#pragma unroll
        for (int s = 0; s < RG_KC / 2; ++s) {
          float av[T2], bv[T2];
#pragma unroll
          for (int q = 0; q < T2; ++q) {
            av[q] = sA[k * RG_KC + 2 * s + lh][wm * 32 + q * 64 + lr];
            bv[q] = sB[k * RG_KC + 2 * s + lh][wn * 32 + q * 64 + lr];
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
            av[q] = sA[k * RG_KC + 8 * lh + q][wm * 32 + t * 64 + lr];
            bv[q] = sB[k * RG_KC + 8 * lh + q][wn * 32 + t * 64 + lr];
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
#pragma unroll
  for (int ni = 0; ni < T2; ++ni) {
    const int cl = wn * 32 + ni * 64 + lr;
    if (t0 + cl >= a.ttot_out) continue;
    const long long yoff = s_yoff[cl], ycs = s_ycs[cl];
#pragma unroll
    for (int mi = 0; mi < T2; ++mi)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int gm = m0 + wm * 32 + mi * 64 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (gm < a.cout) {
          float v = acc[mi][ni][r];
          if (a.bias) v += a.bias[gm];
          if (a.relu) v = fmaxf(v, 0.f);
          a.y[yoff + (long long)gm * ycs] = v;
        }
      }
  }
}

// cin == 1: y[m, j] = act(((w[m,0] x0 + w[m,1] x1) + ...) + bias[m]); grid (column blocks of 256, row blocks of 64)
__global__ __launch_bounds__(RG_THREADS) void ragged_conv1_kernel(RaggedArgs a) {
  __shared__ float sw[RG_TILE][RG_MAXK];
  __shared__ float sb[RG_TILE];
  const int m0 = blockIdx.y * RG_TILE;
  const int rows = min(RG_TILE, a.cout - m0);
  for (int e = threadIdx.x; e < RG_TILE * RG_MAXK; e += RG_THREADS) {
    const int m = e / RG_MAXK, k = e - m * RG_MAXK;
    sw[m][k] = (m < rows && k < a.K) ? a.w[(long long)(m0 + m) * a.K + k] : 0.f;
  }
  if (threadIdx.x < RG_TILE) sb[threadIdx.x] = (a.bias && (int)threadIdx.x < rows) ? a.bias[m0 + threadIdx.x] : 0.f;
  __syncthreads();
  const long long j = (long long)blockIdx.x * RG_THREADS + threadIdx.x;
  if (j >= a.ttot_out) return;
  const int i = ragged_find_segment(a.off_out, a.n, j);
  const long long o = (long long)a.off_out[i];
  const long long jl = j - o;
  const long long base = (long long)a.off_in[i];
  const int len = a.len_in[i];
  const int pos0 = (int)(jl * a.stride - a.pad);
  float xv[RG_MAXK];
#pragma unroll
  for (int k = 0; k < RG_MAXK; ++k) {
    const int pos = pos0 + k * a.dil;
    xv[k] = (k < a.K && pos >= 0 && pos < len) ? a.x[base + pos] : 0.f;
  }
  long long yoff, ycs;
  if (a.blocked) { yoff = (long long)a.cout * o + jl; ycs = (long long)a.off_out[i + 1] - o; }
  else { yoff = j; ycs = a.ttot_out; }
  for (int m = 0; m < rows; ++m) {
    float v = sw[m][0] * xv[0];
#pragma unroll
    for (int k = 1; k < RG_MAXK; ++k) v += sw[m][k] * xv[k];      // taps past K hold exact zeros
    v += sb[m];
    if (a.relu) v = fmaxf(v, 0.f);
    a.y[yoff + (long long)(m0 + m) * ycs] = v;
  }
}

__global__ __launch_bounds__(RG_THREADS) void ragged_code_gather_kernel(const int32_t* idx, const float* W, long long ttot,
                                                                        int d, int k, float* e) {
  const long long j = (long long)blockIdx.x * RG_THREADS + threadIdx.x;
  if (j >= ttot) return;
  const int id = idx[j];
  const bool ok = id >= 0 && id < k;
  const float* row = W + (long long)(ok ? id : 0) * d;
  for (int c = 0; c < d; ++c) e[(long long)c * ttot + j] = ok ? row[c] : 0.f;
}

__global__ __launch_bounds__(RG_THREADS) void ragged_speaker_gather_kernel(const int32_t* speaker, const float* E, int n, int G,
                                                                           int n_speaker, float* out) {
  const long long e = (long long)blockIdx.x * RG_THREADS + threadIdx.x;
  if (e >= (long long)n * G) return;
  const int i = (int)(e / G), g = (int)(e - (long long)i * G);
  const int s = speaker[i];
  out[e] = (s >= 0 && s < n_speaker) ? E[(long long)s * G + g] : 0.f;
}

// the one LDS opt-in and launch of a (mode, tile, taps) instantiation; 128 x 128 tiles (T2 = 2) from RG_WIDE_COUT output
// channels on: by the model's width alone
template <int MODE, int T2, int K>
static int launch_ragged_conv(const RaggedArgs& a, hipStream_t st) {
  constexpr int TILE = RG_TILE * T2;
  constexpr size_t lds = ragged_lds_bytes<T2>();
  if (int e = lds_opt_in<ragged_conv_kernel<MODE, T2, K>>(lds)) return e;
  const dim3 grid((unsigned)((a.ttot_out + TILE - 1) / TILE), (unsigned)cdiv(a.cout, TILE));
  hipLaunchKernelGGL((ragged_conv_kernel<MODE, T2, K>), grid, dim3(RG_THREADS), lds, st, a);
  return 0;
}

static bool ragged_window_ok(const vqvae_ragged_conv_desc* d) {
  if (d->K == 4 && d->stride == 2 && d->pad == 1 && d->dil == 1) return true;
  if (d->K == 3 && d->stride == 1 && d->pad == d->dil)
    return d->dil == 1 || d->dil == 2 || d->dil == 4 || d->dil == 8 || d->dil == 16;
  return false;
}

// the one workspace plan of vqvae_ragged_conv_fwd: nothing is taken today
struct RaggedConvPlan { size_t total; };
static RaggedConvPlan plan_ragged_conv(const vqvae_ragged_conv_desc*) {
  WsPlan p;
  return RaggedConvPlan{p.total};
}

}  // namespace vq

using namespace vq;

extern "C" int vqvae_ragged_abi_version(void) { return 1; }

extern "C" size_t vqvae_ragged_conv_workspace_bytes(const vqvae_ragged_conv_desc* d) {
  if (!d || d->n < 1 || d->cin < 1 || d->cout < 1 || d->ttot_out < 1 || d->x_cstride < 0 || !ragged_window_ok(d))
    return (size_t)-1;
  return plan_ragged_conv(d).total;
}

extern "C" int vqvae_ragged_conv_fwd(const vqvae_ragged_conv_desc* d, const float* x, const int64_t* off_in,
                                     const int32_t* len_in, const int64_t* off_out, const float* W, const float* bias,
                                     float* y, void* ws, size_t ws_bytes, vqvae_stream_t stream) {
  VQ_REQUIRE(d, "ragged_conv_fwd: null descriptor");
  VQ_REQUIRE(x && off_in && len_in && off_out && W && y, "ragged_conv_fwd: null x, off_in, len_in, off_out, W or y");
  VQ_REQUIRE(d->n >= 1 && d->cin >= 1 && d->cout >= 1, "ragged_conv_fwd: n, cin and cout must be at least 1 (got %d, %d, %d)",
             (int)d->n, (int)d->cin, (int)d->cout);
  VQ_REQUIRE(d->ttot_out >= 1, "ragged_conv_fwd: ttot_out must be at least 1 (got %lld)", (long long)d->ttot_out);
  VQ_REQUIRE(ragged_window_ok(d),
             "ragged_conv_fwd: (K, stride, pad, dil) must be (4, 2, 1, 1) or (3, 1, d, d) with d in {1, 2, 4, 8, 16} (got %d, %d, %d, %d)",
             (int)d->K, (int)d->stride, (int)d->pad, (int)d->dil);
  VQ_REQUIRE(d->x_cstride >= 0, "ragged_conv_fwd: x_cstride must not be negative (got %lld)", (long long)d->x_cstride);
  VQ_REQUIRE(g_matmul_dtype != 1, "ragged_conv_fwd: matmul mode 1 (bf16 operands) is not supported by the ragged front end; "
             "use mode 0, 2 or 3");
  const long long tiles = (d->ttot_out + RG_TILE - 1) / RG_TILE;
  VQ_REQUIRE(tiles <= 0x7fffffffLL, "ragged_conv_fwd: %lld columns are more than 2^31 - 1 column tiles", (long long)d->ttot_out);
  const RaggedConvPlan plan = plan_ragged_conv(d);
  VQ_REQUIRE(ws_bytes >= plan.total && (ws || !plan.total), "ragged_conv_fwd: workspace of %zu bytes, %zu needed", ws_bytes, plan.total);
  RaggedArgs a{};
  a.x = x; a.off_in = off_in; a.len_in = len_in; a.off_out = off_out; a.w = W; a.bias = bias; a.y = y;
  a.ttot_out = d->ttot_out; a.x_cstride = d->x_cstride;
  a.n = d->n; a.cin = d->cin; a.cout = d->cout; a.K = d->K; a.stride = d->stride; a.pad = d->pad; a.dil = d->dil;
  a.relu = d->relu ? 1 : 0; a.blocked = d->blocked_out ? 1 : 0;
  const hipStream_t st = (hipStream_t)stream;
  if (d->cin == 1) {
    const long long blocks = (d->ttot_out + RG_THREADS - 1) / RG_THREADS;
    hipLaunchKernelGGL(ragged_conv1_kernel, dim3((unsigned)blocks, (unsigned)cdiv(d->cout, RG_TILE)), dim3(RG_THREADS), 0, st, a);
  } else {
    const bool fp32 = g_matmul_dtype == 0, wide = d->cout >= RG_WIDE_COUT, k4 = d->K == 4;
    int rc = 0;
    if (wide) rc = fp32 ? (k4 ? launch_ragged_conv<0, 2, 4>(a, st) : launch_ragged_conv<0, 2, 3>(a, st))
                        : (k4 ? launch_ragged_conv<3, 2, 4>(a, st) : launch_ragged_conv<3, 2, 3>(a, st));
    else rc = fp32 ? (k4 ? launch_ragged_conv<0, 1, 4>(a, st) : launch_ragged_conv<0, 1, 3>(a, st))
                   : (k4 ? launch_ragged_conv<3, 1, 4>(a, st) : launch_ragged_conv<3, 1, 3>(a, st));
    if (rc) return rc;
  }
  VQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int vqvae_ragged_code_gather(const int32_t* idx, const float* W, int64_t ttot, int d, int k, float* e,
                                        vqvae_stream_t stream) {
  VQ_REQUIRE(idx && W && e, "ragged_code_gather: null idx, W or e");
  VQ_REQUIRE(ttot >= 1 && d >= 1 && k >= 1, "ragged_code_gather: ttot, d and k must be at least 1 (got %lld, %d, %d)",
             (long long)ttot, d, k);
  const long long blocks = (ttot + RG_THREADS - 1) / RG_THREADS;
  VQ_REQUIRE(blocks <= 0x7fffffffLL, "ragged_code_gather: %lld columns are too many for one launch", (long long)ttot);
  hipLaunchKernelGGL(ragged_code_gather_kernel, dim3((unsigned)blocks), dim3(RG_THREADS), 0, (hipStream_t)stream, idx, W,
                     (long long)ttot, d, k, e);
  VQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int vqvae_ragged_speaker_gather(const int32_t* speaker, const float* E, int n, int G, int n_speaker,
                                           float* global_vec, vqvae_stream_t stream) {
  VQ_REQUIRE(speaker && E && global_vec, "ragged_speaker_gather: null speaker, E or global_vec");
  VQ_REQUIRE(n >= 1 && G >= 1 && n_speaker >= 1, "ragged_speaker_gather: n, G and n_speaker must be at least 1 (got %d, %d, %d)",
             n, G, n_speaker);
  const long long blocks = ((long long)n * G + RG_THREADS - 1) / RG_THREADS;
  hipLaunchKernelGGL(ragged_speaker_gather_kernel, dim3((unsigned)blocks), dim3(RG_THREADS), 0, (hipStream_t)stream, speaker, E,
                     n, G, n_speaker, global_vec);
  VQ_LAUNCH_CHECK();
  return 0;
}
