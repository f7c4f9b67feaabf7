// lin_stream_wide.hip -- the residual 1x1 of the 512-channel decoder (Ch = 256 gate channels -> Cr = 512 rows, residual add)
// inside the float32x2 pre-split chain: lin256_stream_kernel, the streaming kernel of lin128_stream_kernel's family for
// the reference's default model (params.py: residual_channels = dilated_channels = 512).
//
// Same shape of problem as the 128 -> 256 projection (HBM-bound: at B = 4, T = 7680 the launch reads z, 31 MB, and x_l,
// 63 MB, and writes x_{l+1}, 63 MB, against 16 GFLOP), same answer: a persistent 8-wave workgroup per CU walks 32-column
// tiles with the weights in registers and a whole tile of loads in flight.  What differs is the weight matrix: 512 x 256
// in two fp16 pieces is 512 KB, four times what one workgroup's registers took at 256 x 128.  So the output rows are
// split over TWO workgroups (row slices [0, 256) and [256, 512)); a wave owns 32 rows of its slice over the whole
// contraction: 16 K steps x 2 pieces x 16 bytes = 128 VGPRs of A fragments per lane, read once.  The two workgroups of a
// column tile sit 8 apart in the grid (same XCD, dispatched together), so the second read of a z tile is an L2 hit: z
// leaves HBM once.
//
// VGPRs: 218 (x_l pre-split) / 214 (x_l fp32) of the 256 a wave has at two waves per SIMD (__launch_bounds__(512, 1)):
// 128 of weights, 16 accumulators, 2 x 16 residual operands (this tile's and the next one's, requested behind the MFMA
// loop), 16 of the z tile in flight, addressing; no scratch, no spill (pinned by tests/test_host_wide_chain.py from the
// code object's metadata).  The wave index is made scalar (readfirstlane): every buffer access then keeps its row offset
// in SGPRs.  LDS: two 32 KB images of a z tile (16 steps x [piece][k-half][column] 16-byte words) + 1 KB of biases.
//
// Arithmetic: float32x2 -- z split under |z| <= 1 while it is staged, three fp16 products per step, small products first,
// K ascending, (acc * 2^ku + bias) + x_l, x_{l+1} stored PRE-SPLIT under the a-priori bound max|x_l| + l1 (presplit_pair;
// DESIGN.md 3a) -- the expressions of lin128_stream_kernel's pre-split instantiation.  The tiled kernel presents this
// contraction as two interleaved halves (launch_gemm), so the two agree to the rounding of a different summation order,
// not bitwise (tests/test_gpu_wide_chain.py compares the stored dwords with float64 over the stored operands).
#include "gemm_common.h"

namespace vq {

namespace {
struct LinWideArgs {
  const uint4* w; int ldw;                 // packed format-3 slab (pack_kernel), one tap, K = 256, ldw >= 512 rows
  const float* z; long z_bstride;          // (B, 256, T)
  const float* add; long add_bstride;      // (B, 512, T): x_l, fp32 or pre-split (ADDPRE)
  float* y; long y_bstride;                // (B, 512, T): x_{l+1}, pre-split
  const float* bias;                       // 512 or null
  int T, tiles_per_b, ntiles;
  const unsigned* wamax; const unsigned* z_amax; float z_amax_static; unsigned* amax_out;
  const unsigned* add_scale; const unsigned* add_amax; const float* l1; unsigned* scale_out;
  const unsigned* floor_w; const unsigned* floor_p;      // see GemmArgs
};
constexpr int LW_K = 256, LW_ROWS = 256, LW_NC = 32;     // contraction; rows per workgroup (slice); columns per tile
constexpr int LW_KS = LW_K / 16;                         // K steps
constexpr int LW_STEPW = 2 * 2 * LW_NC;                  // 16-byte words per K step of the z image: [piece][k-half][column]
}  // namespace

// ADDPRE: x_l arrives pre-split (every block but the stack's first)
template <bool ADDPRE>
__global__ __launch_bounds__(512, 1) void lin256_stream_kernel(const LinWideArgs a) {
  constexpr int NC = LW_NC, KS = LW_KS, STEPW = LW_STEPW, CPC = 2;     // CPC: columns per staging thread (16 column groups x 32 channel quads)
  __shared__ uint4 Bs[2][KS * STEPW];
  __shared__ float4 bias_s[LW_ROWS / 4];
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 31, lk = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);       // wave-uniform: the row offsets of the buffer accesses stay in SGPRs
  const int T = a.T;
  // workgroups id and id + 8 (same XCD) share their column tiles: row slices 0 and 1
  const int slice = (blockIdx.x >> 3) & 1;
  const int wg = (blockIdx.x & 7) + 8 * (blockIdx.x >> 4);
  const int stride = gridDim.x >> 1;
  const int row0 = LW_ROWS * slice + 32 * wave;          // this wave's first output row

  // ---- the weights: this wave's 32 rows x 256 k, as MFMA A fragments, for the whole launch ----
  uint4 af[KS][2];
#pragma unroll
  for (int s = 0; s < KS; ++s)
#pragma unroll
    for (int p = 0; p < 2; ++p) af[s][p] = a.w[((long)(s * 2 + p) * 2 + lk) * a.ldw + row0 + li];
  if (tid < LW_ROWS) reinterpret_cast<float*>(bias_s)[tid] = a.bias ? a.bias[LW_ROWS * slice + tid] : 0.f;

  // ---- staging role: 2 consecutive columns x 4 consecutive channels, in each half of the contraction ----
  const int cg = tid & 15, kq = tid >> 4;
  const int k0 = 4 * kq;                                 // and k0 + 128
  // word (s, piece, k-half, col) holds k = 16 s + 8 half .. + 7; this thread fills 8-byte half `sub` of it
  const int st_word = ((k0 >> 4) * 4 + ((k0 >> 3) & 1)) * NC + CPC * cg;
  const int st_sub = (k0 >> 2) & 1;
  float zr[2][4][CPC];
  const int last = a.ntiles - 1;
#define LW_FETCH(TILE)                                                                         \
  {                                                                                            \
    const int tl_ = min((TILE), last);          /* past the end: re-read the last tile, unused */ \
    const int b_ = tl_ / a.tiles_per_b, t_ = (tl_ - b_ * a.tiles_per_b) * NC;                  \
    const float* p_ = a.z + (long)b_ * a.z_bstride + (long)k0 * T + t_ + CPC * cg;             \
    _Pragma("unroll") for (int h = 0; h < 2; ++h)                                              \
      _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                          \
        const float2 v_ = L128_Z_NT ? __builtin_bit_cast(float2, __builtin_nontemporal_load(reinterpret_cast<const f32x2_t*>(p_ + (long)(128 * h + j) * T))) \
                                    : *reinterpret_cast<const float2*>(p_ + (long)(128 * h + j) * T); \
        zr[h][j][0] = v_.x; zr[h][j][1] = v_.y;                                                \
      }                                                                                        \
  }
#define LW_STAGE(BUF)                                                                          \
  {                                                                                            \
    _Pragma("unroll") for (int h = 0; h < 2; ++h) {                                            \
      uint4* base_ = &Bs[BUF][st_word + h * (KS / 2) * STEPW];                                 \
      _Pragma("unroll") for (int c = 0; c < CPC; ++c) {                                        \
        uint2* d_ = reinterpret_cast<uint2*>(base_ + c) + st_sub;                              \
        unsigned h0, l0, h1, l1;                                                               \
        split2(zr[h][0][c], zr[h][1][c], kz, h0, l0);                                          \
        split2(zr[h][2][c], zr[h][3][c], kz, h1, l1);                                          \
        d_[0] = make_uint2(h0, h1);                                                            \
        d_[2 * (2 * NC)] = make_uint2(l0, l1);                                                 \
      }                                                                                        \
    }                                                                                          \
  }
  // residual operands of a tile, in the accumulator layout (requested a tile ahead, behind the MFMA loop)
  const unsigned voff = 4u * (unsigned)(4 * lk * T + li);
#define LW_XLOAD(XV, TILE)                                                                     \
  {                                                                                            \
    const int tl_ = min((TILE), last);                                                         \
    const int b_ = tl_ / a.tiles_per_b, t_ = (tl_ - b_ * a.tiles_per_b) * NC;                  \
    const rsrc_t rx_ = make_rsrc(reinterpret_cast<const char*>(a.add) + (long)b_ * a.add_bstride * 4); \
    const unsigned sb_ = 4u * (unsigned)(row0 * T + t_);                                       \
    _Pragma("unroll") for (int r = 0; r < 16; ++r)                                             \
      XV[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rx_, voff, sb_ + 4u * (unsigned)(((r & 3) + 8 * (r >> 2)) * T), L128_X_AUX)); \
  }
  // one tile: MFMAs on LDS buffer CUR, next tile's z -> the other buffer, epilogue with XCUR while XNXT (the next tile's
  // residual) and the z tile after the next travel
#define LW_TILE(CUR, XCUR, XNXT)                                                               \
  {                                                                                            \
    const int b = tile / a.tiles_per_b, t0 = (tile - b * a.tiles_per_b) * NC;                  \
    f32x16 acc;                                                                                \
    _Pragma("unroll") for (int r = 0; r < 16; ++r) acc[r] = 0.f;                               \
    const uint4* bb = &Bs[CUR][lk * NC + li];                                                  \
    _Pragma("unroll") for (int s = 0; s < KS; ++s) {                                           \
      uint4 bq[2];                                                                             \
      _Pragma("unroll") for (int p = 0; p < 2; ++p) bq[p] = bb[s * STEPW + p * 2 * NC];        \
      acc = mfma_chain<2>(af[s], bq, acc);                                                     \
    }                                                                                          \
    LW_STAGE(CUR ^ 1);                                                                         \
    LW_XLOAD(XNXT, tile + stride);                                                             \
    {                                                                                          \
      const rsrc_t ry = make_rsrc(reinterpret_cast<char*>(a.y) + (long)b * a.y_bstride * 4);   \
      const unsigned sbase = 4u * (unsigned)(row0 * T + t0);                                   \
      _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                          \
        const float4 bq4 = bias_s[8 * wave + 2 * q + lk];         /* rows row0 + 8q + 4lk .. + 3 */ \
        const float bv[4] = {bq4.x, bq4.y, bq4.z, bq4.w};                                      \
        _Pragma("unroll") for (int j = 0; j < 4; j += 2) {                                     \
          const int r = 4 * q + j;                                                             \
          float va = __builtin_ldexpf(acc[r], ku) + bv[j], vb = __builtin_ldexpf(acc[r + 1], ku) + bv[j + 1]; \
          if constexpr (ADDPRE) { va += presplit_value(XCUR[r], kadd); vb += presplit_value(XCUR[r + 1], kadd); } \
          else { va += XCUR[r]; vb += XCUR[r + 1]; }                                           \
          am = fmaxf(am, fmaxf(fabsf(va), fabsf(vb)));                                         \
          const unsigned so_ = sbase + 4u * (unsigned)((j + 8 * q) * T);                       \
          unsigned da_, db_;                                                                   \
          presplit_pair(va, vb, kout, da_, db_);                                               \
          __builtin_amdgcn_raw_buffer_store_b32((int)da_, ry, voff, so_, L128_ST_AUX);         \
          __builtin_amdgcn_raw_buffer_store_b32((int)db_, ry, voff, so_ + 4u * (unsigned)T, L128_ST_AUX); \
        }                                                                                      \
      }                                                                                        \
    }                                                                                          \
    LW_FETCH(tile + 2 * stride);                                                               \
    __syncthreads();                                                                           \
  }

  int tile = wg;
  if (tile >= a.ntiles) return;
  float xa[16], xb[16];
  LW_FETCH(tile);
  LW_XLOAD(xa, tile);
  // the scales, read while the first tile travels: z is scaled by 2^kz, the accumulators come back by 2^ku
  const int ew = amax_expo(amax_load(a.wamax)), ez = amax_expo(a.z_amax ? amax_load(a.z_amax) : __builtin_bit_cast(unsigned, a.z_amax_static));
  const int kz = 14 - ez, ku = ew + ez - 28;
  [[maybe_unused]] int kadd = 0;                 // x_l comes back by 2^kadd, x_{l+1} is stored under 2^kout
  if constexpr (ADDPRE) kadd = amax_expo(amax_load(a.add_scale)) - 14;
  int kout;
  {
    float bound = bound_margin(__builtin_bit_cast(float, amax_load(a.add_amax)) + a.l1[0]);
    if (a.floor_p != nullptr) {                  // the next block's gate GEMM adds its condition as a K step: leave it room
      const int ef = amax_expo(amax_load(a.floor_p)) - amax_expo(amax_load(a.floor_w)) - 1;
      bound = fmaxf(bound, __builtin_ldexpf(1.f, min(max(ef, -100), 100)));
    }
    kout = 14 - amax_expo(__builtin_bit_cast(unsigned, bound));
    scale_publish(a.scale_out, bound);           // (both row slices of workgroup pair 0 write the same word)
  }
  float am = 0.f;
  LW_STAGE(0);
  __syncthreads();
  LW_FETCH(tile + stride);
  while (true) {
    LW_TILE(0, xa, xb);
    tile += stride;
    if (tile >= a.ntiles) break;
    LW_TILE(1, xb, xa);
    tile += stride;
    if (tile >= a.ntiles) break;
  }
  if (a.amax_out != nullptr) amax_commit(am * PRESPLIT_AMAX_UP, a.amax_out);      // (x_{l+1} is always stored pre-split here)
#undef LW_FETCH
#undef LW_STAGE
#undef LW_XLOAD
#undef LW_TILE
}

// the launches the kernel serves: float32x2, one segment z (B, 256, T) -> 512 rows, residual add, x_{l+1} stored pre-split
// with its bound's inputs, nothing else in the epilogue
bool lin_wide_shape(const GemmArgs& g) {
  const Seg& s0 = g.seg[0];
  if (g.nseg != 1 || g.M != 2 * LW_ROWS || s0.cin != LW_K || g.out[1].y != nullptr || g.B <= 0) return false;
  if (!g.f16x2 || g.out[0].y_fmt != FMT_F16X2 || !g.out[0].add || !g.add_amax || !g.bound_l1 || !g.scale_out || (g.out[0].add_fmt != FMT_F32 && !g.add_scale)) return false;
  if (g.out[0].relu || g.out[0].accumulate || g.out[0].add_is_mask || g.lerp.P != nullptr || g.skip_flag != nullptr || g.ksplit != 1) return false;
  if (s0.fmt != FMT_F32 || !s0.wamax || !(s0.amax || s0.amax_static > 0.f)) return false;
  if (s0.tmul != 1 || s0.tdiv != 1 || s0.toff != 0 || s0.Tin != g.Tout || s0.x_cstride != g.Tout || g.Tout % LW_NC != 0 || !s0.vec) return false;
  if (s0.ldw < 2 * LW_ROWS) return false;
  return (long)2 * LW_ROWS * g.Tout * 4 < (1L << 31);      // 32-bit offsets inside a batch item of x_l / x_{l+1}
}

int launch_lin_wide(const GemmArgs& g, int tag, hipStream_t st) {
  const Seg& s0 = g.seg[0];
  LinWideArgs la;
  la.w = reinterpret_cast<const uint4*>(s0.w); la.ldw = s0.ldw;
  la.z = s0.x; la.z_bstride = s0.x_bstride;
  la.add = g.out[0].add; la.add_bstride = g.out[0].add_bstride;
  la.y = g.out[0].y; la.y_bstride = g.out[0].y_bstride;
  la.bias = g.out[0].bias;
  la.T = g.Tout;
  la.wamax = s0.wamax; la.z_amax = s0.amax; la.z_amax_static = s0.amax_static; la.amax_out = g.out[0].amax_out;
  la.add_scale = g.add_scale; la.add_amax = g.add_amax; la.l1 = g.bound_l1; la.scale_out = g.scale_out;
  la.floor_w = g.floor_w; la.floor_p = g.floor_p;
  la.tiles_per_b = g.Tout / LW_NC; la.ntiles = la.tiles_per_b * g.B;
  static int n_cu = 0;
  if (n_cu == 0) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n_cu <= 0) n_cu = 256;
  }
  // one workgroup per CU, in pairs (two row slices per column tile), eight pairs per group of 16 consecutive ids
  int pairs = n_cu / 2 < la.ntiles ? n_cu / 2 : la.ntiles;
  pairs = (pairs + 7) / 8 * 8;
  const dim3 grid((unsigned)(2 * pairs)), block(512);
  launch_tagged(g.out[0].add_fmt != FMT_F32 ? lin256_stream_kernel<true> : lin256_stream_kernel<false>, grid, block, st, tag, la);
  VQ_LAUNCH_CHECK();
  return 0;
}

}  // namespace vq
