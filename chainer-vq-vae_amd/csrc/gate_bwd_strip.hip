// gate_bwd_strip.hip -- the float32x2 gate-derivative GEMM of ResidualNet's chain with the fused latent pull-back
// (launch_gemm<EPI_GATE_BWD>, pre-split gh out, pb_part set, 128 gate channels, [g_res | g_skip] of one shape) as a
// COLUMN-STRIP STREAMING kernel.
//
// The launch is an HBM kernel: gz = Wr^T g_res + Ws^T g_skip is M = 128, K = 512, N = B T -- 16 GFLOP against 504 MB of
// compulsory traffic at configs[1].  conv_gemm_x3_kernel<EPI_GATE_BWD, 2, 1, 2, true, 0, 3> runs it on 128 x 128 tiles:
// 245 VGPRs and 80 KB of LDS, i.e. 8 waves per CU with ~16 KB of loads in flight, and an epilogue (47 % of a workgroup's
// life) that overlaps another tile's loop only by luck.  Here:
//   * a WAVE owns a 32-column strip of time and all 128 rows of gz (4 x 32 x 32 accumulators, 64 VGPRs).  Its
//     activations are private: global -> registers -> split2 -> MFMA B operand (a lane holds the 8 channels of its k-half
//     for its column, which is the fragment layout) -- no LDS image and no barrier for them;
//   * only the weights are shared: the 8 KB of a 16-channel K step ([piece][k-half][row] 16-byte words, the packed
//     slab's own order) go L2 -> registers -> LDS two steps ahead, double-buffered, one barrier per step;
//   * 16 waves per CU (one 1024-thread workgroup = four 128-column tiles, <= 128 VGPRs), every wave with the loads of two
//     K steps in flight: 16 x 64 x 16 x 4 B = 64 KB per CU, four times the tiled kernel's;
//   * the epilogue runs per wave on QUARTER blocks (8 gz rows x 32 columns = 4 accumulator registers): sigma / z of the
//     quarters ahead are requested before a quarter's stores, so a wave keeps 16-24 loads in flight with 8 registers per
//     quarter instead of 128 for the tile.
// K order (g_res | g_skip channel groups interleaved), the three products of a step, the unscaling and the epilogue's
// expressions are conv_gemm_x3_kernel's: gh, its scale words and max |gh| are the same to the last bit.  So are the
// pull-back partials: a quarter's 16 gh rows are transposed through a 2.3 KB LDS patch per wave, a lane sums one row
// against one of the strip's three coefficient columns in column order (the tiled kernel's FMA chain), and the four
// strips of a 128-column tile are added in the tiled kernel's order ((0 + s0) + s1) + ((0 + s2) + s3) when the
// workgroup is done.
#include "gemm_common.h"

namespace vq {

constexpr int GS_WAVES = 16;                     // waves (= 32-column strips) per workgroup: four 128-column tiles
constexpr int GS_LA = 2;                         // epilogue: quarter blocks requested ahead of the one being stored

__global__ __launch_bounds__(64 * GS_WAVES) void gate_bwd_strip_kernel(const GemmArgs a) {
  __shared__ uint4 Ws[2][512];                                                 // one K step of [Wr ; Ws]^T: [piece][k-half][row]
  __shared__ __attribute__((aligned(16))) float pbG[GS_WAVES * 16 * 36];       // per wave: 16 gh rows x 32 t, row pitch 36
  __shared__ __attribute__((aligned(16))) float pbCt[GS_WAVES][3][32];         // per strip: coefficient of column c for position vs + j
  VQ_STAMP(tp0);
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 31, lk = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int logical;
  {                                              // consecutive workgroups of an XCD take consecutive tiles (as conv_gemm_x3_kernel)
    const int nblk = gridDim.x, id = blockIdx.x;
    const int q = nblk >> 3, r = nblk & 7, xcd = id & 7;
    logical = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (id >> 3);
  }
  const int T = a.Tout, Ch = a.M;
  const int ntiles = a.ntile_n * a.B;            // 128-column tiles, batch-major (pb_part's order)
  const int tile_w = 4 * logical + (wave >> 2);
  const bool active = tile_w < ntiles;           // a wave beyond the last tile re-reads the last tile and stores nothing
  const int tile = min(tile_w, ntiles - 1);
  const int b = tile / a.ntile_n;
  const int tt = (tile - b * a.ntile_n) * BN;    // first column of the wave's tile
  const int t0 = tt + 32 * (wave & 3);           // ... and of its strip
  const Seg& s0 = a.seg[0];
  const Seg& s1 = a.seg[1];

  // ---- scales (float32x2): the launch's product scale 2^(28 - emax), each segment's activation scale, the bound gh is
  // stored under -- conv_gemm_x3_kernel's read_scales for a two-tap launch, word for word
  const unsigned ax0 = s0.amax ? amax_load(s0.amax) : __builtin_bit_cast(unsigned, s0.amax_static);
  const unsigned aw0 = amax_load(s0.wamax);
  const unsigned ax1 = s1.amax ? amax_load(s1.amax) : __builtin_bit_cast(unsigned, s1.amax_static);
  const unsigned aw1 = amax_load(s1.wamax);
  const int emax = max(amax_expo(aw0) + amax_expo(ax0), amax_expo(aw1) + amax_expo(ax1));
  const int kx0 = 14 - emax + amax_expo(aw0), kx1 = 14 - emax + amax_expo(aw1);
  int kout;
  {
    float bound = a.bound_l1[0] * __builtin_bit_cast(float, ax0) + a.bound_l1[1] * __builtin_bit_cast(float, ax1);
    bound = bound_margin(bound);
    kout = 14 - amax_expo(__builtin_bit_cast(unsigned, bound));
    scale_publish(a.scale_out, bound);
  }

  // ---- the strip's pull-back coefficients (column li): position offset 0 or 1 against the strip's first column
  if (lk == 0) {
    const int dv = a.lerp.v0[t0 + li] - a.lerp.v0[t0];
    const float c0 = a.lerp.w0[t0 + li], c1 = a.lerp.w1[t0 + li];
    pbCt[wave][0][li] = dv == 0 ? c0 : 0.f;
    pbCt[wave][1][li] = dv == 0 ? c1 : c0;
    pbCt[wave][2][li] = dv == 0 ? 0.f : c1;
  }

  // ---- fetch state.  Activations: a buffer descriptor per segment (extent = cin rows: nothing is read beyond), a lane
  // offset for (channel 8 lk, column t0 + li) and a wave-uniform offset per channel.  Weights: thread `tid` owns 8 bytes
  // of a step's 8 KB image
  const int ncg = s0.cin / BK;                   // channel groups = K steps per segment
  const unsigned xcsb = 4u * (unsigned)s0.x_cstride, xadvb = (unsigned)BK * xcsb;
  const rsrc_t rx0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(reinterpret_cast<const char*>(s0.x) + (long)b * s0.x_bstride * 4), 0,
                                                       (int)((unsigned)s0.cin * xcsb), 0x00020000);
  const rsrc_t rx1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(reinterpret_cast<const char*>(s1.x) + (long)b * s1.x_bstride * 4), 0,
                                                       (int)((unsigned)s1.cin * xcsb), 0x00020000);
  const unsigned vb = 4u * (unsigned)(8 * lk * s0.x_cstride + t0 + li);
  const rsrc_t rw = make_rsrc(s0.w);
  const unsigned wadvb = 64u * (unsigned)s0.ldw;                                 // a step: 2 pieces x 2 k-halves of ldw 16-byte words
  const unsigned sw1 = (unsigned)(reinterpret_cast<const char*>(s1.w) - reinterpret_cast<const char*>(s0.w));
  const unsigned vw = 16u * (unsigned)((tid >> 8) * s0.ldw + ((tid >> 1) & 127)) + 8u * (unsigned)(tid & 1);
  auto fetch_b = [&](float (&bv)[8], const rsrc_t rx, const int cg) {
    const unsigned sx = (unsigned)cg * xadvb;
#pragma unroll
    for (int e = 0; e < 8; ++e) bv[e] = buf_ld(rx, vb, sx + (unsigned)e * xcsb);
  };
  auto fetch_w = [&](const int cg, const bool seg1) -> uint2 {
    return __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(rw, vw, (unsigned)cg * wadvb + (seg1 ? sw1 : 0u), 0));
  };

  f32x16 acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  // one K step: split the arrived activations, request the same segment's next channel group into the freed registers,
  // then 4 row blocks x 3 products against the weight image (conv_gemm_x3_kernel's mfma_chain order)
  auto step = [&](float (&bv)[8], const rsrc_t rx, const int kx, const int cg_next, const uint4* wimg) {
    unsigned h[4], l[4];
#pragma unroll
    for (int e = 0; e < 8; e += 2) split2(bv[e], bv[e + 1], kx, h[e / 2], l[e / 2]);
    const uint4 bf[2] = {make_uint4(h[0], h[1], h[2], h[3]), make_uint4(l[0], l[1], l[2], l[3])};
    fetch_b(bv, rx, cg_next);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint4 af[2] = {wimg[lk * 128 + 32 * i + li], wimg[(2 + lk) * 128 + 32 * i + li]};
      acc[i] = mfma_chain<2>(af, bf, acc[i]);
    }
  };

  VQ_STAMP(tp1);
  {
    float pb[8], qb[8];                          // P: g_res (even steps), Q: g_skip (odd steps)
    uint2 wp, wq;
    fetch_b(pb, rx0, 0);
    wp = fetch_w(0, false);
    fetch_b(qb, rx1, 0);
    wq = fetch_w(0, true);
    reinterpret_cast<uint2*>(Ws[0])[tid] = wp;
    wp = fetch_w(min(1, ncg - 1), false);
    __syncthreads();
    for (int cg = 0; cg < ncg; ++cg) {
      const int c1 = min(cg + 1, ncg - 1), c2 = min(cg + 2, ncg - 1);      // past the end: re-read the last group, never used
      step(pb, rx0, kx0, c1, Ws[0]);
      reinterpret_cast<uint2*>(Ws[1])[tid] = wq;
      wq = fetch_w(c1, true);
      __syncthreads();
      step(qb, rx1, kx1, c1, Ws[1]);
      reinterpret_cast<uint2*>(Ws[0])[tid] = wp;
      wp = fetch_w(c2, false);
      __syncthreads();
    }
  }
  VQ_STAMP(tp2);
  const int ku = emax - 28;                      // back from the launch's product scale, register by register where it is used

  // ---- epilogue, quarter block by quarter block: Q = 0 .. 15 holds gz rows 8 Q + 4 lk + j (accumulator registers
  // 4 (Q & 3) + j of row block Q >> 2), column t0 + li
  const OutR& od = a.out[0];
  const bool gsig = a.gsig != 0;
  const unsigned sQ = 4u * (unsigned)(Ch * T);
  const rsrc_t rGt = make_rsrc(od.add + (long)b * od.add_bstride);
  const rsrc_t rZs = make_rsrc(gsig ? a.zsrc + (long)b * Ch * T : od.add + (long)b * od.add_bstride);      // gsig: z (B, Ch, T) in tanh's place
  // (a wave beyond the last tile gets a descriptor of extent 0: its stores are dropped, no branch around them)
  const rsrc_t rGh = __builtin_amdgcn_make_buffer_rsrc(od.y + (long)b * od.y_bstride, 0, active ? (int)(2u * sQ) : 0, 0x00020000);
  const unsigned voff = 4u * (unsigned)(4 * lk * T + t0 + li);
  float* const gw = pbG + wave * (16 * 36);
  const int prow = lane & 15, pj = lane >> 4;    // pull-back role: gh row of the quarter x position (pj == 3: idle)
  const float* const grow = gw + prow * 36;
  const float* const crow = &pbCt[wave][min(pj, 2)][0];
  float am = 0.f;
  // (named register sets and sums, expanded by hand: hipcc leaves [16][4] arrays indexed through an unrolled loop in scratch)
#define GS_LOAD(Qv, TA, SB)                                                                                      \
  _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                                 \
    const unsigned so = 4u * (unsigned)((8 * (Qv) + j) * T);                                                      \
    TA[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rZs, voff, so, X3_GBWD_LD_AUX));       \
    SB[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rGt, voff, so + sQ, X3_GBWD_LD_AUX));  \
  }
  // one quarter: (request quarter Qv + GS_LA into the set freed last,) both gate derivatives from the 4 gz registers, the
  // patch, the pre-split stores; then the quarter's pull-back: rows 0..7 = ga of z channels 8 Qv .., rows 8..15 = gb;
  // lane (prow, pj) sums row prow against the coefficients of position vs + pj over the strip's 32 columns, in column order
#define GS_QUARTER(Qv, TA, SB, TAN, SBN, PS)                                                                     \
  {                                                                                                               \
    __builtin_amdgcn_sched_barrier(0);        /* (keeps hipcc from gathering several quarters' loads and LDS reads: it spilled the accumulators for them) */ \
    if ((Qv) + GS_LA < 16) { GS_LOAD((Qv) + GS_LA, TAN, SBN) }                                                    \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                               \
      __builtin_amdgcn_sched_barrier(0);                                                                          \
      const float gz = __builtin_ldexpf(acc[(Qv) >> 2][4 * ((Qv) & 3) + j], ku);                                  \
      const float sv = SB[j];                                                                                     \
      const float tv = gsig ? TA[j] * __builtin_amdgcn_rcpf(fmaxf(sv, 1e-30f)) : TA[j];      /* gsig: tanh = z / sigmoid */ \
      const float ga = gz * sv * (1.f - tv * tv), gb = gz * tv * sv * (1.f - sv);                                 \
      gw[(4 * lk + j) * 36 + li] = ga;                                                                            \
      gw[(8 + 4 * lk + j) * 36 + li] = gb;                                                                        \
      am = fmaxf(am, fmaxf(fabsf(ga), fabsf(gb)));                                                                \
      unsigned da, db;                                                                                            \
      presplit_pair(ga, gb, kout, da, db);                                                                        \
      const unsigned so = 4u * (unsigned)((8 * (Qv) + j) * T);                                                    \
      __builtin_amdgcn_raw_buffer_store_b32((int)da, rGh, voff, so, X3_GBWD_ST_AUX);                              \
      __builtin_amdgcn_raw_buffer_store_b32((int)db, rGh, voff, so + sQ, X3_GBWD_ST_AUX);                         \
    }                                                                                                             \
    float s = 0.f;                                                                                                \
    _Pragma("unroll") for (int q = 0; q < 8; ++q) {                                                               \
      __builtin_amdgcn_sched_barrier(0);                                                                          \
      const float4 g4 = *reinterpret_cast<const float4*>(grow + 4 * q);                                           \
      const float4 c4 = *reinterpret_cast<const float4*>(crow + 4 * q);                                           \
      s = fmaf(g4.x, c4.x, s); s = fmaf(g4.y, c4.y, s); s = fmaf(g4.z, c4.z, s); s = fmaf(g4.w, c4.w, s);         \
    }                                                                                                             \
    if ((Qv) < 4) wsum[64 * (Qv)] = s; else PS = s;      /* the first four sums wait in the dead weight image: registers are shortest here */ \
  }
  static_assert(GS_LA == 2, "the expansion below rotates three register sets");
  float ta0[4], sb0[4], ta1[4], sb1[4], ta2[4], sb2[4];
  float* const wsum = reinterpret_cast<float*>(&Ws[0][0]) + 256 * wave + lane;      // (every wave is behind the K loop's last barrier)
  [[maybe_unused]] float ps0 = 0.f, ps1 = 0.f, ps2 = 0.f, ps3 = 0.f;      // (the macro names a register for every quarter)
  float ps4, ps5, ps6, ps7, ps8, ps9, ps10, ps11, ps12, ps13, ps14, ps15;
  GS_LOAD(0, ta0, sb0)
  GS_LOAD(1, ta1, sb1)
  GS_QUARTER(0, ta0, sb0, ta2, sb2, ps0)
  GS_QUARTER(1, ta1, sb1, ta0, sb0, ps1)
  GS_QUARTER(2, ta2, sb2, ta1, sb1, ps2)
  GS_QUARTER(3, ta0, sb0, ta2, sb2, ps3)
  GS_QUARTER(4, ta1, sb1, ta0, sb0, ps4)
  GS_QUARTER(5, ta2, sb2, ta1, sb1, ps5)
  GS_QUARTER(6, ta0, sb0, ta2, sb2, ps6)
  GS_QUARTER(7, ta1, sb1, ta0, sb0, ps7)
  GS_QUARTER(8, ta2, sb2, ta1, sb1, ps8)
  GS_QUARTER(9, ta0, sb0, ta2, sb2, ps9)
  GS_QUARTER(10, ta1, sb1, ta0, sb0, ps10)
  GS_QUARTER(11, ta2, sb2, ta1, sb1, ps11)
  GS_QUARTER(12, ta0, sb0, ta2, sb2, ps12)
  GS_QUARTER(13, ta1, sb1, ta0, sb0, ps13)
  GS_QUARTER(14, ta2, sb2, ta1, sb1, ps14)
  GS_QUARTER(15, ta0, sb0, ta2, sb2, ps15)
#undef GS_QUARTER
#undef GS_LOAD
  VQ_STAMP(tp3);

  // ---- the tile's partials: [column half][tile of the workgroup][gh channel][position], zeroed, then the even strips
  // of every half, then the odd ones (conv_gemm_x3_kernel: tp[off + j] += s_j, sub-tile 0 before sub-tile 1), then
  // half 0 + half 1.  The image takes the place of the waves' patches.
  float* const H = pbG;
  __syncthreads();
  for (int i = tid; i < 2 * 4 * 2 * Ch * 4; i += 64 * GS_WAVES) H[i] = 0.f;
  __syncthreads();
  const int pb_off = a.lerp.v0[t0] - a.lerp.v0[tt];          // 0 .. 2: the strip's first position among the tile's four
  float* const hp = H + ((((wave >> 1) & 1) * 4 + (wave >> 2)) * (2 * Ch) + (prow >> 3) * Ch + (prow & 7)) * 4 + pb_off + pj;
#pragma unroll
  for (int odd = 0; odd < 2; ++odd) {
    if ((wave & 1) == odd && active && pj < 3 && pb_off + pj < 4) {
      hp[0] += wsum[0]; hp[32] += wsum[64]; hp[64] += wsum[128]; hp[96] += wsum[192]; hp[128] += ps4; hp[160] += ps5; hp[192] += ps6; hp[224] += ps7;
      hp[256] += ps8; hp[288] += ps9; hp[320] += ps10; hp[352] += ps11; hp[384] += ps12; hp[416] += ps13; hp[448] += ps14; hp[480] += ps15;      // gh channel 8 Q + ..
    }
    __syncthreads();
  }
  for (int i = tid; i < 4 * 2 * Ch * 4; i += 64 * GS_WAVES) {
    const int tl = 4 * logical + i / (2 * Ch * 4);
    if (tl < ntiles) a.pb_part[(long)4 * logical * (2 * Ch * 4) + i] = H[i] + H[4 * 2 * Ch * 4 + i];
  }
  // max |gh| of the workgroup -> one slot (amax_commit, with the shuffle addresses taken afresh: shared with amax_load's in
  // the prologue they stayed live -- spilled -- across the whole kernel)
  if (od.amax_out != nullptr) {
    float* const red = H;                        // (the pull-back image has been read: the barrier below orders it)
    int ll = lane;
    asm volatile("" : "+v"(ll));
    float m = active ? am : 0.f;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((ll ^ o) << 2, __builtin_bit_cast(int, m))));
    __syncthreads();
    if (ll == 0) red[wave] = m;
    __syncthreads();
    if (tid == 0) {
      for (int i = 1; i < GS_WAVES; ++i) m = fmaxf(m, red[i]);
      m *= PRESPLIT_AMAX_UP;                     // gh is stored pre-split: cover what it decodes to
      atomicMax(od.amax_out + (blockIdx.x & (AMAX_SLOTS - 1)), __builtin_bit_cast(unsigned, m));
    }
  }
#ifdef VQ_PHASE_TIMING
  if (lane == 0) {                               // per WAVE: prologue / K loop / epilogue ticks, [4] counts waves
    atomicAdd(&g_phase[EPI_GATE_BWD][0], (unsigned long long)(tp1 - tp0));
    atomicAdd(&g_phase[EPI_GATE_BWD][1], (unsigned long long)(tp2 - tp1));
    atomicAdd(&g_phase[EPI_GATE_BWD][3], (unsigned long long)(tp3 - tp2));
    atomicAdd(&g_phase[EPI_GATE_BWD][4], 1ull);
  }
#endif
}

// the launches the strip kernel serves: float32x2, [g_res | g_skip] of one shape over whole K steps, 128 gate channels,
// plain fp32 operands, gh stored pre-split, the pull-back fused (which brings T % 128 == 0 and the resize tables)
bool gate_bwd_strip_shape(const GemmArgs& g) {
  if (g.nseg != 2 || g.M != 128 || g.Tout % BN != 0 || g.B <= 0) return false;
  if (g.out[0].y_fmt != FMT_F16X2 || !g.pb_part || !g.bound_l1 || !g.scale_out || !g.lerp.v0 || !g.lerp.w0 || !g.lerp.w1) return false;
  if (g.seg[0].fmt != FMT_F32 || g.seg[1].fmt != FMT_F32 || g.out[0].add_fmt != FMT_F32 || g.skip_flag || g.ksplit != 1 || (g.gsig && !g.zsrc)) return false;
  const Seg& s0 = g.seg[0];
  const Seg& s1 = g.seg[1];
  if (s0.cin != s1.cin || s0.cin % BK != 0 || s0.cin <= 0 || s0.ldw != s1.ldw || s0.ldw < 128) return false;
  for (int i = 0; i < 2; ++i) {
    const Seg& s = g.seg[i];
    if (s.tmul != 1 || s.tdiv != 1 || s.toff != 0 || s.Tin != g.Tout || s.x_cstride != s0.x_cstride || s.x_cstride < g.Tout) return false;
    if (!s.wamax || !(s.amax || s.amax_static > 0.f)) return false;
  }
  if (s1.w < s0.w || reinterpret_cast<const char*>(s1.w) - reinterpret_cast<const char*>(s0.w) >= (1L << 30)) return false;
  return (long)2 * g.M * g.Tout * 4 < (1L << 31);          // 32-bit offsets inside a batch item of the gates and of gh
}

int launch_gate_bwd_strip(const GemmArgs& g, int tag, hipStream_t st) {
  const unsigned grid = (unsigned)cdiv(g.ntile_n * g.B, 4);
  launch_tagged(gate_bwd_strip_kernel, dim3(grid), dim3(64 * GS_WAVES), st, tag, g);
  VQ_LAUNCH_CHECK();
  return 0;
}

}  // namespace vq
