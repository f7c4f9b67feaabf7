// misc.hip -- HBM-bound kernels of the path: element-wise Variable arithmetic,
// reductions, align-corners up-sampling, speaker-embedding broadcast, fused
// softmax cross-entropy, Adam and EMA over flat arenas.  All are grid-stride,
// coalesced along the contiguous time axis; fp32 ops that the NumPy path rounds
// individually use the _rn intrinsics so hipcc cannot contract them into FMAs.
#include "common.h"

namespace vq {

static inline int grid_for(size_t n, int block = 256, int cap = 2048) {
  size_t g = (n + block - 1) / block;
  if (g > (size_t)cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

__global__ void ew_kernel(int op, size_t n, const float* __restrict__ a, const float* __restrict__ b,
                          float* __restrict__ out, float alpha, float beta) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x) {
    float v;
    switch (op) {
      case VQVAE_EW_ADD: v = __fadd_rn(a[i], b[i]); break;
      case VQVAE_EW_SUB: v = __fsub_rn(a[i], b[i]); break;
      case VQVAE_EW_MUL: v = __fmul_rn(a[i], b[i]); break;
      case VQVAE_EW_AXPBY: v = __fadd_rn(__fmul_rn(alpha, a[i]), __fmul_rn(beta, b[i])); break;
      case VQVAE_EW_SCALE: v = __fmul_rn(alpha, a[i]); break;
      case VQVAE_EW_SQUARE: v = __fmul_rn(a[i], a[i]); break;
      case VQVAE_EW_RELU: v = fmaxf(a[i], 0.f); break;
      case VQVAE_EW_RELU_BWD: v = b[i] > 0.f ? a[i] : 0.f; break;
      case VQVAE_EW_FILL: v = alpha; break;
      case VQVAE_EW_MUL_SCALAR_DEV: v = __fmul_rn(__fmul_rn(a[i], b[0]), alpha); break;
      default: v = 0.f;
    }
    out[i] = v;
  }
}

__device__ __forceinline__ float block_sum_256(float v, float* sh) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[w] = v;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}

__global__ __launch_bounds__(256) void sum_stage1(const float* __restrict__ x, size_t n, float* partial) {
  __shared__ float sh[4];
  float acc = 0.f;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x) acc += x[i];
  const float t = block_sum_256(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = t;
}
__global__ __launch_bounds__(256) void sum_stage2(const float* __restrict__ partial, int np, float scale, float* out) {
  __shared__ float sh[4];
  float acc = 0.f;
  for (int i = threadIdx.x; i < np; i += 256) acc += partial[i];
  const float t = block_sum_256(acc, sh);
  if (threadIdx.x == 0) out[0] = t * scale;
}

// ---- mean((a - b)^2) as one node (net.py:90-91: the codebook and commitment losses; as Variable arithmetic each was
// sub, square, two-stage sum forward and fill, scale, mul, scale, negate backward).  Same roundings in the same order as
// that chain: d = fl(a - b), fl(d d) summed by the two-stage sum; backward fl(fl(fl(fl(1/n) g) d) 2).
__global__ __launch_bounds__(256) void sqdiff_stage1(const float* __restrict__ a, const float* __restrict__ b, size_t n, float* partial) {
  __shared__ float sh[4];
  float acc = 0.f;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float d = __fsub_rn(a[i], b[i]);
    acc += __fmul_rn(d, d);
  }
  const float t = block_sum_256(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = t;
}
__global__ void sqdiff_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ g, size_t n,
                                  float invn, float* __restrict__ ga, float* __restrict__ gb) {
  const float gm = __fmul_rn(invn, g[0]);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float v = __fmul_rn(__fmul_rn(gm, __fsub_rn(a[i], b[i])), 2.f);
    if (ga) ga[i] = v;
    if (gb) gb[i] = -v;
  }
}

// ---- up-sampling ---------------------------------------------------------
__global__ void upsample_fwd_kernel(const float* __restrict__ x, int B, int C, int Tin, int Tout,
                                    const int32_t* __restrict__ v0, const int32_t* __restrict__ v1,
                                    const float* __restrict__ w0, const float* __restrict__ w1,
                                    float* __restrict__ y, long y_bstride) {
  const long total = (long)B * C * Tout;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const int t = (int)(i % Tout);
    const long r = i / Tout;
    const int c = (int)(r % C);
    const long b = r / C;
    const float* xr = x + (b * C + c) * (long)Tin;
    y[b * y_bstride + (long)c * Tout + t] =
        __fadd_rn(__fmul_rn(w0[t], xr[v0[t]]), __fmul_rn(w1[t], xr[v1[t]]));
  }
}

__global__ void upsample_bwd_kernel(const float* __restrict__ gy, long gy_bstride, int B, int C,
                                    int Tin, int Tout, const float* __restrict__ w0,
                                    const float* __restrict__ w1, const int32_t* __restrict__ lo0,
                                    const int32_t* __restrict__ hi0, const int32_t* __restrict__ lo1,
                                    const int32_t* __restrict__ hi1, float* __restrict__ gx,
                                    long gx_bstride) {
  const long total = (long)B * C * Tin;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const int v = (int)(i % Tin);
    const long r = i / Tin;
    const int c = (int)(r % C);
    const long b = r / C;
    const float* g = gy + b * gy_bstride + (long)c * Tout;
    double acc = 0.0;     // numpy.bincount(weights=...) accumulates in float64
    for (int t = lo0[v]; t < hi0[v]; ++t) acc += (double)__fmul_rn(g[t], w0[t]);
    for (int t = lo1[v]; t < hi1[v]; ++t) acc += (double)__fmul_rn(g[t], w1[t]);
    gx[b * gx_bstride + (long)c * Tin + v] = (float)acc;
  }
}

// one workgroup per (b,c) row: the weighted row (g*w0 | g*w1) is staged through LDS with coalesced
// 16-B loads, then every output v = sum_{t in R1(v)} g*w1 + sum_{t in R0(v)} g*w0 (two adjacent ranges of
// ~Tout/Tin elements) is summed in float64 by a FIXED-ORDER tree over eight lanes: four lanes per range,
// lane q taking elements q, q+4, ... in ascending order with two interleaved accumulators, combined as
// ((q0+q1)+(q2+q3)) per range and then range0 + range1 by three butterfly shuffles -- deterministic, and
// Tin*8 = 960 short chains on 1024 threads instead of round 2's 240 chains of ~64 on 256 threads (2 waves
// per SIMD could not hide the LDS latency of a serial chain: 2.7 TB/s).  Workgroups are persistent, two
// per CU (64 VGPRs), the NEXT row's loads are in flight while the current row is summed.  (The decoder's
// 64x pull-back takes upsample_bwd_seg_kernel below; this form serves the small ratios.)
constexpr int UPB_NT = 1024, UPB_KV = 2;      // threads, float4 per thread and pass
__global__ __launch_bounds__(UPB_NT, 8) void upsample_bwd_rows_kernel(
    const float* __restrict__ gy, long gy_bstride, int B, int C, int Tin, int Tout,
    const float* __restrict__ w0, const float* __restrict__ w1, const int32_t* __restrict__ lo0,
    const int32_t* __restrict__ hi0, const int32_t* __restrict__ lo1,
    const int32_t* __restrict__ hi1, float* __restrict__ gx, long gx_bstride) {
  // [2][Tpad] products at index t + (t >> 3): one pad word per 8 elements makes both access patterns
  // conflict-free -- the staging writes (lane stride 4 t -> 4.5 words) and the range sums (the four lanes
  // of a range read 4 consecutive t, the ranges of a wave sit ~64.5 t = 72.6 words apart).
  extern __shared__ float sm[];
  const int Tpad = Tout + (Tout >> 3) + 8;
  float* r0 = sm;
  float* r1 = sm + Tpad;
  const int rows = B * C;
  const int tid = threadIdx.x;
  const bool vec = (Tout % 4 == 0) && (gy_bstride % 4 == 0) && (((uintptr_t)gy) % 16 == 0) &&
                   (((uintptr_t)w0) % 16 == 0) && (((uintptr_t)w1) % 16 == 0);
  const int n4 = Tout >> 2;
  const bool pipe = vec && n4 <= UPB_NT * UPB_KV;       // a whole row in one pass of UPB_KV float4 per thread
  float4 v[UPB_KV];
  auto fetch = [&](int r) {
    const int b = r / C, c = r % C;
    const float* g = gy + (long)b * gy_bstride + (long)c * Tout;
#pragma unroll
    for (int k = 0; k < UPB_KV; ++k) {
      const int q = k * UPB_NT + tid;
      v[k] = q < n4 ? reinterpret_cast<const float4*>(g)[q] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto stage4 = [&](int q, const float4 gv, const float4 a, const float4 bq) {   // products of 4 consecutive t -> LDS
    const int t = q << 2;
    const int o = t + (t >> 3);                  // 4 consecutive t never straddle an 8-block
    r0[o] = __fmul_rn(gv.x, a.x); r0[o + 1] = __fmul_rn(gv.y, a.y);
    r0[o + 2] = __fmul_rn(gv.z, a.z); r0[o + 3] = __fmul_rn(gv.w, a.w);
    r1[o] = __fmul_rn(gv.x, bq.x); r1[o + 1] = __fmul_rn(gv.y, bq.y);
    r1[o + 2] = __fmul_rn(gv.z, bq.z); r1[o + 3] = __fmul_rn(gv.w, bq.w);
  };
  // this thread's share of the sums: output (tid >> 3) [+ UPB_NT/8 per pass], range (tid >> 2) & 1
  // (0: the w1 range, which comes first in t; 1: the w0 range), lane (tid & 3) of the range
  const int npass = (Tin * 8 + UPB_NT - 1) / UPB_NT;
  if (pipe && blockIdx.x < rows) fetch(blockIdx.x);
  for (int r = blockIdx.x; r < rows; r += gridDim.x) {
    const int b = r / C, c = r % C;
    const float* g = gy + (long)b * gy_bstride + (long)c * Tout;
    __syncthreads();
    if (pipe) {
#pragma unroll
      for (int k = 0; k < UPB_KV; ++k) {
        const int q = k * UPB_NT + tid;
        if (q < n4) stage4(q, v[k], reinterpret_cast<const float4*>(w0)[q], reinterpret_cast<const float4*>(w1)[q]);
      }
    } else if (vec) {
      for (int q = tid; q < n4; q += UPB_NT)
        stage4(q, reinterpret_cast<const float4*>(g)[q], reinterpret_cast<const float4*>(w0)[q], reinterpret_cast<const float4*>(w1)[q]);
    } else {
      for (int t = tid; t < Tout; t += UPB_NT) {
        const float vv = g[t];
        r0[t + (t >> 3)] = __fmul_rn(vv, w0[t]);
        r1[t + (t >> 3)] = __fmul_rn(vv, w1[t]);
      }
    }
    __syncthreads();
    if (pipe && r + (int)gridDim.x < rows) fetch(r + gridDim.x);      // in flight during the sums below
    for (int p = 0; p < npass; ++p) {          // wave-uniform trip count: the shuffles need all eight lanes
      const int vi = (p * UPB_NT + tid) >> 3, part0 = (tid >> 2) & 1, qt = tid & 3;
      const bool ok = vi < Tin;
      const int vc = ok ? vi : 0;
      const float* rr = part0 ? r0 : r1;
      const int lo = part0 ? lo0[vc] : lo1[vc];
      const int hi = ok ? (part0 ? hi0[vc] : hi1[vc]) : lo;
      int t = lo + qt;
      double a0 = 0.0, a1 = 0.0;
      for (; t + 4 < hi; t += 8) {
        a0 += (double)rr[t + (t >> 3)];
        a1 += (double)rr[t + 4 + ((t + 4) >> 3)];
      }
      if (t < hi) a0 += (double)rr[t + (t >> 3)];
      double sacc = a0 + a1;
      sacc += __shfl_xor(sacc, 1, 64);       // (q0+q1) | (q2+q3)
      sacc += __shfl_xor(sacc, 2, 64);       // (q0+q1)+(q2+q3): fp64 addition commutes, all four lanes agree
      sacc += __shfl_xor(sacc, 4, 64);       // w1-range sum + w0-range sum
      if (ok && (tid & 7) == 0) gx[(long)b * gx_bstride + (long)c * Tin + vi] = (float)sacc;
    }
  }
}

// The decoder's latent pull-back (Tout >= 8 Tin, e.g. 7680 -> 120; 21 launches per configs[1] step) without
// staging the row: every thread keeps its 4 consecutive t (one 16-B load, next row prefetched) and its
// interpolation weights in registers, multiplies, and reduces its four products to at most two partial
// sums per weight -- "lo" (the elements that share the source index v0 of its first element) and "hi"
// (the rest: the next source index; nonzero for the ~Tin threads that straddle a boundary).  The
// partials go to LDS (16 B per thread instead of 32 B per 4 elements), and output v is the sum of the
// ~Tout/(4 Tin) lo partials of its w0 range, the one hi partial below it, and the same for the w1
// range -- eight lanes per v (four per range, lane j taking partials j, j+4, ... in ascending order),
// combined by three butterfly shuffles: a FIXED-ORDER fp32 tree (4 -> ~17 -> 2), deterministic, within a few
// ulp of the float64 sum.  LDS is double-buffered by row parity: one barrier per row.  ~30
// instructions per thread and row against ~150 for the LDS-staged float64 form above.
// IN16: gy is stored as bf16 (the bf16 mode's gh, vqvae_upsample_linear_bwd_bf16): 8-byte loads of 4 t, widened in
// registers; gy_bstride counts elements either way.
constexpr int UPS_NT = 1024, UPS_PITCH = 2048 + 128;
// IN16 = 2: gy is stored PRE-SPLIT (matmul mode 3, VQVAE_STORE_GH_F16X2: one dword per element = fp16 hi | fp16 lo << 16 of
// gy * 2^k, k from the bound in its `scale` words): hi + lo is exact in fp32 and the pull-back is linear, so the rows are
// summed as they are and the weights carry the 2^-k.
template <int IN16>
__global__ __launch_bounds__(UPS_NT, 8) void upsample_bwd_seg_kernel(
    const float* __restrict__ gy, long gy_bstride, int B, int C, int Tin, int Tout,
    const float* __restrict__ w0, const float* __restrict__ w1, const int32_t* __restrict__ lo0,
    const int32_t* __restrict__ hi0, const int32_t* __restrict__ lo1,
    const int32_t* __restrict__ hi1, float* __restrict__ gx, long gx_bstride, const uint32_t* __restrict__ scale,
    int L, long gy_lstride, long gx_lstride) {
  // L > 1: the rows of L tensors in one launch (vqvae_upsample_linear_bwd_blocks: every block's gh of a ResidualNet at
  // once); tensor l starts gy_lstride elements (of gy's element type) / gx_lstride floats behind tensor l - 1
  __shared__ float S[2][4][UPS_PITCH];       // [row parity][w0 lo, w0 hi, w1 lo, w1 hi][q + (q >> 4)]
  const int tid = threadIdx.x, n4 = Tout >> 2, rows = L * B * C;
  // phase-1 constants: weights and the lo / hi split point of this thread's column groups q = tid, tid + 1024
  float4 wa[2], wb[2];
  int ks[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int q = k * UPS_NT + tid;
    const bool ok = q < n4;
    wa[k] = ok ? reinterpret_cast<const float4*>(w0)[q] : make_float4(0.f, 0.f, 0.f, 0.f);
    wb[k] = ok ? reinterpret_cast<const float4*>(w1)[q] : make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (IN16 == 2) {                 // the stored values are gy * 2^(14 - e): an exact power of two, folded into the weights
      unsigned mx = 0u;
      for (int i = 0; i < 16; ++i) mx = max(mx, scale[i]);
      const int e = (int)((mx >> 23) & 0xffu);
      const int kinv = ((e < 1 ? 1 : e) - 127) - 14;
      wa[k] = make_float4(ldexpf(wa[k].x, kinv), ldexpf(wa[k].y, kinv), ldexpf(wa[k].z, kinv), ldexpf(wa[k].w, kinv));
      wb[k] = make_float4(ldexpf(wb[k].x, kinv), ldexpf(wb[k].y, kinv), ldexpf(wb[k].z, kinv), ldexpf(wb[k].w, kinv));
    }
    // source index of element 4q: the v whose w0 range [lo0[v], hi0[v]) holds it (the ranges tile [0, Tout)
    // in order); floor(t (Tin-1) / (Tout-1)) is right to within one -- three independent table reads
    // settle it (a binary search here was seven dependent L2 round trips before the first row)
    const int t = ok ? 4 * q : 0;
    const int e = min(max((int)(((long)t * (Tin - 1)) / (Tout - 1)), 1), Tin - 2);
    const int hm = hi0[e - 1], h0 = hi0[e], hp = hi0[min(e + 1, Tin - 1)];
    const int hend = t < hm ? hm : (t < h0 ? h0 : hp);
    ks[k] = max(1, min(4, hend - t));
  }
  // phase-2 constants: output vi = tid >> 3 (+ 128 per pass), range (tid >> 2) & 1, lane tid & 3
  const int npass = (Tin * 8 + UPS_NT - 1) / UPS_NT;
  const int part = (tid >> 2) & 1, j4 = tid & 3;
  // the loads of rows r + stride and r + 2 stride are in flight while row r is reduced (rotating register
  // sets; with the row loop unrolled by two instead the kernel needs > 64 registers, i.e. one workgroup
  // per CU: measured 53 us against 34)
  float4 va[2], vb[2];
#define UPS_FETCH(V, R)                                                                        \
  {                                                                                            \
    const int rr_ = min((R), rows - 1);           /* past the end: re-read the last row, unused */ \
    const int lb_ = rr_ / C;                                                                   \
    const long e_ = (long)(lb_ / B) * gy_lstride + (long)(lb_ % B) * gy_bstride + (long)(rr_ % C) * Tout; \
    const float* g_ = gy + e_;                                                                 \
    const unsigned short* h_ = reinterpret_cast<const unsigned short*>(gy) + e_;               \
    _Pragma("unroll") for (int k = 0; k < 2; ++k) {                                            \
      const int q = k * UPS_NT + tid;                                                          \
      if constexpr (IN16 == 2) {                                                               \
        typedef _Float16 h2_t_ __attribute__((ext_vector_type(2)));                            \
        const uint4 u_ = q < n4 ? reinterpret_cast<const uint4*>(g_)[q] : make_uint4(0u, 0u, 0u, 0u); \
        const h2_t_ a_ = __builtin_bit_cast(h2_t_, u_.x), b_ = __builtin_bit_cast(h2_t_, u_.y), c_ = __builtin_bit_cast(h2_t_, u_.z), d_ = __builtin_bit_cast(h2_t_, u_.w); \
        V[k] = make_float4((float)a_[0] + (float)a_[1], (float)b_[0] + (float)b_[1], (float)c_[0] + (float)c_[1], (float)d_[0] + (float)d_[1]); \
      } else                                                                                   \
      if constexpr (IN16 == 1) {                                                               \
        const uint2 u_ = q < n4 ? reinterpret_cast<const uint2*>(h_)[q] : make_uint2(0u, 0u);  \
        V[k] = make_float4(__builtin_bit_cast(float, u_.x << 16), __builtin_bit_cast(float, u_.x & 0xffff0000u), \
                           __builtin_bit_cast(float, u_.y << 16), __builtin_bit_cast(float, u_.y & 0xffff0000u)); \
      } else V[k] = q < n4 ? reinterpret_cast<const float4*>(g_)[q] : make_float4(0.f, 0.f, 0.f, 0.f); \
    }                                                                                          \
  }
#define UPS_ROW(V, PAR)                                                                        \
  {                                                                                            \
    const int lb = r / C, c = r % C;                                                           \
    const long gxo = (long)(lb / B) * gx_lstride + (long)(lb % B) * gx_bstride + (long)c * Tin; \
    float (*Sp)[UPS_PITCH] = S[PAR];                                                           \
    _Pragma("unroll") for (int k = 0; k < 2; ++k) {                                            \
      const int q = k * UPS_NT + tid;                                                          \
      if (q < n4) {                                                                            \
        const float p0[4] = {__fmul_rn(V[k].x, wa[k].x), __fmul_rn(V[k].y, wa[k].y), __fmul_rn(V[k].z, wa[k].z), __fmul_rn(V[k].w, wa[k].w)}; \
        const float p1[4] = {__fmul_rn(V[k].x, wb[k].x), __fmul_rn(V[k].y, wb[k].y), __fmul_rn(V[k].z, wb[k].z), __fmul_rn(V[k].w, wb[k].w)}; \
        float l0, h0 = 0.f, l1, h1 = 0.f;                                                      \
        if (ks[k] >= 4) {                                                                      \
          l0 = (p0[0] + p0[1]) + (p0[2] + p0[3]);                                              \
          l1 = (p1[0] + p1[1]) + (p1[2] + p1[3]);                                              \
        } else {                 /* the group straddles a source boundary after ks elements (1..3) */ \
          l0 = p0[0]; l1 = p1[0];                                                              \
          if (ks[k] >= 2) { l0 += p0[1]; l1 += p1[1]; } else { h0 = p0[1]; h1 = p1[1]; }       \
          if (ks[k] >= 3) { l0 += p0[2]; l1 += p1[2]; } else { h0 += p0[2]; h1 += p1[2]; }     \
          h0 += p0[3]; h1 += p1[3];                                                            \
        }                                                                                      \
        const int o = q + (q >> 4);                                                            \
        Sp[0][o] = l0; Sp[1][o] = h0; Sp[2][o] = l1; Sp[3][o] = h1;                            \
      }                                                                                        \
    }                                                                                          \
    __syncthreads();                                                                           \
    _Pragma("unroll") for (int k = 0; k < 2; ++k) V[k] = vb[k];      /* the row fetched one row ago */ \
    UPS_FETCH(vb, r + 2 * stride);                /* two rows in flight */ \
    for (int p = 0; p < npass; ++p) {   /* wave-uniform trip count: the shuffles need all eight lanes */ \
      const int vi = (p * UPS_NT + tid) >> 3;                                                  \
      const bool ok = vi < Tin;                                                                \
      const int vc = ok ? vi : 0;                                                              \
      const int tl = part ? lo1[vc] : lo0[vc];                                                 \
      const int th = ok ? (part ? hi1[vc] : hi0[vc]) : tl;                                     \
      const float* Sl = Sp[2 * part];                                                          \
      const float* Sh = Sp[2 * part + 1];                                                      \
      float acc = 0.f;                                                                         \
      const int qe = (th + 3) >> 2;                                                            \
      for (int q = ((tl + 3) >> 2) + j4; q < qe; q += 4) acc += Sl[q + (q >> 4)];              \
      if (j4 == 0 && th > tl && (tl & 3)) { const int q = tl >> 2; acc += Sh[q + (q >> 4)]; }  \
      acc += __shfl_xor(acc, 1, 64);                                                           \
      acc += __shfl_xor(acc, 2, 64);                                                           \
      acc += __shfl_xor(acc, 4, 64);              /* w1-range sum + w0-range sum */            \
      if (ok && (tid & 7) == 0) gx[gxo + vi] = acc;                                            \
    }                                                                                          \
    /* no second barrier: the next row writes the other parity, and nobody can reach the row after  \
       that (which overwrites this parity) before every thread has passed the next row's barrier */ \
  }
  const int stride = gridDim.x;
  int r = blockIdx.x;
  if (r >= rows) return;
  UPS_FETCH(va, r);
  UPS_FETCH(vb, r + stride);
  for (int par = 0; r < rows; r += stride, par ^= 1) UPS_ROW(va, par);
#undef UPS_FETCH
#undef UPS_ROW
}

// ---- speaker embedding broadcast -----------------------------------------
__global__ void embed_bcast_fwd_kernel(const float* __restrict__ E, const int32_t* __restrict__ ids,
                                       int B, int G, int T, float* __restrict__ y, long y_bstride) {
  const long total = (long)B * G * T;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const int t = (int)(i % T);
    const long r = i / T;
    const int c = (int)(r % G);
    const long b = r / G;
    y[b * y_bstride + (long)c * T + t] = E[(long)ids[b] * G + c];
  }
}

// one wavefront per (b,c) row: rowsum[b*G+c] = sum_t gy[b,c,t]
__global__ __launch_bounds__(256) void rowsum_kernel(const float* __restrict__ gy, long gy_bstride,
                                                     int B, int G, int T, float* __restrict__ rs) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B * G) return;
  const int b = row / G, c = row % G;
  const float* g = gy + (long)b * gy_bstride + (long)c * T;
  float acc = 0.f;
  for (int t = threadIdx.x & 63; t < T; t += 64) acc += g[t];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if ((threadIdx.x & 63) == 0) rs[row] = acc;
}

__global__ void embed_scatter_kernel(const float* __restrict__ rs, const int32_t* __restrict__ ids,
                                     int B, int G, int n_id, float* __restrict__ gE, int accumulate) {
  const long total = (long)n_id * G;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % G);
    const int sid = (int)(i / G);
    float acc = 0.f;
    for (int b = 0; b < B; ++b)
      if (ids[b] == sid) acc += rs[(long)b * G + c];
    gE[i] = accumulate ? gE[i] + acc : acc;
  }
}

// ---- softmax cross entropy -------------------------------------------------
// 64 positions (b,t) x 4 class groups per workgroup: lanes run along t (every load coalesced, channel
// stride T), the four waves split the class axis and combine max / sum-exp through LDS -- four times
// the parallelism of one thread per position for the 2 x q dependent strided loads.
__global__ __launch_bounds__(256) void xent_fwd_kernel(const float* __restrict__ y,
                                                       const int32_t* __restrict__ tg, int B, int q,
                                                       int T, float* __restrict__ lse,
                                                       float* __restrict__ partial) {
  __shared__ float sh[4];
  __shared__ float red[4][64];
  const long N = (long)B * T;
  const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int c0 = (int)(((long)q * grp) / 4), c1 = (int)(((long)q * (grp + 1)) / 4);
  float lacc = 0.f;
  for (long base = (long)blockIdx.x * 64; base < N; base += (long)gridDim.x * 64) {
    const long i = base + lane;
    const bool ok = i < N;
    const long b = ok ? i / T : 0;
    const int t = ok ? (int)(i % T) : 0;
    const float* yp = y + b * (long)q * T + t;
    float m = -INFINITY;
    if (ok)
#pragma unroll 8
      for (int c = c0; c < c1; ++c) m = fmaxf(m, yp[(long)c * T]);
    red[grp][lane] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0][lane], red[1][lane]), fmaxf(red[2][lane], red[3][lane]));
    __syncthreads();
    float ssum = 0.f;
    if (ok)
#pragma unroll 8
      for (int c = c0; c < c1; ++c) ssum += expf(yp[(long)c * T] - m);
    red[grp][lane] = ssum;
    __syncthreads();
    if (grp == 0 && ok) {
      const float l = logf((red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane])) + m;
      lse[i] = l;
      lacc += l - yp[(long)tg[i] * T];
    }
    __syncthreads();
  }
  const float tot = block_sum_256(lacc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

__global__ void xent_bwd_kernel(const float* __restrict__ y, const int32_t* __restrict__ tg,
                                const float* __restrict__ lse, const float* __restrict__ gloss,
                                int B, int q, int T, float scale, float* __restrict__ gy, uint32_t* __restrict__ amax_out) {
  const long total = (long)B * q * T;
  const float gs = (gloss ? gloss[0] : 1.f) * scale;
  // |gy| = |softmax - onehot| |gs| <= |gs|: an upper bound is all a float32x2 scale needs, and this one is within a few 1e-3
  // of the maximum (some position always has a small target probability) -- it saves the consumer a scan of 126 MB
  if (amax_out != nullptr && blockIdx.x == 0 && threadIdx.x < 16)
    amax_out[threadIdx.x] = threadIdx.x == 0 ? __float_as_uint(fmaxf(fabsf(gs) * 1.001f, 1e-30f)) : 0u;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const int t = (int)(i % T);
    const long r = i / T;
    const int c = (int)(r % q);
    const long b = r / q;
    const long pos = b * T + t;
    float p = expf(y[i] - lse[pos]);
    if (tg[pos] == c) p -= 1.f;
    gy[i] = p * gs;
  }
}

// The same per-element arithmetic on four consecutive positions of one (b, c) row per lane (T % 4 == 0): 16-byte loads and
// stores, the index divisions once per four elements.
typedef float xb_f4 __attribute__((ext_vector_type(4), aligned(4)));      // (the tensors are only known to be float-aligned)
typedef int xb_i4 __attribute__((ext_vector_type(4), aligned(4)));
__global__ __launch_bounds__(256) void xent_bwd4_kernel(const float* __restrict__ y, const int32_t* __restrict__ tg,
                                                        const float* __restrict__ lse, const float* __restrict__ gloss,
                                                        int B, int q, int T, float scale, float* __restrict__ gy, uint32_t* __restrict__ amax_out) {
  const long total4 = (long)B * q * T / 4;
  const int T4 = T / 4;
  const float gs = (gloss ? gloss[0] : 1.f) * scale;
  if (amax_out != nullptr && blockIdx.x == 0 && threadIdx.x < 16)        // (the bound of xent_bwd_kernel)
    amax_out[threadIdx.x] = threadIdx.x == 0 ? __float_as_uint(fmaxf(fabsf(gs) * 1.001f, 1e-30f)) : 0u;
  for (long i4 = (long)blockIdx.x * blockDim.x + threadIdx.x; i4 < total4; i4 += (long)gridDim.x * blockDim.x) {
    const int t = (int)(i4 % T4) * 4;
    const long r = i4 / T4;
    const int c = (int)(r % q);
    const long b = r / q;
    const long pos = b * T + t;
    const xb_f4 yv = *reinterpret_cast<const xb_f4*>(y + i4 * 4);
    const xb_f4 lv = *reinterpret_cast<const xb_f4*>(lse + pos);
    const xb_i4 tv = *reinterpret_cast<const xb_i4*>(tg + pos);
    xb_f4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float p = expf(yv[k] - lv[k]);
      if (tv[k] == c) p -= 1.f;
      o[k] = p * gs;
    }
    *reinterpret_cast<xb_f4*>(gy + i4 * 4) = o;
  }
}

// ---- discretised mixture-of-logistics NLL (WaveNet.calculate_logistic_loss,
//      modules.py:169-230).  Thread per (b,t); the 3*nmix channels are strided by T so
//      every load is coalesced along t.  MODE 0: per-position loss -> block partial sums;
//      MODE 1: gradient w.r.t. y.  Same op sequence as the oracle (tanh-form sigmoid,
//      softplus = max(x,0) + log1p(exp(-|x|))).
__device__ __forceinline__ float sig_(float x) { return tanhf(x * 0.5f) * 0.5f + 0.5f; }
__device__ __forceinline__ float softplus_(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

template <int MODE>
__global__ __launch_bounds__(256) void mol_kernel(const float* __restrict__ y, const float* __restrict__ tg,
                                                  int B, int nmix, int T, float half, float ls_min,
                                                  const float* __restrict__ gloss, float scale,
                                                  float* __restrict__ partial, float* __restrict__ gy) {
  __shared__ float sh[4];
  constexpr int MAXM = 16;
  const long N = (long)B * T;
  float lacc = 0.f;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < N;
       i += (long)gridDim.x * blockDim.x) {
    const long b = i / T;
    const int t = (int)(i % T);
    const float* yp = y + b * 3L * nmix * T + t;
    const float tt = 127.5f * tg[i];
    const bool left = tt < 127.5f * -0.999f, right = tt > 127.5f * 0.999f;
    float lp[MAXM], v[MAXM], dpl[MAXM], dmi[MAXM], pin[MAXM], mii[MAXM], istd[MAXM];
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < MAXM; ++k) if (k < nmix) { lp[k] = yp[(long)k * T]; m = fmaxf(m, lp[k]); }
    float se = 0.f;
#pragma unroll
    for (int k = 0; k < MAXM; ++k) if (k < nmix) se += expf(lp[k] - m);
    const float lz = logf(se) + m;                       // log-sum-exp of the mixture logits
    float vm = -INFINITY;
#pragma unroll
    for (int k = 0; k < MAXM; ++k) if (k < nmix) {
      const float mu = yp[(long)(nmix + k) * T];
      const float ls = fmaxf(yp[(long)(2 * nmix + k) * T], ls_min);
      const float c = tt - mu;
      const float is = expf(-ls);
      const float p = is * (c + half), q = is * (c - half);
      const float cp = sig_(p), cm = sig_(q);
      const float cd = cp - cm;
      float lpr;
      if (left) { lpr = p - softplus_(p); dpl[k] = 1.f - cp; dmi[k] = 0.f; }
      else if (right) { lpr = -softplus_(q); dpl[k] = 0.f; dmi[k] = -cm; }
      else {
        lpr = logf(fmaxf(cd, 1e-12f));
        const float inv = cd >= 1e-12f ? 1.f / fmaxf(cd, 1e-12f) : 0.f;
        dpl[k] = inv * cp * (1.f - cp);
        dmi[k] = -inv * cm * (1.f - cm);
      }
      pin[k] = p; mii[k] = q; istd[k] = is;
      v[k] = lpr + (lp[k] - lz);
      vm = fmaxf(vm, v[k]);
    }
    float sv = 0.f;
#pragma unroll
    for (int k = 0; k < MAXM; ++k) if (k < nmix) sv += expf(v[k] - vm);
    const float lse = logf(sv) + vm;
    if (MODE == 0) {
      lacc += lse;
    } else {
      const float gs = -(gloss ? gloss[0] : 1.f) * scale;      // d loss / d lse
      float* gp = gy + b * 3L * nmix * T + t;
      float gsum = 0.f;
#pragma unroll
      for (int k = 0; k < MAXM; ++k) if (k < nmix) { v[k] = gs * expf(v[k] - lse); gsum += v[k]; }
#pragma unroll
      for (int k = 0; k < MAXM; ++k) if (k < nmix) {
        gp[(long)k * T] = v[k] - expf(lp[k] - lz) * gsum;
        gp[(long)(nmix + k) * T] = v[k] * (dpl[k] + dmi[k]) * (-istd[k]);
        const float gl = v[k] * (dpl[k] * (-pin[k]) + dmi[k] * (-mii[k]));
        gp[(long)(2 * nmix + k) * T] = yp[(long)(2 * nmix + k) * T] >= ls_min ? gl : 0.f;
      }
    }
  }
  if (MODE == 0) {
    const float tot = block_sum_256(lacc, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
  }
}

// ---- device-side input pipeline -----------------------------------------
// mu-law binning by threshold search: thr[j-1] (j = 1..mu-1) is the smallest fp32 input whose
// NumPy MuLaw.transform (utils.py:18-23) is >= j, found on the host by bisection against that
// very function; the transform is monotone, so bin(x) = #{j : x >= thr[j-1]} reproduces it bit
// for bit without re-implementing log/digitize rounding on the device.
__global__ void mulaw_bins_kernel(const float* __restrict__ x, size_t n, const float* __restrict__ thr,
                                  int nthr, int32_t* __restrict__ q) {
  extern __shared__ float sthr[];
  for (int i = threadIdx.x; i < nthr; i += blockDim.x) sthr[i] = thr[i];
  __syncthreads();
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x) {
    const float v = x[i];
    int lo = 0, hi = nthr;                 // count of thresholds <= v  (upper bound search)
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (sthr[mid] <= v) lo = mid + 1; else hi = mid;
    }
    q[i] = lo;
  }
}

// one-hot(idx) as fp32 (B, q, T): what Preprocess feeds the decoder (utils.py:85-87); used by the
// index-input embed conv's weight gradient so that it stays the dense contraction
__global__ void onehot_kernel(const int32_t* __restrict__ idx, long idx_bstride, int B, int q, int T,
                              float* __restrict__ out) {
  const long total = (long)B * q * T;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const int t = (int)(i % T);
    const long r = i / T;
    const int c = (int)(r % q);
    const long b = r / q;
    out[i] = idx[b * idx_bstride + t] == c ? 1.f : 0.f;
  }
}

// causal embed conv of a one-hot input, as a gather: y[b,co,t] = bias[co] +
// sum_tap W[co, idx[b, t-(K-1-tap)], tap]   (zero for negative times; modules.py:127-128,151-152)
__global__ void embed_gather_kernel(const int32_t* __restrict__ idx, long idx_bstride, int B, int T,
                                    const float* __restrict__ W, const float* __restrict__ bias,
                                    int Cout, int q, int K, float* __restrict__ y,
                                    const int32_t* __restrict__ run_flag) {
  if (run_flag != nullptr && *run_flag == 0) return;      // device-side conditional launch
  const long total = (long)B * Cout * T;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const int t = (int)(i % T);
    const long r = i / T;
    const int co = (int)(r % Cout);
    const long b = r / Cout;
    const int32_t* ib = idx + b * idx_bstride;
    const float* wc = W + (long)co * q * K;
    float acc = 0.f;
    for (int tap = 0; tap < K; ++tap) {                 // same order as the GEMM's segments
      const int ti = t - (K - 1 - tap);
      if (ti >= 0) acc = __fadd_rn(acc, wc[(long)ib[ti] * K + tap]);
    }
    y[i] = bias ? __fadd_rn(acc, bias[co]) : acc;
  }
}

// ---- the decoder's embed conv on a ONE-HOT input (modules.py:127-128, 151-152; utils.py:85-87) ----
// The reference feeds the 256-channel one-hot tensor through a dense conv: 2*B*T*Cout*q*K FLOP of
// multiplications by zero, forward and again in the weight gradient.  onehot_scan_kernel recovers the
// class index of every column and proves (or refutes) on the device that the tensor is exactly
// one-hot; the gather / bincount forms below and the dense kernels are then both launched, each
// guarded by the flag, so the choice needs no host round trip and a non-one-hot input silently
// takes the dense path.
__global__ __launch_bounds__(256) void onehot_scan_kernel(const float* __restrict__ x, int B, int q, int T,
                                                          int32_t* __restrict__ idx,
                                                          int32_t* __restrict__ flag) {
  const long N = (long)B * T;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long)gridDim.x * blockDim.x) {
    const long b = i / T;
    const int t = (int)(i % T);
    const float* xp = x + b * (long)q * T + t;
    int pos = 0, ones = 0;
    bool ok = true;
#pragma unroll 8
    for (int c = 0; c < q; ++c) {
      const float v = xp[(long)c * T];
      if (v == 1.0f) { pos = c; ++ones; }
      else if (v != 0.0f) ok = false;
    }
    idx[i] = pos;
    if (!ok || ones != 1) atomicExch(flag, 0);
  }
}
__global__ void set_flag_kernel(int32_t* flag, int32_t v) { *flag = v; }

// T % 4 == 0 form: 64 column quads x 4 channel groups per workgroup, 16-byte loads, four in flight
__global__ __launch_bounds__(256) void onehot_scan4_kernel(const float* __restrict__ x, int B, int q, int T,
                                                           int32_t* __restrict__ idx,
                                                           int32_t* __restrict__ flag) {
  __shared__ int s_pos[4][64][4];
  __shared__ int s_cnt[4][64][4];       // number of ones; -1000 marks an entry that is neither 0 nor 1
  const int cq = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const long nquad = (long)B * T / 4;
  const long quad = (long)blockIdx.x * 64 + cq;
  int pos[4] = {0, 0, 0, 0}, cnt[4] = {0, 0, 0, 0};
  if (quad < nquad) {
    const long i0 = quad * 4;
    const long b = i0 / T;
    const int t = (int)(i0 % T);
    const int c0 = (int)(((long)q * grp) / 4), c1 = (int)(((long)q * (grp + 1)) / 4);
    const float* xp = x + b * (long)q * T + t;
    auto look = [&](const float4 v, int c) {
      const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (e[j] == 1.0f) { pos[j] = c; ++cnt[j]; }
        else if (e[j] != 0.0f) cnt[j] = -1000;
      }
    };
    int c = c0;
    for (; c + 3 < c1; c += 4) {
      const float4 v0 = *reinterpret_cast<const float4*>(xp + (long)c * T);
      const float4 v1 = *reinterpret_cast<const float4*>(xp + (long)(c + 1) * T);
      const float4 v2 = *reinterpret_cast<const float4*>(xp + (long)(c + 2) * T);
      const float4 v3 = *reinterpret_cast<const float4*>(xp + (long)(c + 3) * T);
      look(v0, c); look(v1, c + 1); look(v2, c + 2); look(v3, c + 3);
    }
    for (; c < c1; ++c) look(*reinterpret_cast<const float4*>(xp + (long)c * T), c);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) { s_pos[grp][cq][j] = pos[j]; s_cnt[grp][cq][j] = cnt[j]; }
  __syncthreads();
  if (grp == 0 && quad < nquad) {
    int4 out;
    int* o = reinterpret_cast<int*>(&out);
    bool good = true;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int n = 0, p = 0;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int cg = s_cnt[g][cq][j];
        if (cg < 0) good = false;
        if (cg > 0) p = s_pos[g][cq][j];
        n += cg;
      }
      if (n != 1) good = false;
      o[j] = p;
    }
    *reinterpret_cast<int4*>(idx + quad * 4) = out;
    if (!good) atomicExch(flag, 0);
  }
}

// weight gradient of the embed conv from the class indices: gW[co, c, tap] = sum of gy[b, co, t] over
// the positions whose input class (at t - (K-1-tap)) is c -- a weighted bincount of each output-
// gradient row.  One wave per (b, co) row, bins in LDS (ds_add_f32; lanes of one instruction that hit
// the same bin are applied in lane order, instructions in program order: deterministic), per-row
// partial histograms to HBM, then a fixed-order sum over the batch.
__global__ __launch_bounds__(256) void embed_bincount_kernel(const int32_t* __restrict__ idx,
                                                             const float* __restrict__ gy, int B, int Cout,
                                                             int q, int K, int T, float* __restrict__ part,
                                                             const int32_t* __restrict__ run_flag) {
  extern __shared__ float bins[];                 // [4 waves][K][q]
  if (run_flag != nullptr && *run_flag == 0) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* mine = bins + (size_t)wave * K * q;
  const long rows = (long)B * Cout;
  for (long row = (long)blockIdx.x * 4 + wave; row < rows; row += (long)gridDim.x * 4) {
    for (int i = lane; i < K * q; i += 64) mine[i] = 0.f;
    const long b = row / Cout;
    const int32_t* ib = idx + b * T;
    const float* g = gy + row * T;
    for (int t0 = 0; t0 < T; t0 += 64) {
      const int t = t0 + lane;
      if (t < T) {
        const float v = g[t];
        for (int tap = 0; tap < K; ++tap) {
          const int ti = t - (K - 1 - tap);
          if (ti >= 0) { const int c = ib[ti]; if ((unsigned)c < (unsigned)q) atomicAdd(&mine[tap * q + c], v); }   // a class outside [0, q) has no one-hot row: no contribution, no stray LDS write
        }
      }
    }
    float* out = part + row * (long)K * q;
    for (int i = lane; i < K * q; i += 64) out[i] = mine[i];
  }
}
__global__ void embed_bincount_reduce_kernel(const float* __restrict__ part, int B, int Cout, int q, int K,
                                             float* __restrict__ gW, int accumulate,
                                             const int32_t* __restrict__ run_flag) {
  if (run_flag != nullptr && *run_flag == 0) return;
  const long total = (long)Cout * K * q;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % q);
    const long r = i / q;
    const int tap = (int)(r % K), co = (int)(r / K);
    float v = 0.f;
    for (int b = 0; b < B; ++b) v += part[(((long)b * Cout + co) * K + tap) * q + c];
    float* dst = gW + ((long)co * q + c) * K + tap;                 // Chainer layout (Cout, q, K)
    *dst = accumulate ? *dst + v : v;
  }
}
// bias gradient = row sum of gy = sum over batch and classes of the UNSHIFTED tap's histograms
// (every position has exactly one class there).  One wave per output channel, fixed order.
__global__ __launch_bounds__(64) void embed_bincount_bias_kernel(const float* __restrict__ part, int B,
                                                                 int Cout, int q, int K, float* __restrict__ gb,
                                                                 int accumulate,
                                                                 const int32_t* __restrict__ run_flag) {
  if (run_flag != nullptr && *run_flag == 0) return;
  const int co = blockIdx.x, lane = threadIdx.x;
  float v = 0.f;
  for (int b = 0; b < B; ++b) {
    const float* pp = part + (((long)b * Cout + co) * K + (K - 1)) * q;
    for (int c = lane; c < q; c += 64) v += pp[c];
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  if (lane == 0) gb[co] = accumulate ? gb[co] + v : v;
}

// K == 2, T % 4 == 0: four output columns per thread, one 16-byte store
__global__ __launch_bounds__(256) void embed_gather2x4_kernel(const int32_t* __restrict__ idx, int B, int T,
                                                              const float* __restrict__ W,
                                                              const float* __restrict__ bias, int Cout, int q,
                                                              float* __restrict__ y,
                                                              const int32_t* __restrict__ run_flag) {
  if (run_flag != nullptr && *run_flag == 0) return;
  const int T4 = T >> 2;
  const long total = (long)B * Cout * T4;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int t = (int)(i % T4) * 4;
    const long r = i / T4;
    const int co = (int)(r % Cout);
    const long b = r / Cout;
    const int32_t* ib = idx + b * T + t;
    const int4 c1 = *reinterpret_cast<const int4*>(ib);             // classes at t .. t+3   (tap 1)
    const int cm = t > 0 ? ib[-1] : -1;                              // class at t-1          (tap 0 of column t)
    const float* wc = W + (long)co * q * 2;
    const float bv = bias ? bias[co] : 0.f;
    // same order as the dense GEMM's segments: tap 0 first, then tap 1, then the bias
    float4 o;
    o.x = __fadd_rn(cm >= 0 ? wc[2 * cm] : 0.f, wc[2 * c1.x + 1]);
    o.y = __fadd_rn(wc[2 * c1.x], wc[2 * c1.y + 1]);
    o.z = __fadd_rn(wc[2 * c1.y], wc[2 * c1.z + 1]);
    o.w = __fadd_rn(wc[2 * c1.z], wc[2 * c1.w + 1]);
    if (bias) { o.x = __fadd_rn(o.x, bv); o.y = __fadd_rn(o.y, bv); o.z = __fadd_rn(o.z, bv); o.w = __fadd_rn(o.w, bv); }
    *reinterpret_cast<float4*>(y + (b * Cout + co) * (long)T + t) = o;
  }
}

// The same gather with the output channel's 2 q weights staged in LDS: a workgroup walks whole (b, co) rows, so the eight
// random reads per thread are LDS reads instead of eight gathers through the address path (54 -> ~30 us at configs[1]: the
// kernel sits in front of the first gate launch).  Same additions in the same order: bit-identical.
__global__ __launch_bounds__(256) void embed_gather2x4_lds_kernel(const int32_t* __restrict__ idx, int B, int T,
                                                                  const float* __restrict__ W,
                                                                  const float* __restrict__ bias, int Cout, int q,
                                                                  float* __restrict__ y,
                                                                  const int32_t* __restrict__ run_flag) {
  extern __shared__ float wrow[];                 // [q][2]: tap 0 | tap 1 of every class, this row's output channel
  if (run_flag != nullptr && *run_flag == 0) return;
  const int T4 = T >> 2, rows = B * Cout;
  for (int r = blockIdx.x; r < rows; r += gridDim.x) {
    const int co = r % Cout, b = r / Cout;
    __syncthreads();                              // the previous row's readers are done
    for (int i = threadIdx.x; i < 2 * q; i += 256) wrow[i] = W[(long)co * q * 2 + i];
    __syncthreads();
    const float bv = bias ? bias[co] : 0.f;
    const int32_t* ib0 = idx + (long)b * T;
    float* yr = y + (long)r * T;
    for (int i = threadIdx.x; i < T4; i += 256) {
      const int t = 4 * i;
      const int4 c1 = *reinterpret_cast<const int4*>(ib0 + t);       // classes at t .. t+3   (tap 1)
      const int cm = t > 0 ? ib0[t - 1] : -1;                         // class at t-1          (tap 0 of column t)
      float4 o;
      o.x = __fadd_rn(cm >= 0 ? wrow[2 * cm] : 0.f, wrow[2 * c1.x + 1]);
      o.y = __fadd_rn(wrow[2 * c1.x], wrow[2 * c1.y + 1]);
      o.z = __fadd_rn(wrow[2 * c1.y], wrow[2 * c1.z + 1]);
      o.w = __fadd_rn(wrow[2 * c1.z], wrow[2 * c1.w + 1]);
      if (bias) { o.x = __fadd_rn(o.x, bv); o.y = __fadd_rn(o.y, bv); o.z = __fadd_rn(o.z, bv); o.w = __fadd_rn(o.w, bv); }
      *reinterpret_cast<float4*>(yr + t) = o;
    }
  }
}

// K == 2, T % 4 == 0 form of the bincount: four positions per lane (16-byte loads), two chunks in flight.
// The kernel is bound by the LDS atomic unit, about 3 clocks per lane-add whatever the addresses
// are: spreading the lanes over BC_NCOPY private copies of the histograms (8 copies, 2 waves)
// measured 313 us against 309 us for one copy per wave, so one copy it is -- 8 KB of LDS per
// workgroup, which lets it share a CU with the MFMA kernels it is overlapped with.
constexpr int BC_NCOPY = 1, BC_WAVES = 4;
__global__ __launch_bounds__(64 * BC_WAVES) void embed_bincount2x4_kernel(const int32_t* __restrict__ idx,
                                                                const float* __restrict__ gy, int B, int Cout,
                                                                int q, int T, float* __restrict__ part,
                                                                const int32_t* __restrict__ run_flag) {
  extern __shared__ float bins[];                 // [BC_WAVES][NCOPY][2][q]
  if (run_flag != nullptr && *run_flag == 0) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* base = bins + (size_t)wave * BC_NCOPY * 2 * q;
  float* b0 = base + (size_t)(lane % BC_NCOPY) * 2 * q;   // tap 0: class of the previous position
  float* b1 = b0 + q;                                      // tap 1: class of the position itself
  const long rows = (long)B * Cout;
  for (long row = (long)blockIdx.x * BC_WAVES + wave; row < rows; row += (long)gridDim.x * BC_WAVES) {
    for (int i = lane; i < BC_NCOPY * 2 * q; i += 64) base[i] = 0.f;
    const long b = row / Cout;
    const int32_t* ib = idx + b * T;
    const float* g = gy + row * T;
    const unsigned uq = (unsigned)q;           // a class outside [0, q) has no one-hot row: it contributes nothing
    auto add = [&](const float4 v, const int4 c, int cm) {
      const bool ox = (unsigned)c.x < uq, oy = (unsigned)c.y < uq, oz = (unsigned)c.z < uq, ow = (unsigned)c.w < uq;
      if (ox) atomicAdd(&b1[c.x], v.x);
      if (oy) atomicAdd(&b1[c.y], v.y);
      if (oz) atomicAdd(&b1[c.z], v.z);
      if (ow) atomicAdd(&b1[c.w], v.w);
      if ((unsigned)cm < uq) atomicAdd(&b0[cm], v.x);
      if (ox) atomicAdd(&b0[c.x], v.y);
      if (oy) atomicAdd(&b0[c.y], v.z);
      if (oz) atomicAdd(&b0[c.z], v.w);
    };
    int t = 4 * lane;
    for (; t + 256 < T; t += 512) {               // two independent chunks per iteration
      const float4 v0 = *reinterpret_cast<const float4*>(g + t);
      const int4 c0 = *reinterpret_cast<const int4*>(ib + t);
      const int m0 = t > 0 ? ib[t - 1] : -1;
      const float4 v1 = *reinterpret_cast<const float4*>(g + t + 256);
      const int4 c1 = *reinterpret_cast<const int4*>(ib + t + 256);
      const int m1 = ib[t + 255];
      add(v0, c0, m0);
      add(v1, c1, m1);
    }
    for (; t < T; t += 256) {
      const float4 v0 = *reinterpret_cast<const float4*>(g + t);
      const int4 c0 = *reinterpret_cast<const int4*>(ib + t);
      add(v0, c0, t > 0 ? ib[t - 1] : -1);
    }
    float* out = part + row * (long)2 * q;
    for (int i = lane; i < 2 * q; i += 64) {
      float v = 0.f;
#pragma unroll
      for (int cpy = 0; cpy < BC_NCOPY; ++cpy) v += base[(size_t)cpy * 2 * q + i];
      out[i] = v;
    }
  }
}


// ---- K == 2 bincount as a gather over class-sorted positions ----------------------------------------------
// The LDS-atomic form above costs ~3 clocks per lane-add (345 us at configs[1]: 63 M adds).  The positions of
// one batch item are the same for all Cout rows of that item, so they are sorted by class ONCE per item
// (embed_sort_kernel: stable counting sort -> perm[b][.], off[b][c]) and every row then sums, per class, the
// gradient values at that class's positions (tap 1) and at the positions after them (tap 0: the class of the
// PREVIOUS sample) -- plain LDS reads, no atomics.  ES_LPC lanes share a class (position j of the class's list
// goes to lane j % ES_LPC), their partial sums are combined in lane order: a fixed summation order.
constexpr int ES_NT = 1024, ES_NW = ES_NT / 64;
// Stable counting sort of one batch item's positions by class.  Every wave owns a contiguous chunk of the time
// axis and a private counter row: the returning ds_add gives a position its rank among the SAME-class positions
// of its chunk (lanes of one instruction are applied in lane order, instructions in program order), a scan over
// (class, wave) turns the counters into start offsets.  Deterministic, and position-ordered within a class.
__global__ __launch_bounds__(ES_NT) void embed_sort_kernel(const int32_t* __restrict__ idx, int q, int T,
                                                           unsigned short* __restrict__ perm, int32_t* __restrict__ off,
                                                           const int32_t* __restrict__ run_flag) {
  extern __shared__ unsigned char es_smem[];
  if (run_flag != nullptr && *run_flag == 0) return;
  int* wcnt = reinterpret_cast<int*>(es_smem);                                  // [ES_NW][q]
  int* sc = wcnt + ES_NW * q;                                                   // [ES_NT] block scan
  unsigned short* rank = reinterpret_cast<unsigned short*>(sc + ES_NT);         // [T]
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t* ib = idx + (long)b * T;
  for (int i = tid; i < ES_NW * q; i += ES_NT) wcnt[i] = 0;
  __syncthreads();
  const int ch = ((T + ES_NW - 1) / ES_NW + 63) & ~63;                          // chunk length, a multiple of 64
  const int t_lo = wave * ch, t_hi = min(T, t_lo + ch);
  int* mine = wcnt + wave * q;
  for (int t = t_lo + lane; t < t_hi; t += 64) {
    const int c = ib[t];
    if ((unsigned)c < (unsigned)q) rank[t] = (unsigned short)atomicAdd(&mine[c], 1);
  }
  __syncthreads();
  int tot = 0;
  if (tid < q) for (int w = 0; w < ES_NW; ++w) { const int v = wcnt[w * q + tid]; wcnt[w * q + tid] = tot; tot += v; }
  sc[tid] = tid < q ? tot : 0;
  __syncthreads();
  for (int d = 1; d < ES_NT; d <<= 1) {                                         // inclusive block scan over the classes
    const int v = tid >= d ? sc[tid - d] : 0;
    __syncthreads();
    sc[tid] += v;
    __syncthreads();
  }
  if (tid < q) off[(long)b * (q + 1) + tid] = sc[tid] - tot;
  if (tid == q - 1) off[(long)b * (q + 1) + q] = sc[tid];
  unsigned short* pb = perm + (long)b * T;
  for (int t = t_lo + lane; t < t_hi; t += 64) {
    const int c = ib[t];
    if ((unsigned)c < (unsigned)q) pb[(c ? sc[c - 1] : 0) + mine[c] + rank[t]] = (unsigned short)t;    // class start + this wave's start within the class + rank within the wave's chunk
  }
}

constexpr int EG_ROWS = 8;                                 // rows (output channels) of one batch item per workgroup
__global__ __launch_bounds__(ES_NT) void embed_gathersum_kernel(const float* __restrict__ gy, int B, int Cout, int q, int T,
                                                                int lpc, const unsigned short* __restrict__ perm,
                                                                const int32_t* __restrict__ off, float* __restrict__ part,
                                                                const int32_t* __restrict__ run_flag) {
  extern __shared__ unsigned char eg_smem[];
  if (run_flag != nullptr && *run_flag == 0) return;
  float* g0 = reinterpret_cast<float*>(eg_smem);                               // [2][T + 4] gradient rows (double buffer)
  const int pitch = T + 4;
  unsigned short* pl = reinterpret_cast<unsigned short*>(g0 + 2 * pitch);      // [T] this item's sorted positions
  int* ol = reinterpret_cast<int*>(reinterpret_cast<unsigned char*>(pl) + (((size_t)T * 2 + 15) & ~(size_t)15));   // [q + 1]
  const int tid = threadIdx.x;
  const int groups = (Cout + EG_ROWS - 1) / EG_ROWS;
  const int b = blockIdx.x / groups, r0 = (blockIdx.x % groups) * EG_ROWS;
  const int nr = min(EG_ROWS, Cout - r0);
  for (int t = tid; t < T; t += ES_NT) pl[t] = perm[(long)b * T + t];
  for (int i = tid; i <= q; i += ES_NT) ol[i] = off[(long)b * (q + 1) + i];
  const float* gb = gy + ((long)b * Cout + r0) * T;
  const int T4 = T >> 2;                                   // host: T % 4 == 0, rows 16-byte aligned
  for (int i = tid; i < T4; i += ES_NT) *reinterpret_cast<float4*>(g0 + 4 * i) = *reinterpret_cast<const float4*>(gb + 4 * i);
  if (tid < 4) g0[T + tid] = 0.f, g0[pitch + T + tid] = 0.f;                   // g[T] = 0: the position after the last one
  __syncthreads();
  const int c = tid / lpc, k = tid % lpc;
  const int j0 = c < q ? ol[c] : 0, j1 = c < q ? ol[c + 1] : 0;
  for (int r = 0; r < nr; ++r) {
    float* g = g0 + (r & 1) * pitch;
    if (r + 1 < nr) {                                      // next row into the other buffer while this one is summed
      float* gn = g0 + ((r + 1) & 1) * pitch;
      const float* src = gb + (long)(r + 1) * T;
      for (int i = tid; i < T4; i += ES_NT) *reinterpret_cast<float4*>(gn + 4 * i) = *reinterpret_cast<const float4*>(src + 4 * i);
    }
    float s0 = 0.f, s1 = 0.f;
    for (int j = j0 + k; j < j1; j += lpc) {
      const int t = pl[j];
      s1 += g[t];                                          // tap 1: the class of the position itself
      s0 += g[t + 1];                                      // tap 0: this position is the PREVIOUS sample of t + 1 (g[T] = 0)
    }
    for (int d = 1; d < lpc; d <<= 1) {                    // lanes of a class are adjacent: fixed-order tree
      s0 += __shfl_xor(s0, d, 64);
      s1 += __shfl_xor(s1, d, 64);
    }
    if (c < q && k == 0) {
      float* out = part + ((long)b * Cout + r0 + r) * 2 * q;
      out[c] = s0;
      out[q + c] = s1;
    }
    __syncthreads();
  }
}

// ---- concat / split of equally sized parameter arrays ---------------------------
struct PtrList32 { float* p[32]; };
__global__ void concat_kernel(const PtrList32 src, int n, long count, float* __restrict__ dst) {
  const long total = (long)n * count;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x)
    dst[i] = src.p[i / count][i % count];
}
__global__ void split_kernel(const float* __restrict__ src, const PtrList32 dst, int n, long count,
                             int accumulate) {
  const long total = (long)n * count;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    float* d = dst.p[i / count];
    if (!d) continue;
    const long j = i % count;
    d[j] = accumulate ? d[j] + src[i] : src[i];
  }
}

// ---- many small device-to-device copies in one launch (arena adoption: a copy per parameter and arena was ~900
// __amd_rocclr_copyBuffer dispatches at start-up) ------------------------------
struct CopyJobs { float* dst[64]; const float* src[64]; unsigned n[64]; };
__global__ __launch_bounds__(256) void copy_list_kernel(const CopyJobs j) {
  float* __restrict__ d = j.dst[blockIdx.y];
  const float* __restrict__ s = j.src[blockIdx.y];
  const unsigned n = j.n[blockIdx.y];
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) d[i] = s[i];      // (size_t: a 32-bit index wraps for n within one grid stride of 2^32)
}

// ---- Adam / EMA ------------------------------------------------------------
// lr_table != nullptr: the step size is lr_table[*step] -- a captured step (hipGraph) is replayed with the next entry
// every time; step_inc_kernel advances the counter behind the update
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                            float* __restrict__ v, size_t n, float lr, float c1, float c2, float eps,
                            const float* __restrict__ lr_table, const int32_t* __restrict__ step) {
  if (lr_table != nullptr) lr = lr_table[*step];
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x) {
    const float gi = g[i];
    const float mi = __fadd_rn(m[i], __fmul_rn(c1, __fsub_rn(gi, m[i])));
    const float vi = __fadd_rn(v[i], __fmul_rn(c2, __fsub_rn(__fmul_rn(gi, gi), v[i])));
    m[i] = mi;
    v[i] = vi;
    p[i] = __fsub_rn(p[i], __fdiv_rn(__fmul_rn(lr, mi), __fadd_rn(__fsqrt_rn(vi), eps)));
  }
}

__global__ void step_inc_kernel(int32_t* step) { *step += 1; }

__global__ void ema_kernel(float* __restrict__ ema, const float* __restrict__ tgt, size_t n, float d,
                           float om) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x)
    ema[i] = __fadd_rn(__fmul_rn(d, tgt[i]), __fmul_rn(om, ema[i]));
}

// float32x2's pre-split storage contract, checked where the numbers are (vqvae_f32x2_contract_check): pair i = (scale words,
// maximum words) of one pre-split tensor -- the BOUND it was split under (word 0 of its scale group) against the ACTUAL
// maximum its producer published (the maximum over the group).  A bound 2^m above the maximum costs m bits of the mode's
// 2^-39 absolute floor; beyond `log2_limit` the tensor is outside what the mode promises.  One thread per pair.
struct ContractPairs { const uint32_t* scale[64]; const uint32_t* amax[64]; };
__global__ void f32x2_contract_kernel(const ContractPairs cp, int n, int log2_limit, uint32_t* report) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || cp.scale[i] == nullptr || cp.amax[i] == nullptr) return;
  const float bound = __builtin_bit_cast(float, cp.scale[i][0]);
  uint32_t mx = 0;
  for (int j = 0; j < VQVAE_AMAX_SLOTS; ++j) mx = max(mx, cp.amax[i][j]);
  const float amax = __builtin_bit_cast(float, mx);
  if (!(bound > 0.f) || !(amax > 0.f)) return;            // nothing was split under this group / an all-zero tensor has no precision to lose
  atomicAdd(report + 2, 1u);
  const float ratio = bound / amax;                        // >= 1 by construction of the bounds; < 1 would itself be a violation (overflow of the split)
  atomicMax(report + 1, __builtin_bit_cast(uint32_t, fmaxf(ratio, 0.f)));
  if (ratio > __builtin_ldexpf(1.f, log2_limit) || ratio < 0.999f) atomicAdd(report, 1u);
}

}  // namespace vq

using namespace vq;

// The one launcher of upsample_bwd_seg_kernel<fmt> (fmt = the kernel's IN16 = how gy is stored: 0 fp32, 1 bf16, 2 pre-split
// with its `scale` words) behind the four pull-back exports: L equally shaped tensors, gy_lstride / gx_lstride apart.
// served = false: not a shape the kernel takes (nothing launched, no error set) -- the caller falls back or rejects.
static int launch_upsample_bwd_seg(int fmt, const void* gy, unsigned gy_align, long gy_lstride, long gy_bstride, int L, int B, int C,
                                   int Tin, int Tout, const float* w0, const float* w1, const int32_t* lo0, const int32_t* hi0,
                                   const int32_t* lo1, const int32_t* hi1, float* gx, long gx_lstride, long gx_bstride,
                                   const uint32_t* scale, vqvae_stream_t s, bool& served) {
  served = Tin >= 3 && Tout >= 8 * Tin && Tout % 4 == 0 && Tout / 4 <= 2 * UPS_NT && gy_bstride % 4 == 0 && gy_lstride % 4 == 0 &&
           ((uintptr_t)gy) % gy_align == 0 && ((uintptr_t)w0) % 16 == 0 && ((uintptr_t)w1) % 16 == 0 && (long)L * B * C < (1L << 31);
  if (!served) return 0;
  long nb = (long)L * B * C;
  if (nb > 512) nb = 512;                        // persistent: 2 workgroups per CU
  auto k = fmt == 2 ? upsample_bwd_seg_kernel<2> : (fmt == 1 ? upsample_bwd_seg_kernel<1> : upsample_bwd_seg_kernel<0>);
  hipLaunchKernelGGL(k, dim3((unsigned)nb), dim3(UPS_NT), 0, (hipStream_t)s, reinterpret_cast<const float*>(gy), gy_bstride, B, C, Tin, Tout,
                     w0, w1, lo0, hi0, lo1, hi1, gx, gx_bstride, scale, L, gy_lstride, gx_lstride);
  VQ_LAUNCH_CHECK();
  return 0;
}

extern "C" {

int vqvae_elementwise(int op, size_t n, const float* a, const float* b, float* out, float alpha,
                      float beta, vqvae_stream_t s) {
  VQ_REQUIRE(out, "elementwise: null out");
  VQ_REQUIRE(op >= 0 && op <= VQVAE_EW_MUL_SCALAR_DEV, "elementwise: bad op %d", op);
  if (!n) return 0;
  hipLaunchKernelGGL(ew_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)s, op, n, a, b, out, alpha, beta);
  VQ_LAUNCH_CHECK();
  return 0;
}

int vqvae_sum(const float* x, size_t n, float scale, float* out, void* ws, size_t ws_bytes,
              vqvae_stream_t s) {
  VQ_REQUIRE(x && out && ws, "sum: null pointer");
  if (ws_bytes < 4096 * 4) { set_error("sum: workspace too small"); return VQVAE_E_WORKSPACE; }
  const int np = grid_for(n, 256, 1024);
  hipLaunchKernelGGL(sum_stage1, dim3(np), dim3(256), 0, (hipStream_t)s, x, n, (float*)ws);
  VQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(sum_stage2, dim3(1), dim3(256), 0, (hipStream_t)s, (const float*)ws, np, scale, out);
  VQ_LAUNCH_CHECK();
  return 0;
}

int vqvae_sqdiff_mean(const float* a, const float* b, size_t n, float* out, void* ws, size_t ws_bytes, vqvae_stream_t s) {
  VQ_REQUIRE(a && b && out && ws && n > 0, "sqdiff_mean: bad arguments");
  if (ws_bytes < 4096 * 4) { set_error("sqdiff_mean: workspace too small"); return VQVAE_E_WORKSPACE; }
  const int np = grid_for(n, 256, 1024);
  hipLaunchKernelGGL(sqdiff_stage1, dim3(np), dim3(256), 0, (hipStream_t)s, a, b, n, (float*)ws);
  VQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(sum_stage2, dim3(1), dim3(256), 0, (hipStream_t)s, (const float*)ws, np, (float)(1.0 / (double)n), out);
  VQ_LAUNCH_CHECK();
  return 0;
}
int vqvae_sqdiff_mean_bwd(const float* a, const float* b, const float* gloss, size_t n, float* ga, float* gb, vqvae_stream_t s) {
  VQ_REQUIRE(a && b && gloss && n > 0 && (ga || gb), "sqdiff_mean_bwd: bad arguments");
  hipLaunchKernelGGL(sqdiff_bwd_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)s, a, b, gloss, n, (float)(1.0 / (double)n), ga, gb);
  VQ_LAUNCH_CHECK();
  return 0;
}

int vqvae_upsample_linear_fwd(const float* x, int B, int C, int Tin, int Tout, const int32_t* v0,
                              const int32_t* v1, const float* w0, const float* w1, float* y,
                              long y_bstride, vqvae_stream_t s) {
  VQ_REQUIRE(x && v0 && v1 && w0 && w1 && y, "upsample_fwd: null pointer");
  const size_t n = (size_t)B * C * Tout;
  hipLaunchKernelGGL(upsample_fwd_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)s, x, B, C, Tin, Tout, v0, v1, w0, w1, y, y_bstride);
  VQ_LAUNCH_CHECK();
  return 0;
}

int vqvae_upsample_linear_bwd(const float* gy, long gy_bstride, int B, int C, int Tin, int Tout,
                              const float* w0, const float* w1, const int32_t* lo0,
                              const int32_t* hi0, const int32_t* lo1, const int32_t* hi1, float* gx,
                              long gx_bstride, vqvae_stream_t s) {
  VQ_REQUIRE(gy && w0 && w1 && lo0 && hi0 && lo1 && hi1 && gx, "upsample_bwd: null pointer");
  const size_t n = (size_t)B * C * Tin;
  bool served = false;
  if (int e = launch_upsample_bwd_seg(0, gy, 16, 0L, gy_bstride, 1, B, C, Tin, Tout, w0, w1, lo0, hi0, lo1, hi1, gx, 0L, gx_bstride, nullptr, s, served)) return e;
  if (served) return 0;
  const size_t tpad = (size_t)Tout + Tout / 8 + 8;
  const size_t lds = (2 * tpad + 2) * sizeof(float);
  if (lds <= 78 * 1024) {                      // two workgroups per CU
    int nb = B * C;
    if (nb > 8192) nb = 8192;
    const bool pipe = (Tout % 4 == 0) && (Tout / 4 <= UPB_NT * UPB_KV);
    if (pipe && nb > 512) nb = 512;            // persistent: 2 workgroups per CU, next row prefetched
    if (int e = lds_opt_in<upsample_bwd_rows_kernel>(lds)) return e;
    hipLaunchKernelGGL(upsample_bwd_rows_kernel, dim3(nb), dim3(UPB_NT), lds, (hipStream_t)s, gy, gy_bstride, B, C, Tin, Tout, w0, w1, lo0, hi0, lo1, hi1, gx, gx_bstride);
  } else {
    hipLaunchKernelGGL(upsample_bwd_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)s, gy, gy_bstride, B, C, Tin, Tout, w0, w1, lo0, hi0, lo1, hi1, gx, gx_bstride);
  }
  VQ_LAUNCH_CHECK();
  return 0;
}

// gy stored as bf16 (the bf16 mode's gh: vqvae_resblock_desc::storage & VQVAE_STORE_GH_BF16); the decoder's pull-back
// shape only (the segmented kernel above)
int vqvae_upsample_linear_bwd_bf16(const void* gy, long gy_bstride, int B, int C, int Tin, int Tout,
                                   const float* w0, const float* w1, const int32_t* lo0,
                                   const int32_t* hi0, const int32_t* lo1, const int32_t* hi1, float* gx,
                                   long gx_bstride, vqvae_stream_t s) {
  VQ_REQUIRE(gy && w0 && w1 && lo0 && hi0 && lo1 && hi1 && gx, "upsample_bwd_bf16: null pointer");
  bool served = false;
  if (int e = launch_upsample_bwd_seg(1, gy, 8, 0L, gy_bstride, 1, B, C, Tin, Tout, w0, w1, lo0, hi0, lo1, hi1, gx, 0L, gx_bstride, nullptr, s, served)) return e;
  VQ_REQUIRE(served, "upsample_bwd_bf16: serves ratios >= 8 with Tout %% 4 == 0, Tout <= %d", 8 * UPS_NT);
  return 0;
}

// The pull-back of L equally shaped tensors in ONE launch (every block's gh of a ResidualNet once the chain has run: a launch
// per block was 20-40 launches of ~30 us on data the chain had left in the Infinity Cache; this one streams them from HBM
// at a higher rate and leaves the chain alone).  bf16 != 0: gy holds bf16 (2-byte elements, strides in those elements).
int vqvae_upsample_linear_bwd_blocks(const void* gy, int bf16, long gy_lstride, long gy_bstride, int L, int B, int C, int Tin, int Tout,
                                     const float* w0, const float* w1, const int32_t* lo0, const int32_t* hi0,
                                     const int32_t* lo1, const int32_t* hi1, float* gx, long gx_lstride, long gx_bstride,
                                     vqvae_stream_t s) {
  VQ_REQUIRE(gy && w0 && w1 && lo0 && hi0 && lo1 && hi1 && gx && L >= 1, "upsample_bwd_blocks: null pointer");
  bool served = false;
  if (int e = launch_upsample_bwd_seg(bf16 ? 1 : 0, gy, 16, gy_lstride, gy_bstride, L, B, C, Tin, Tout, w0, w1, lo0, hi0, lo1, hi1, gx, gx_lstride, gx_bstride, nullptr, s, served)) return e;
  VQ_REQUIRE(served, "upsample_bwd_blocks: serves ratios >= 8 with Tout %% 4 == 0, Tout <= %d", 8 * UPS_NT);
  return 0;
}

// gy stored pre-split (matmul mode 3's gh: vqvae_resblock_desc::storage & VQVAE_STORE_GH_F16X2; `scale`: its scale
// words); the decoder's pull-back shape only
int vqvae_upsample_linear_bwd_f16x2(const void* gy, long gy_bstride, int B, int C, int Tin, int Tout,
                                    const float* w0, const float* w1, const int32_t* lo0,
                                    const int32_t* hi0, const int32_t* lo1, const int32_t* hi1, float* gx,
                                    long gx_bstride, const uint32_t* scale, vqvae_stream_t s) {
  VQ_REQUIRE(gy && w0 && w1 && lo0 && hi0 && lo1 && hi1 && gx && scale, "upsample_bwd_f16x2: null pointer");
  bool served = false;
  if (int e = launch_upsample_bwd_seg(2, gy, 16, 0L, gy_bstride, 1, B, C, Tin, Tout, w0, w1, lo0, hi0, lo1, hi1, gx, 0L, gx_bstride, scale, s, served)) return e;
  VQ_REQUIRE(served, "upsample_bwd_f16x2: serves ratios >= 8 with Tout %% 4 == 0, Tout <= %d", 8 * UPS_NT);
  return 0;
}

int vqvae_embed_broadcast_fwd(const float* E, const int32_t* ids, int B, int G, int T, float* y,
                              long y_bstride, vqvae_stream_t s) {
  VQ_REQUIRE(E && ids && y, "embed_fwd: null pointer");
  const size_t n = (size_t)B * G * T;
  hipLaunchKernelGGL(embed_bcast_fwd_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)s, E, ids, B, G, T, y, y_bstride);
  VQ_LAUNCH_CHECK();
  return 0;
}

int vqvae_embed_broadcast_bwd(const float* gy, long gy_bstride, const int32_t* ids, int B, int G,
                              int T, int n_id, float* gE, int accumulate, void* ws, size_t ws_bytes,
                              vqvae_stream_t s) {
  VQ_REQUIRE(gy && ids && gE && ws, "embed_bwd: null pointer");
  if (ws_bytes < (size_t)B * G * 4) { set_error("embed_bwd: workspace too small"); return VQVAE_E_WORKSPACE; }
  hipLaunchKernelGGL(rowsum_kernel, dim3(cdiv(B * G, 4)), dim3(256), 0, (hipStream_t)s, gy, gy_bstride, B, G, T, (float*)ws);
  VQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(embed_scatter_kernel, dim3(grid_for((size_t)n_id * G)), dim3(256), 0, (hipStream_t)s, (const float*)ws, ids, B, G, n_id, gE, accumulate);
  VQ_LAUNCH_CHECK();
  return 0;
}

size_t vqvae_softmax_xent_workspace_bytes(int B, int q, int T) { (void)B; (void)q; (void)T; return 4096 * 4; }

int vqvae_softmax_xent_fwd(const float* y, const int32_t* t, int B, int q, int T, float* lse,
                           float* loss, void* ws, size_t ws_bytes, vqvae_stream_t s) {
  VQ_REQUIRE(y && t && lse && loss && ws, "softmax_xent_fwd: null pointer");
  if (ws_bytes < 4096 * 4) { set_error("softmax_xent_fwd: workspace too small"); return VQVAE_E_WORKSPACE; }
  const size_t N = (size_t)B * T;
  const int np = grid_for(N, 64, 1024);
  hipLaunchKernelGGL(xent_fwd_kernel, dim3(np), dim3(256), 0, (hipStream_t)s, y, t, B, q, T, lse, (float*)ws);
  VQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(sum_stage2, dim3(1), dim3(256), 0, (hipStream_t)s, (const float*)ws, np, (float)(1.0 / (double)N), loss);
  VQ_LAUNCH_CHECK();
  return 0;
}

int vqvae_softmax_xent_bwd_amax(const float* y, const int32_t* t, const float* lse, const float* gloss,
                                int B, int q, int T, float* gy, uint32_t* amax_out, vqvae_stream_t s) {
  VQ_REQUIRE(y && t && lse && gy, "softmax_xent_bwd: null pointer");
  const size_t n = (size_t)B * q * T;
  if (T % 4 == 0)
    hipLaunchKernelGGL(xent_bwd4_kernel, dim3(grid_for(n / 4, 256, 8192)), dim3(256), 0, (hipStream_t)s, y, t, lse, gloss, B, q, T, (float)(1.0 / ((double)B * T)), gy, amax_out);
  else
    hipLaunchKernelGGL(xent_bwd_kernel, dim3(grid_for(n, 256, 4096)), dim3(256), 0, (hipStream_t)s, y, t, lse, gloss, B, q, T, (float)(1.0 / ((double)B * T)), gy, amax_out);
  VQ_LAUNCH_CHECK();
  return 0;
}
int vqvae_softmax_xent_bwd(const float* y, const int32_t* t, const float* lse, const float* gloss,
                           int B, int q, int T, float* gy, vqvae_stream_t s) {
  return vqvae_softmax_xent_bwd_amax(y, t, lse, gloss, B, q, T, gy, nullptr, s);
}

int vqvae_mol_nll_fwd(const float* y, const float* t, int B, int n_mixture, int T, int quantize,
                      float log_scale_min, float* loss, void* ws, size_t ws_bytes,
                      vqvae_stream_t s) {
  VQ_REQUIRE(y && t && loss && ws, "mol_nll_fwd: null pointer");
  VQ_REQUIRE(n_mixture >= 1 && n_mixture <= 16 && quantize >= 2, "mol_nll_fwd: 1..16 mixtures supported");
  if (ws_bytes < 4096 * 4) { set_error("mol_nll_fwd: workspace too small"); return VQVAE_E_WORKSPACE; }
  const size_t N = (size_t)B * T;
  const int np = grid_for(N, 256, 1024);
  hipLaunchKernelGGL(mol_kernel<0>, dim3(np), dim3(256), 0, (hipStream_t)s, y, t, B, n_mixture, T,
                     (float)(127.5 / (quantize - 1)), log_scale_min, (const float*)nullptr, 0.f,
                     (float*)ws, (float*)nullptr);
  VQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(sum_stage2, dim3(1), dim3(256), 0, (hipStream_t)s, (const float*)ws, np, (float)(-1.0 / (double)N), loss);
  VQ_LAUNCH_CHECK();
  return 0;
}

int vqvae_mol_nll_bwd(const float* y, const float* t, const float* gloss, int B, int n_mixture,
                      int T, int quantize, float log_scale_min, float* gy, vqvae_stream_t s) {
  VQ_REQUIRE(y && t && gy, "mol_nll_bwd: null pointer");
  VQ_REQUIRE(n_mixture >= 1 && n_mixture <= 16 && quantize >= 2, "mol_nll_bwd: 1..16 mixtures supported");
  const size_t N = (size_t)B * T;
  hipLaunchKernelGGL(mol_kernel<1>, dim3(grid_for(N, 256, 2048)), dim3(256), 0, (hipStream_t)s, y, t, B,
                     n_mixture, T, (float)(127.5 / (quantize - 1)), log_scale_min, gloss,
                     (float)(1.0 / (double)N), (float*)nullptr, gy);
  VQ_LAUNCH_CHECK();
  return 0;
}

int vqvae_mulaw_bins(const float* x, size_t n, const float* thresholds, int n_thresholds,
                     int32_t* q, vqvae_stream_t s) {
  VQ_REQUIRE(x && thresholds && q && n_thresholds >= 1 && n_thresholds <= 8192, "mulaw_bins: bad arguments");
  hipLaunchKernelGGL(mulaw_bins_kernel, dim3(grid_for(n)), dim3(256), (size_t)n_thresholds * 4, (hipStream_t)s, x, n, thresholds, n_thresholds, q);
  VQ_LAUNCH_CHECK();
  return 0;
}

int vqvae_onehot(const int32_t* idx, long idx_bstride, int B, int q, int T, float* out,
                 vqvae_stream_t s) {
  VQ_REQUIRE(idx && out && B > 0 && q > 0 && T > 0, "onehot: bad arguments");
  hipLaunchKernelGGL(onehot_kernel, dim3(grid_for((size_t)B * q * T, 256, 4096)), dim3(256), 0, (hipStream_t)s, idx, idx_bstride, B, q, T, out);
  VQ_LAUNCH_CHECK();
  return 0;
}

// An upper bound of max |y| of the embed conv over index input, from the weights alone: every output is b[co] plus ONE entry
// of W[co, :, tap] per tap, so |y[., co, .]| <= |b[co]| + sum_tap max_q |W[co, q, tap]|.  A wave per output channel
// (lanes along q).  What matmul mode 3 needs of the first gate GEMM's operand -- instead of
// a scan of the (B, Cout, T) tensor (126 MB at configs[1]).
__global__ __launch_bounds__(256) void embed_bound_kernel(const float* __restrict__ W, const float* __restrict__ b, int Cout, int q, int K,
                                                          uint32_t* __restrict__ amax_out) {
  // a wave per output channel (lanes along q), four channels per workgroup; amax_out was zeroed by the caller
  __shared__ float red[4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int co = blockIdx.x * 4 + wave;
  float bound = 0.f;
  if (co < Cout) {
    const float* w = W + (long)co * q * K;
    bound = b ? fabsf(b[co]) : 0.f;
    for (int tap = 0; tap < K; ++tap) {
      float m = 0.f;
      for (int i = lane; i < q; i += 64) m = fmaxf(m, fabsf(w[(long)i * K + tap]));
      for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
      bound += m;
    }
  }
  if (lane == 0) red[wave] = bound;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    atomicMax(amax_out + (blockIdx.x & 15), __float_as_uint(fmaxf(m * 1.001f, 1e-30f)));
  }
}
int vqvae_embed_gather_bound(const float* W, const float* b, int Cout, int q, int K, uint32_t* amax_out, vqvae_stream_t s) {
  VQ_REQUIRE(W && amax_out && Cout > 0 && q > 0 && K >= 1, "embed_gather_bound: bad arguments");
  VQ_CHECK_HIP(hipMemsetAsync(amax_out, 0, 16 * sizeof(uint32_t), (hipStream_t)s));
  hipLaunchKernelGGL(embed_bound_kernel, dim3((Cout + 3) / 4), dim3(256), 0, (hipStream_t)s, W, b, Cout, q, K, amax_out);
  VQ_LAUNCH_CHECK();
  return 0;
}

int vqvae_embed_gather_fwd(const int32_t* idx, long idx_bstride, int B, int T, const float* W,
                           const float* b, int Cout, int q, int K, float* y, vqvae_stream_t s) {
  VQ_REQUIRE(idx && W && y && B > 0 && T > 0 && Cout > 0 && q > 0 && K >= 1, "embed_gather_fwd: bad arguments");
  if (K == 2 && T % 4 == 0 && idx_bstride == (long)T && (((uintptr_t)y) % 16 == 0) && (((uintptr_t)idx) % 16 == 0)) {
    if (q <= 4096 && T >= 1024) hipLaunchKernelGGL(embed_gather2x4_lds_kernel, dim3((unsigned)min((long)B * Cout, 8192L)), dim3(256), (size_t)q * 8, (hipStream_t)s, idx, B, T, W, b, Cout, q, y, (const int32_t*)nullptr);
    else
    hipLaunchKernelGGL(embed_gather2x4_kernel, dim3(grid_for((size_t)B * Cout * (T / 4), 256, 8192)), dim3(256), 0, (hipStream_t)s, idx, B, T, W, b, Cout, q, y, (const int32_t*)nullptr);
    VQ_LAUNCH_CHECK();
    return 0;
  }
  hipLaunchKernelGGL(embed_gather_kernel, dim3(grid_for((size_t)B * Cout * T, 256, 4096)), dim3(256), 0, (hipStream_t)s, idx, idx_bstride, B, T, W, b, Cout, q, K, y, (const int32_t*)nullptr);
  VQ_LAUNCH_CHECK();
  return 0;
}

// workspace: [per-row partial histograms | class-sorted positions | class offsets (K == 2 gather form) | dense-conv fallback]
struct EmbedPlan { vqvae_conv1d_desc conv_desc; size_t part, perm, off, conv, total; };
static EmbedPlan embed_plan(int B, int Cout, int q, int K, int T) {
  WsPlan w;
  EmbedPlan p = {{B, q, T, Cout, T, K, 1, K - 1, 1, 0}};       // the dense causal conv: pad K-1, cropped to T
  p.part = w.take((size_t)B * Cout * K * q * sizeof(float));
  p.perm = w.take((size_t)B * T * sizeof(unsigned short));
  p.off = w.take((size_t)B * (q + 1) * sizeof(int32_t));
  p.conv = w.take(vqvae_conv1d_workspace_bytes(&p.conv_desc));
  p.total = w.total + 256;
  return p;
}
size_t vqvae_embed_onehot_workspace_bytes(int B, int Cout, int q, int K, int T) { return embed_plan(B, Cout, q, K, T).total; }

int vqvae_embed_onehot_fwd(const float* x, const float* W, const float* b, int B, int Cout, int q,
                           int K, int T, float* y, int32_t* idx, int32_t* flag, void* ws,
                           size_t ws_bytes, vqvae_stream_t s) {
  VQ_REQUIRE(x && W && y && idx && flag && ws && B > 0 && Cout > 0 && q > 0 && K >= 1 && T > 0, "embed_onehot_fwd: bad arguments");
  const EmbedPlan p = embed_plan(B, Cout, q, K, T);
  if (ws_bytes < p.total) { set_error("embed_onehot_fwd: workspace too small"); return VQVAE_E_WORKSPACE; }
  hipStream_t st = (hipStream_t)s;
  hipLaunchKernelGGL(set_flag_kernel, dim3(1), dim3(1), 0, st, flag, 1);
  const bool vec4 = (T % 4 == 0) && (((uintptr_t)x) % 16 == 0) && (((uintptr_t)y) % 16 == 0);
  if (vec4) {
    const long nquad = (long)B * T / 4;
    hipLaunchKernelGGL(onehot_scan4_kernel, dim3((unsigned)((nquad + 63) / 64)), dim3(256), 0, st, x, B, q, T, idx, flag);
  } else {
    hipLaunchKernelGGL(onehot_scan_kernel, dim3(grid_for((size_t)B * T, 256, 2048)), dim3(256), 0, st, x, B, q, T, idx, flag);
  }
  VQ_LAUNCH_CHECK();
  // one-hot: gather of K weight columns (bit-identical to the dense conv) ...
  if (vec4 && K == 2) {
    if (q <= 4096 && T >= 1024) hipLaunchKernelGGL(embed_gather2x4_lds_kernel, dim3((unsigned)min((long)B * Cout, 8192L)), dim3(256), (size_t)q * 8, st, idx, B, T, W, b, Cout, q, y, (const int32_t*)flag);
    else
    hipLaunchKernelGGL(embed_gather2x4_kernel, dim3(grid_for((size_t)B * Cout * (T / 4), 256, 8192)), dim3(256), 0, st, idx, B, T, W, b, Cout, q, y, (const int32_t*)flag);
  } else {
    hipLaunchKernelGGL(embed_gather_kernel, dim3(grid_for((size_t)B * Cout * T, 256, 4096)), dim3(256), 0, st, idx, (long)T, B, T, W, b, Cout, q, K, y, (const int32_t*)flag);
  }
  VQ_LAUNCH_CHECK();
  // ... anything else: the dense causal conv, skipped on the device when flag != 0
  return vqvae_conv1d_fwd_cond(&p.conv_desc, x, W, b, y, (char*)ws + p.conv, ws_bytes - p.conv, flag, s);
}

int vqvae_embed_onehot_wgrad(const float* x, const int32_t* idx, const int32_t* flag, const float* gy,
                             int B, int Cout, int q, int K, int T, float* gW, float* gb,
                             int accumulate, void* ws, size_t ws_bytes, vqvae_stream_t s) {
  VQ_REQUIRE(idx && gy && gW && ws && B > 0 && Cout > 0 && q > 0 && K >= 1 && T > 0, "embed_onehot_wgrad: bad arguments");
  VQ_REQUIRE(flag == nullptr || x != nullptr, "embed_onehot_wgrad: a flag needs the dense input for its fallback");
  const EmbedPlan p = embed_plan(B, Cout, q, K, T);
  if (ws_bytes < p.total) { set_error("embed_onehot_wgrad: workspace too small"); return VQVAE_E_WORKSPACE; }
  hipStream_t st = (hipStream_t)s;
  float* part = (float*)((char*)ws + p.part);
  const size_t lds = (size_t)4 * K * q * sizeof(float);
  VQ_REQUIRE(lds <= 64 * 1024, "embed_onehot_wgrad: K*q too large for the LDS histograms");
  const long rows = (long)B * Cout;
  int nb = (int)((rows + 3) / 4);
  if (nb > 2048) nb = 2048;
  const size_t lds2 = (size_t)BC_WAVES * BC_NCOPY * 2 * q * sizeof(float);
  int lpc = 1;
  while (lpc * 2 * q <= ES_NT && lpc < 64) lpc *= 2;       // lanes per class: 4 at q = 256
  const size_t lds_sort = (size_t)(ES_NW * q + ES_NT) * sizeof(int) + (size_t)T * 2;
  const size_t lds_gath = (size_t)2 * (T + 4) * sizeof(float) + (((size_t)T * 2 + 15) & ~(size_t)15) + (size_t)(q + 1) * sizeof(int);
  if (K == 2 && T % 4 == 0 && T <= 65535 && q <= ES_NT && (((uintptr_t)gy) % 16 == 0) &&
      lds_sort <= 64 * 1024 && lds_gath <= 150 * 1024) {
    unsigned short* perm = (unsigned short*)((char*)ws + p.perm);
    int32_t* off = (int32_t*)((char*)ws + p.off);
    hipLaunchKernelGGL(embed_sort_kernel, dim3(B), dim3(ES_NT), lds_sort, st, idx, q, T, perm, off, flag);
    VQ_LAUNCH_CHECK();
    const int groups = (Cout + EG_ROWS - 1) / EG_ROWS;
    if (int e = lds_opt_in<embed_gathersum_kernel>(lds_gath)) return e;
    hipLaunchKernelGGL(embed_gathersum_kernel, dim3(B * groups), dim3(ES_NT), lds_gath, st, gy, B, Cout, q, T, lpc,
                       (const unsigned short*)perm, (const int32_t*)off, part, flag);
  } else
  if (K == 2 && T % 4 == 0 && (((uintptr_t)gy) % 16 == 0) && (((uintptr_t)idx) % 16 == 0) && lds2 <= 64 * 1024) {   // int4 loads of idx, float4 loads of gy
    int nb2 = (int)((rows + BC_WAVES - 1) / BC_WAVES);
    if (nb2 > 4096) nb2 = 4096;
    hipLaunchKernelGGL(embed_bincount2x4_kernel, dim3(nb2), dim3(64 * BC_WAVES), lds2, st, idx, gy, B, Cout, q, T, part, flag);
  } else {
    hipLaunchKernelGGL(embed_bincount_kernel, dim3(nb), dim3(256), lds, st, idx, gy, B, Cout, q, K, T, part, flag);
  }
  VQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(embed_bincount_reduce_kernel, dim3(grid_for((size_t)Cout * K * q, 256, 2048)), dim3(256), 0, st,
                     (const float*)part, B, Cout, q, K, gW, accumulate, flag);
  VQ_LAUNCH_CHECK();
  if (gb != nullptr) {
    hipLaunchKernelGGL(embed_bincount_bias_kernel, dim3(Cout), dim3(64), 0, st, (const float*)part, B, Cout, q, K, gb, accumulate, flag);
    VQ_LAUNCH_CHECK();
  }
  if (flag == nullptr) return 0;                          // index-fed input: there is no dense form to fall back to
  return vqvae_conv1d_bwd_weight_cond(&p.conv_desc, x, gy, gW, gb, accumulate, (char*)ws + p.conv, ws_bytes - p.conv, flag, s);
}

int vqvae_concat(float* dst, const float* const* srcs, int n, size_t count, vqvae_stream_t s) {
  VQ_REQUIRE(dst && srcs && n >= 1 && n <= 32, "concat: bad arguments (1..32 arrays)");
  PtrList32 pl;
  for (int i = 0; i < n; ++i) { VQ_REQUIRE(srcs[i], "concat: null source"); pl.p[i] = (float*)srcs[i]; }
  hipLaunchKernelGGL(concat_kernel, dim3(grid_for((size_t)n * count)), dim3(256), 0, (hipStream_t)s, pl, n, (long)count, dst);
  VQ_LAUNCH_CHECK();
  return 0;
}

int vqvae_copy_list(int n, float* const* dst, const float* const* src, const size_t* count, vqvae_stream_t s) {
  VQ_REQUIRE(n >= 0 && (n == 0 || (dst && src && count)), "copy_list: null pointer");
  for (int lo = 0; lo < n; lo += 64) {
    CopyJobs j;
    const int m = n - lo < 64 ? n - lo : 64;
    size_t mx = 0;
    for (int i = 0; i < m; ++i) {
      VQ_REQUIRE(dst[lo + i] && src[lo + i] && count[lo + i] < (1ul << 32), "copy_list: bad job %d", lo + i);
      j.dst[i] = dst[lo + i]; j.src[i] = src[lo + i]; j.n[i] = (unsigned)count[lo + i];
      if (count[lo + i] > mx) mx = count[lo + i];
    }
    int gx = (int)((mx + 1023) / 1024);
    if (gx < 1) gx = 1;
    if (gx > 256) gx = 256;
    hipLaunchKernelGGL(copy_list_kernel, dim3(gx, m), dim3(256), 0, (hipStream_t)s, j);
    VQ_LAUNCH_CHECK();
  }
  return 0;
}

int vqvae_f32x2_contract_check(int n, const uint32_t* const* scale, const uint32_t* const* amax, int log2_limit,
                               uint32_t* report, vqvae_stream_t s) {
  VQ_REQUIRE(n >= 0 && (n == 0 || (scale && amax)) && report && log2_limit >= 0 && log2_limit <= 60, "f32x2_contract_check: bad arguments");
  for (int lo = 0; lo < n; lo += 64) {
    ContractPairs cp;
    const int m = n - lo < 64 ? n - lo : 64;
    for (int i = 0; i < 64; ++i) { cp.scale[i] = i < m ? scale[lo + i] : nullptr; cp.amax[i] = i < m ? amax[lo + i] : nullptr; }
    hipLaunchKernelGGL(f32x2_contract_kernel, dim3(1), dim3(64), 0, (hipStream_t)s, cp, m, log2_limit, report);
    VQ_LAUNCH_CHECK();
  }
  return 0;
}

int vqvae_split(const float* src, float* const* dsts, int n, size_t count, int accumulate,
                vqvae_stream_t s) {
  VQ_REQUIRE(src && dsts && n >= 1 && n <= 32, "split: bad arguments (1..32 arrays)");
  PtrList32 pl;
  for (int i = 0; i < n; ++i) pl.p[i] = dsts[i];
  hipLaunchKernelGGL(split_kernel, dim3(grid_for((size_t)n * count)), dim3(256), 0, (hipStream_t)s, src, pl, n, (long)count, accumulate);
  VQ_LAUNCH_CHECK();
  return 0;
}

int vqvae_adam_step(float* p, const float* g, float* m, float* v, size_t n, double lr_t,
                    double beta1, double beta2, double eps, vqvae_stream_t s) {
  VQ_REQUIRE(p && g && m && v, "adam_step: null pointer");
  if (!n) return 0;
  hipLaunchKernelGGL(adam_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)s, p, g, m, v, n,
                     (float)lr_t, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps, (const float*)nullptr, (const int32_t*)nullptr);
  VQ_LAUNCH_CHECK();
  return 0;
}

int vqvae_adam_step_dev(float* p, const float* g, float* m, float* v, size_t n, const float* lr_table,
                        int32_t* step, double beta1, double beta2, double eps, vqvae_stream_t s) {
  VQ_REQUIRE(p && g && m && v && lr_table && step, "adam_step_dev: null pointer");
  if (!n) return 0;
  hipLaunchKernelGGL(adam_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)s, p, g, m, v, n,
                     0.f, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps, lr_table, (const int32_t*)step);
  VQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(step_inc_kernel, dim3(1), dim3(1), 0, (hipStream_t)s, step);
  VQ_LAUNCH_CHECK();
  return 0;
}

int vqvae_ema_step(float* ema, const float* target, size_t n, double decay, vqvae_stream_t s) {
  VQ_REQUIRE(ema && target, "ema_step: null pointer");
  if (!n) return 0;
  hipLaunchKernelGGL(ema_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)s, ema, target, n,
                     (float)decay, (float)(1.0 - decay));
  VQ_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
