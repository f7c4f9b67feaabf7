// The mixture-of-logistics side of the ragged teacher-forced decoder pass (csrc/ragged_mol.h, which states the rule): the
// raw-sample embed of an input_dim = 1 decoder and the per-position NLL over the (3 M, ttot) output that vqvae_rdec_head
// leaves in its `logits`.  Everything between the two is csrc/ragged_decoder.hip's, unchanged.
//
// rdmol_embed_kernel: rd_embed_kernel's grid (column blocks of 256, channel groups of 64) and bounds; two products, one
//   sum, the bias (-ffp-contract=off).
// rdmol_nll_kernel:   a thread per column; the column's 3 M values are 3 M coalesced loads a row apart; mol_kernel<0>'s
//   (csrc/misc.hip) operation sequence with the component arrays fully unrolled into registers
//   (tests/test_host_scoring_mol_budget.py holds them there).
// Both are memory-bound VALU.  Every address is formed in 64 bits; stores go to (row < R, column < ttot) only; plain
// vector stores, no atomics, no LDS, no workspace.
#include "common.h"
#include "ragged_seg.h"
#include "ragged_mol.h"

namespace vq {

constexpr int RDMOL_THREADS = 256;
constexpr int RDMOL_ROWS = 64;         // channels of x one workgroup of the embed writes

__global__ __launch_bounds__(RDMOL_THREADS) void rdmol_embed_kernel(const int64_t* off, const int64_t* woff, const float* w,
                                                                    const float* W, const float* b, float* x, long long ttot,
                                                                    int n, int R) {
  const long long j = (long long)blockIdx.x * RDMOL_THREADS + threadIdx.x;
  if (j >= ttot) return;
  const int i = ragged_find_segment(off, n, j);
  const long long jl = j - (long long)off[i];
  const float* wi = w + (long long)woff[i];
  const bool first = jl == 0;
  const float s1 = wi[jl], s0 = first ? 0.f : wi[jl - 1];
  const int r0 = blockIdx.y * RDMOL_ROWS, r1 = min(r0 + RDMOL_ROWS, R);
  for (int c = r0; c < r1; ++c) {
    const float p1 = W[2 * (long long)c + 1] * s1;
    float v = first ? p1 : W[2 * (long long)c] * s0 + p1;
    if (b) v += b[c];
    x[(long long)c * ttot + j] = v;
  }
}

__device__ __forceinline__ float rdmol_sigmoid(float x) { return tanhf(x * 0.5f) * 0.5f + 0.5f; }
__device__ __forceinline__ float rdmol_softplus(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

__global__ __launch_bounds__(RDMOL_THREADS) void rdmol_nll_kernel(const int64_t* off, const int64_t* woff, const float* w,
                                                                  const float* y, float* nll, long long ttot, int n, int nmix,
                                                                  float half, float ls_min) {
  constexpr int MAXM = VQVAE_RDMOL_MAX_MIX;
  const long long j = (long long)blockIdx.x * RDMOL_THREADS + threadIdx.x;
  if (j >= ttot) return;
  const int i = ragged_find_segment(off, n, j);
  const long long jl = j - (long long)off[i];
  const float tt = 127.5f * w[(long long)woff[i] + jl + 1];
  const bool left = tt < 127.5f * -0.999f, right = tt > 127.5f * 0.999f;
  const float* yp = y + j;
  float lp[MAXM], v[MAXM];
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < MAXM; ++k) if (k < nmix) { lp[k] = yp[(long long)k * ttot]; m = fmaxf(m, lp[k]); }
  float se = 0.f;
#pragma unroll
  for (int k = 0; k < MAXM; ++k) if (k < nmix) se += expf(lp[k] - m);
  const float lz = logf(se) + m;                         // log-sum-exp of the mixture logits
  float vm = -INFINITY;
#pragma unroll
  for (int k = 0; k < MAXM; ++k) if (k < nmix) {
    const float mu = yp[(long long)(nmix + k) * ttot];
    const float ls = fmaxf(yp[(long long)(2 * nmix + k) * ttot], ls_min);
    const float c = tt - mu;
    const float is = expf(-ls);
    const float p = is * (c + half), q = is * (c - half);
    float lpr;
    if (left) lpr = p - rdmol_softplus(p);
    else if (right) lpr = -rdmol_softplus(q);
    else lpr = logf(fmaxf(rdmol_sigmoid(p) - rdmol_sigmoid(q), 1e-12f));
    v[k] = lpr + (lp[k] - lz);
    vm = fmaxf(vm, v[k]);
  }
  float sv = 0.f;
#pragma unroll
  for (int k = 0; k < MAXM; ++k) if (k < nmix) sv += expf(v[k] - vm);
  nll[j] = -(logf(sv) + vm);
}

}  // namespace vq

using namespace vq;

// the descriptor check is the ragged decoder's own: its workspace query answers (size_t)-1 for what its entry points refuse
#define RDMOL_COMMON(who)                                                                                                  \
  VQ_REQUIRE(d, who ": null descriptor");                                                                                  \
  VQ_REQUIRE(vqvae_rdec_workspace_bytes(d) != (size_t)-1, who ": a descriptor the ragged decoder refuses (got n %d, R %d, " \
             "D %d, S %d, Q %d, Cl %d, G %d, n_blocks %d, upscale %d, ttot %lld, tltot %lld)", (int)d->n, (int)d->R,       \
             (int)d->D, (int)d->S, (int)d->Q, (int)d->Cl, (int)d->G, (int)d->n_blocks, (int)d->upscale,                    \
             (long long)d->ttot, (long long)d->tltot)

extern "C" int vqvae_rdmol_revision(void) { return 1; }

extern "C" int vqvae_rdmol_embed(const vqvae_rdec_desc* d, const vqvae_rdec_tables* t, const float* w, const int64_t* woff,
                                 const float* W, const float* b, float* x, vqvae_stream_t stream) {
  RDMOL_COMMON("rdmol_embed");
  VQ_REQUIRE(t && t->off, "rdmol_embed: null tables or off");
  VQ_REQUIRE(w && woff && W && x, "rdmol_embed: null w, woff, W or x");
  const long long blocks = (d->ttot + RDMOL_THREADS - 1) / RDMOL_THREADS;
  hipLaunchKernelGGL(rdmol_embed_kernel, dim3((unsigned)blocks, (unsigned)cdiv(d->R, RDMOL_ROWS)), dim3(RDMOL_THREADS), 0,
                     (hipStream_t)stream, t->off, woff, w, W, b, x, (long long)d->ttot, (int)d->n, (int)d->R);
  VQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int vqvae_rdmol_nll(const vqvae_rdec_desc* d, const vqvae_rdec_tables* t, const float* y, const float* w,
                               const int64_t* woff, int n_mix, int quantize, float log_scale_min, float* nll,
                               vqvae_stream_t stream) {
  RDMOL_COMMON("rdmol_nll");
  VQ_REQUIRE(t && t->off, "rdmol_nll: null tables or off");
  VQ_REQUIRE(y && w && woff && nll, "rdmol_nll: null y, w, woff or nll");
  VQ_REQUIRE(n_mix >= 1 && n_mix <= VQVAE_RDMOL_MAX_MIX, "rdmol_nll: n_mix must be in 1 .. %d (got %d)", VQVAE_RDMOL_MAX_MIX, n_mix);
  VQ_REQUIRE(d->Q == 3 * n_mix, "rdmol_nll: the descriptor's Q must be 3 n_mix = %d (got %d)", 3 * n_mix, (int)d->Q);
  VQ_REQUIRE(quantize >= 2, "rdmol_nll: quantize must be at least 2 (got %d)", quantize);
  const long long blocks = (d->ttot + RDMOL_THREADS - 1) / RDMOL_THREADS;
  hipLaunchKernelGGL(rdmol_nll_kernel, dim3((unsigned)blocks), dim3(RDMOL_THREADS), 0, (hipStream_t)stream, t->off, woff, w, y,
                     nll, (long long)d->ttot, (int)d->n, n_mix, (float)(127.5 / (quantize - 1)), log_scale_min);
  VQ_LAUNCH_CHECK();
  return 0;
}
