// The condition column of a lockstep step, computed from the latent-rate condition (include/vqvae_gen_cond.h).
//
// A generation step reads exactly one column of the (n, Cc, T) condition tensor, and that tensor is an align-corners
// x`upscale` linear up-sampling of a (Cl, tl) latent block plus a speaker vector that is constant in time.  This launch,
// issued in front of the step's own kernels, evaluates the up-sampling at the one time index each column is at and
// writes a compact (rows, Cc) array; the gate kernel reads it through the descriptor's unit-stride form.  The interpolation
// position is the float64 expression NumPy's linspace evaluates (functions.resize_tables_host), the value is
// upsample_fwd_kernel's expression (csrc/misc.hip), so the column carries the dense tensor's bits.
//
// One workgroup per column of the step; the 256 threads walk the Cc channels.  The position, the two taps and the two
// weights depend on the column only and are computed by every thread (two float64 operations).  A latent row is tl
// floats long, so the two loads of a thread are a gather with stride tl; it is 2 Cl loads per column per step.
// No LDS, no atomics; every store goes to column[row * Cc + ch] with ch < Cc and row < the row count the header names.
#include "common.h"
#include "../../include/vqvae_gen_cond.h"

namespace vq {

constexpr int GC_THREADS = 256;

struct GenCondArgs {
  const float* local; const int64_t* local_off; const int32_t* tl; const float* global_vec; const int32_t* col_seq;
  float* column;
  const int* slot_seq; const int* slot_t; const int* live;      // the slots form; all nullptr in the plain form
  const int* step;
  int n, n_seq, Cl, G, upscale, max_steps;
};

__global__ __launch_bounds__(GC_THREADS) void gen_cond_column_kernel(GenCondArgs a) {
  const int tick = *a.step;
  if (tick >= a.max_steps) return;
  const bool slots = a.slot_seq != nullptr;
  if (slots && *a.live == 0) return;
  const int c = blockIdx.x;
  if (c >= a.n) return;
  int q, t, row;
  if (slots) {
    q = a.slot_seq[c]; t = a.slot_t[c]; row = q;
  } else {
    q = a.col_seq ? a.col_seq[c] : c; t = tick; row = c;
  }
  if (q < 0 || q >= a.n_seq || t < 0) return;                      // an idle slot, or an id that names no sequence
  const int Cc = a.Cl + a.G;
  float* out = a.column + (size_t)row * Cc;
  const int tl = a.tl[q];
  const long long Tq = (long long)a.upscale * tl;
  const bool inside = (long long)t < Tq;                         // tl < 1 gives Tq <= 0: nothing is read
  int v0 = 0, v1 = 0;
  float w0 = 0.f, w1 = 1.f;
  if (inside && tl > 1) {
    double v = (double)t * ((double)(tl - 1) / (double)(Tq - 1));
    if ((long long)t == Tq - 1) v = (double)(tl - 1);
    int f = (int)floor(v);
    f = f < 0 ? 0 : (f > tl - 2 ? tl - 2 : f);
    v0 = f; v1 = f + 1;
    w0 = (float)((double)v1 - v);
    w1 = (float)(v - (double)v0);
  }
  const float* x = a.local + a.local_off[q];
  const float* g = a.global_vec + (size_t)q * a.G;
  for (int ch = threadIdx.x; ch < Cc; ch += GC_THREADS) {
    float val;
    if (ch >= a.Cl) {
      val = g[ch - a.Cl];
    } else if (!inside) {
      val = 0.f;
    } else {
      const float* xr = x + (size_t)ch * tl;
      val = __fadd_rn(__fmul_rn(w0, xr[v0]), __fmul_rn(w1, xr[v1]));
    }
    out[ch] = val;
  }
}

}  // namespace vq

using namespace vq;

extern "C" int vqvae_gen_cond_abi_version(void) { return 1; }

extern "C" int vqvae_gen_cond_column(const vqvae_gen_latent_cond* c, const vqvae_gen_desc* d, const vqvae_gen_slots* slots,
                                     vqvae_stream_t stream) {
  VQ_REQUIRE(c && d, "gen_cond_column: null latent condition or descriptor");
  VQ_REQUIRE(d->step, "gen_cond_column: null step counter (d->step)");
  VQ_REQUIRE(d->n >= 1 && d->n <= VQVAE_GEN_MAX_LOCKSTEP, "gen_cond_column: d->n must be 1..%d columns (got %d)",
             VQVAE_GEN_MAX_LOCKSTEP, d->n);
  VQ_REQUIRE(c->n_seq >= 0 && c->Cl >= 0 && c->G >= 0, "gen_cond_column: negative count (n_seq %d, Cl %d, G %d)", c->n_seq,
             c->Cl, c->G);
  VQ_REQUIRE(c->upscale >= 1, "gen_cond_column: upscale must be >= 1 (got %d)", c->upscale);
  VQ_REQUIRE((long)c->Cl + c->G == d->cond_dim, "gen_cond_column: Cl + G = %d + %d is not the decoder's cond_dim %d", c->Cl, c->G,
             d->cond_dim);
  VQ_REQUIRE(c->local && c->local_off && c->tl && c->column && (c->global_vec || c->G == 0),
             "gen_cond_column: null latent condition member");
  if (slots) {
    VQ_REQUIRE(slots->slot_seq && slots->slot_t && slots->live, "gen_cond_column: null slot table member");
    VQ_REQUIRE(slots->n_seq == c->n_seq, "gen_cond_column: the slot table has %d sequences, the latent condition %d", slots->n_seq,
               c->n_seq);
  }
  GenCondArgs a{};
  a.local = c->local; a.local_off = c->local_off; a.tl = c->tl; a.global_vec = c->global_vec; a.col_seq = c->col_seq;
  a.column = c->column;
  if (slots) { a.slot_seq = slots->slot_seq; a.slot_t = slots->slot_t; a.live = slots->live; }
  a.step = d->step;
  a.n = d->n; a.n_seq = c->n_seq; a.Cl = c->Cl; a.G = c->G; a.upscale = c->upscale; a.max_steps = d->max_steps;
  hipLaunchKernelGGL(gen_cond_column_kernel, dim3(d->n), dim3(GC_THREADS), 0, (hipStream_t)stream, a);
  VQ_LAUNCH_CHECK();
  return 0;
}
