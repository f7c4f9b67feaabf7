// Optimizer hooks on the device (include/vqvae_optim.h): the gradient arena's sum of squares per parameter, the state
// block of global-norm clipping / the non-finite guard / the group norms, and the Adam step that reads that block.
//
//   optim_sumsq_kernel     one workgroup of 256 lanes per (parameter, chunk) work item, 4 096 elements: every lane holds its
//                          (at most five) aligned quads in registers before it adds -- all of a chunk's loads are in flight
//                          at once, 16 bytes a lane where the whole quad lies inside the chunk, single floats at the two
//                          ragged ends -- squares them in float64, and the 256 lane sums are folded in halves through LDS.
//                          ~1 600 workgroups at configs[1] (5.4 M gradients): six to a CU.
//   optim_finalise_kernel  ONE workgroup: lane p adds parameter p's chunk partials in ascending order, lane 0 then adds the
//                          parameters in layout order and writes the header, lane j the j-th group's norm; the float32
//                          values a report reads also go into row (steps mod n_slots) of the report ring.
//   adam_hooked_kernel     misc.hip's adam_kernel on g * scale; returns at once on a guarded non-finite step.
// Nothing is handed between workgroups inside a launch: the kernel boundary is the only synchronisation, and no sum
// depends on how the workgroups were scheduled.
#include "common.h"
#include "../../include/vqvae_optim.h"

namespace {

constexpr int CHUNK = VQVAE_OPTIM_CHUNK;
constexpr int THREADS = VQVAE_OPTIM_THREADS;
constexpr int QUADS = CHUNK / 4 / THREADS + 1;     // quads a lane can meet: a chunk that starts inside a quad spans one more
static_assert(CHUNK % (4 * THREADS) == 0, "a chunk is a whole number of rounds of 256 quads");

struct OptimState {                                // the header of the state block (vqvae_optim.h)
  double S, norm, rate;
  float scale;
  int32_t nonfinite, skipped, steps;
  float norm_f, rate_f;
  int32_t reserved1[4];
};
static_assert(sizeof(OptimState) == VQVAE_OPTIM_STATE_HEADER, "state header layout");

__device__ __forceinline__ double sq64(float x) { const double d = (double)x; return d * d; }

__global__ __launch_bounds__(THREADS) void optim_sumsq_kernel(const float* __restrict__ g, unsigned n,
                                                               const int32_t* __restrict__ items,
                                                               double* __restrict__ partial) {
  __shared__ double tree[THREADS];
  const int t = threadIdx.x;
  // (a table entry is clipped to the arena and to one chunk: nothing outside g[0, n) is ever addressed)
  const unsigned s = min((unsigned)max(items[2 * blockIdx.x], 0), n);
  const unsigned e = s + min(min((unsigned)max(items[2 * blockIdx.x + 1], 0), (unsigned)CHUNK), n - s);
  const unsigned q0 = s >> 2;
  float4 x[QUADS];
#pragma unroll
  for (int r = 0; r < QUADS; ++r) {
    const unsigned i = (q0 + (unsigned)t + (unsigned)r * THREADS) << 2;          // first element of the quad
    x[r] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i >= s && i + 4u <= e) {
      x[r] = *reinterpret_cast<const float4*>(g + i);
    } else if (i < e && i + 4u > s) {                                              // a ragged end: the elements inside [s, e)
      if (i >= s) x[r].x = g[i];
      if (i + 1u >= s && i + 1u < e) x[r].y = g[i + 1u];
      if (i + 2u >= s && i + 2u < e) x[r].z = g[i + 2u];
      if (i + 3u >= s && i + 3u < e) x[r].w = g[i + 3u];
    }
  }
  double acc = 0.0;
#pragma unroll
  for (int r = 0; r < QUADS; ++r) {
    acc = acc + sq64(x[r].x);
    acc = acc + sq64(x[r].y);
    acc = acc + sq64(x[r].z);
    acc = acc + sq64(x[r].w);
  }
  tree[t] = acc;
  __syncthreads();
#pragma unroll
  for (int h = THREADS / 2; h >= 1; h >>= 1) {
    if (t < h) tree[t] = tree[t] + tree[t + h];
    __syncthreads();
  }
  if (t == 0) partial[blockIdx.x] = tree[0];
}

__global__ __launch_bounds__(THREADS) void optim_finalise_kernel(const double* __restrict__ partial, int n_items,
                                                                  const int32_t* __restrict__ params, int n_params,
                                                                  const int32_t* __restrict__ group_off,
                                                                  const int32_t* __restrict__ group_members, int n_groups,
                                                                  int n_slots, double threshold, int flags,
                                                                  OptimState* __restrict__ st) {
  double* __restrict__ sp = reinterpret_cast<double*>(st + 1);
  float* __restrict__ gn = reinterpret_cast<float*>(sp + n_params);
  // this launch's row of the report ring: (norm, rate, group norms); `steps` is only advanced behind the barrier below
  float* __restrict__ row = gn + n_groups + (size_t)((unsigned)st->steps % (unsigned)n_slots) * (2 + n_groups);
  const int t = threadIdx.x;
  for (int p = t; p < n_params; p += THREADS) {
    const int first = min(max(params[2 * p], 0), n_items);
    const int count = min(max(params[2 * p + 1], 0), n_items - first);
    double a = 0.0;
    for (int c = 0; c < count; ++c) a = a + partial[first + c];
    sp[p] = a;
  }
  __syncthreads();                                 // (one workgroup: the S_p just written are visible to all of its lanes)
  if (t == 0) {
    double S = 0.0;
    for (int p = 0; p < n_params; ++p) S = S + sp[p];
    const double norm = sqrt(S);
    const double rate = threshold / norm;
    const int bad = !(fabs(S) <= 1.7976931348623157e308);      // !isfinite(S): inf and NaN both fail the comparison
    st->S = S;
    st->norm = norm;
    st->rate = rate;
    st->scale = rate < 1.0 ? (float)rate : 1.0f;
    st->nonfinite = bad;
    if (bad && (flags & VQVAE_OPTIM_GUARD)) st->skipped = st->skipped + 1;
    st->norm_f = (float)norm;
    st->rate_f = (float)rate;
    row[0] = (float)norm;
    row[1] = (float)rate;
  }
  const int n_members = n_groups > 0 ? max(group_off[n_groups], 0) : 0;     // (the table's own total: every bound is clipped to it)
  for (int j = t; j < n_groups; j += THREADS) {
    const int b = min(max(group_off[j], 0), n_members), e = min(max(group_off[j + 1], 0), n_members);
    double a = 0.0;
    for (int i = b; i < e; ++i) {
      const int p = group_members[i];
      if (p >= 0 && p < n_params) a = a + sp[p];
    }
    gn[j] = (float)sqrt(a);
    row[2 + j] = (float)sqrt(a);
  }
  __syncthreads();                                 // every lane has taken its row from the old count
  if (t == 0) st->steps = st->steps + 1;
}

// misc.hip's adam_kernel, operation for operation, on gi = g[i] * scale
__global__ void adam_hooked_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                   float* __restrict__ v, size_t n, float lr, float c1, float c2, float eps,
                                   const float* __restrict__ lr_table, const int32_t* __restrict__ step,
                                   const OptimState* __restrict__ st, int flags) {
  if ((flags & VQVAE_OPTIM_GUARD) && st->nonfinite) return;
  if (lr_table != nullptr) lr = lr_table[*step];
  const float scale = st->scale;
  const bool write_back = scale != 1.0f;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x) {
    const float gi = __fmul_rn(g[i], scale);
    const float mi = __fadd_rn(m[i], __fmul_rn(c1, __fsub_rn(gi, m[i])));
    const float vi = __fadd_rn(v[i], __fmul_rn(c2, __fsub_rn(__fmul_rn(gi, gi), v[i])));
    m[i] = mi;
    v[i] = vi;
    p[i] = __fsub_rn(p[i], __fdiv_rn(__fmul_rn(lr, mi), __fadd_rn(__fsqrt_rn(vi), eps)));
    if (write_back) g[i] = gi;
  }
}

__global__ void optim_step_inc_kernel(int32_t* step) { *step += 1; }

}  // namespace

extern "C" {

int vqvae_optim_abi_version(void) { return 1; }

int vqvae_optim_plan_items(const int64_t* sizes, int n_params, int32_t* items, int32_t* params) {
  if (!sizes || n_params < 0) return -1;
  int64_t off = 0, n_items = 0;
  for (int p = 0; p < n_params; ++p) {
    const int64_t size = sizes[p];
    if (size < 0 || off + size > (int64_t)VQVAE_OPTIM_MAX_N) return -1;
    const int64_t count = (size + VQVAE_OPTIM_CHUNK - 1) / VQVAE_OPTIM_CHUNK;
    if (params) { params[2 * p] = (int32_t)n_items; params[2 * p + 1] = (int32_t)count; }
    for (int64_t c = 0; c < count; ++c) {
      const int64_t start = off + c * VQVAE_OPTIM_CHUNK;
      const int64_t len = size - c * VQVAE_OPTIM_CHUNK < VQVAE_OPTIM_CHUNK ? size - c * VQVAE_OPTIM_CHUNK : VQVAE_OPTIM_CHUNK;
      if (items) { items[2 * (n_items + c)] = (int32_t)start; items[2 * (n_items + c) + 1] = (int32_t)len; }
    }
    n_items += count;
    off += size;
  }
  return (int)n_items;
}

size_t vqvae_optim_workspace_bytes(int n_items) { return n_items < 1 ? 0 : (size_t)n_items * sizeof(double); }

size_t vqvae_optim_state_bytes(int n_params, int n_groups, int n_slots) {
  if (n_params < 1 || n_groups < 0 || n_slots < 1) return 0;
  return VQVAE_OPTIM_STATE_HEADER + (size_t)n_params * sizeof(double) + (size_t)n_groups * sizeof(float) +
         (size_t)n_slots * (2 + (size_t)n_groups) * sizeof(float);
}

int vqvae_optim_sumsq(const float* g, size_t n, const int32_t* items, int n_items, const int32_t* params,
                      int n_params, const int32_t* group_off, const int32_t* group_members, int n_groups,
                      int n_slots, double threshold, int flags, void* state, void* ws, size_t ws_bytes,
                      vqvae_optim_stream_t s) {
  VQ_REQUIRE(g && items && params && state && ws, "optim_sumsq: null pointer");
  VQ_REQUIRE(n >= 1 && n <= (size_t)VQVAE_OPTIM_MAX_N, "optim_sumsq: n = %zu outside [1, 2^31)", n);
  VQ_REQUIRE(n_items >= 1 && n_params >= 1 && n_groups >= 0 && n_slots >= 1,
             "optim_sumsq: bad table sizes (%d items, %d parameters, %d groups, %d report slots)", n_items, n_params, n_groups, n_slots);
  VQ_REQUIRE(n_groups == 0 || (group_off && group_members), "optim_sumsq: %d groups without their tables", n_groups);
  VQ_REQUIRE(((uintptr_t)g & 15) == 0 && ((uintptr_t)state & 7) == 0 && ((uintptr_t)ws & 7) == 0,
             "optim_sumsq: g must be 16-byte aligned, state and ws 8-byte aligned");
  VQ_REQUIRE(ws_bytes >= vqvae_optim_workspace_bytes(n_items), "optim_sumsq: workspace of %zu bytes, %zu needed", ws_bytes,
             vqvae_optim_workspace_bytes(n_items));
  hipLaunchKernelGGL(optim_sumsq_kernel, dim3(n_items), dim3(THREADS), 0, (hipStream_t)s, g, (unsigned)n, items,
                     (double*)ws);
  VQ_LAUNCH_CHECK();
  hipLaunchKernelGGL(optim_finalise_kernel, dim3(1), dim3(THREADS), 0, (hipStream_t)s, (const double*)ws, n_items, params,
                     n_params, group_off, group_members, n_groups, n_slots, threshold, flags, (OptimState*)state);
  VQ_LAUNCH_CHECK();
  return 0;
}

int vqvae_optim_adam_step_hooked(float* p, float* g, float* m, float* v, size_t n, double lr_t, const float* lr_table,
                                 int32_t* step, double beta1, double beta2, double eps, const void* state, int flags,
                                 vqvae_optim_stream_t s) {
  VQ_REQUIRE(p && g && m && v && state, "optim_adam_step_hooked: null pointer");
  VQ_REQUIRE((lr_table == nullptr) == (step == nullptr), "optim_adam_step_hooked: lr_table and step go together");
  if (!n) return 0;
  size_t grid = (n + 255) / 256;
  if (grid > 2048) grid = 2048;                    // (vqvae_adam_step's grid)
  hipLaunchKernelGGL(adam_hooked_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)s, p, g, m, v, n,
                     lr_table ? 0.f : (float)lr_t, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps, lr_table,
                     (const int32_t*)step, (const OptimState*)state, flags);
  VQ_LAUNCH_CHECK();
  if (step) {
    hipLaunchKernelGGL(optim_step_inc_kernel, dim3(1), dim3(1), 0, (hipStream_t)s, step);
    VQ_LAUNCH_CHECK();
  }
  return 0;
}

}  // extern "C"
