// Statistics of the discrete codes of a ragged list of utterances (include/vqvae_codes.h states the rule).  Integer work only.
//
// codes_runs_kernel: one workgroup of 256 threads per utterance, passes of 256 positions.  A position flags a run start;
//   one LDS scan per pass carries two things, the number of starts up to a position and the last start's position, with a
//   running base across the passes.  The thread at a run's LAST position knows the run's index, code and start, and writes
//   u, dur and the histogram bucket: nothing is read back from the outputs.
// codes_hist_kernel: one workgroup per utterance, atomicAdd on 64-bit integers in global memory (exact, order-free: the
//   house rule of vq.hip's vq_gw_hist_kernel).  No LDS privatisation: nothing measured asks for it.
// codes_agree_kernel: one workgroup per pair, an integer fold through LDS.
// codes_edit_kernel: ONE workgroup of 256 threads per pair walks the anti-diagonals of the matrix's inside, cell (x, y) =
//   D(x + 1, y + 1), k = x + y = 0 .. La + Lb - 2, exactly as align_dtw_kernel does: thread t takes the cells pLo + t,
//   pLo + t + 256, ... of a diagonal (p: the coordinate on the SHORTER side), three diagonals of (D, S) int2 cells rotate
//   through LDS, diagonal k in slot k mod 3, ONE barrier per diagonal.  The borders D(i, 0) = i, D(0, j) = j, S = 0 are
//   closed forms.  No direction table, no workspace, all pairs in one launch.  Dynamic LDS: 24 * max_short bytes, asked
//   for through lds_opt_in above 64 KB (147432 bytes at VQVAE_CODES_MAX_SHORT).
//
// An utterance or pair whose table entries contradict the descriptor is skipped (the header says what is written then).
// Every address is formed in 64 bits; plain vector stores and integer atomics only.
#include "common.h"
#include "../../include/vqvae_codes.h"

namespace vq {

constexpr int CS_THREADS = VQVAE_CODES_THREADS;
constexpr size_t CS_LDS_CAP = 160 * 1024;            // the LDS of a CU, which one workgroup may take
constexpr size_t CS_CELL_BYTES = 3 * 2 * sizeof(int);   // three diagonals of (D, S)
constexpr long long CS_MAX_LEN = 0x3fffffffLL;       // La + Lb and every count of one utterance stay inside int32
static_assert(CS_CELL_BYTES * VQVAE_CODES_MAX_SHORT <= 144 * 1024 && 144 * 1024 <= CS_LDS_CAP,
              "three diagonals of the longest pair must fit the 144 KiB opt-in");
static_assert(CS_THREADS == 256, "the scans and folds below are written for 256 threads");

// utterance i of a list: ok when its codes lie inside the buffer
struct Seg { long long at; int n; bool ok; };
__device__ __forceinline__ Seg cs_seg(const int64_t* start, const int32_t* len, long long i, long long total) {
  Seg s;
  s.at = (long long)start[i]; s.n = len[i];
  s.ok = s.n >= 1 && (long long)s.n <= CS_MAX_LEN && s.at >= 0 && s.at + s.n <= total;
  return s;
}

// ---------------------------------------------------------------------------------------------------------------------
struct RunsArgs {
  vqvae_codes_runs_desc d;
  const int32_t* codes; const int64_t* start; const int32_t* len;
  int32_t* u; int32_t* dur; int32_t* m; unsigned long long* run_hist;
};

__global__ __launch_bounds__(CS_THREADS) void codes_runs_kernel(RunsArgs a) {
  __shared__ int s_cnt[CS_THREADS];                   // run starts up to and including this position of the pass
  __shared__ int s_pos[CS_THREADS];                   // the last start's position inside the utterance, -1: none in this pass
  const int tid = threadIdx.x;
  const long long i = blockIdx.x;
  const Seg g = cs_seg(a.start, a.len, i, a.d.total);
  if (!g.ok) {                                        // uniform for the workgroup
    if (tid == 0) a.m[i] = 0;
    return;
  }
  const int32_t* c = a.codes + g.at;
  int32_t* u = a.u + g.at;
  int32_t* dur = a.dur + g.at;
  int runs = 0, open = 0;                             // runs started before this pass; where the last of them started
  for (int base = 0; base < g.n; base += CS_THREADS) {
    const int t = base + tid;
    const bool in = t < g.n;
    const int32_t mine = in ? c[t] : 0;
    const bool first = in && (t == 0 || c[t - 1] != mine);
    s_cnt[tid] = first ? 1 : 0;
    s_pos[tid] = first ? t : -1;
    __syncthreads();
    for (int off = 1; off < CS_THREADS; off <<= 1) {  // inclusive scan: sum of the flags, maximum of the positions
      const int v = tid >= off ? s_cnt[tid - off] : 0;
      const int w = tid >= off ? s_pos[tid - off] : -1;
      __syncthreads();
      s_cnt[tid] += v;
      if (w > s_pos[tid]) s_pos[tid] = w;
      __syncthreads();
    }
    if (in && (t == g.n - 1 || c[t + 1] != mine)) {   // the run's last position
      const int r = runs + s_cnt[tid] - 1;            // r <= t: inside the utterance's slots
      const int from = s_pos[tid] < 0 ? open : s_pos[tid];
      const int L = t - from + 1;
      u[r] = mine;
      dur[r] = L;
      if (a.run_hist) atomicAdd(&a.run_hist[(L < a.d.max_run ? L : a.d.max_run) - 1], 1ULL);
    }
    const int more = s_cnt[CS_THREADS - 1], last = s_pos[CS_THREADS - 1];
    runs += more;
    if (last >= 0) open = last;
    __syncthreads();                                  // the next pass overwrites the two arrays
  }
  if (tid == 0) a.m[i] = runs;
}

// ---------------------------------------------------------------------------------------------------------------------
struct HistArgs {
  vqvae_codes_hist_desc d;
  const int32_t* codes; const int64_t* start; const int32_t* len; const int32_t* group;
  unsigned long long* uni; unsigned long long* big; unsigned long long* invalid;
};

__global__ __launch_bounds__(CS_THREADS) void codes_hist_kernel(HistArgs a) {
  const int tid = threadIdx.x;
  const long long i = blockIdx.x;
  const Seg g = cs_seg(a.start, a.len, i, a.d.total);
  if (!g.ok) return;                                  // uniform for the workgroup
  const int grp = a.group[i];
  if (grp < 0 || grp >= a.d.groups) {
    if (tid == 0) atomicAdd(a.invalid, (unsigned long long)g.n);
    return;
  }
  const int32_t* c = a.codes + g.at;
  const long long k = a.d.k;
  unsigned long long* row = a.uni + (long long)grp * k;
  unsigned long long bad = 0;
  for (int t = tid; t < g.n; t += CS_THREADS) {
    const long long x = c[t];
    if (x < 0 || x >= k) { ++bad; continue; }
    atomicAdd(&row[x], 1ULL);
    if (a.big && t + 1 < g.n) {
      const long long y = c[t + 1];
      if (y >= 0 && y < k) atomicAdd(&a.big[x * k + y], 1ULL);
    }
  }
  if (bad) atomicAdd(a.invalid, bad);
}

// ---------------------------------------------------------------------------------------------------------------------
struct PairGeom { long long sa, sb; int La, Lb; bool ok; };

__device__ __forceinline__ PairGeom cs_pair(const vqvae_codes_pair_tables& t, const vqvae_codes_pair_desc& d, long long i) {
  const Seg a = cs_seg(t.start_a, t.len_a, i, d.total_a), b = cs_seg(t.start_b, t.len_b, i, d.total_b);
  PairGeom g;
  g.sa = a.at; g.sb = b.at; g.La = a.n; g.Lb = b.n; g.ok = a.ok && b.ok;
  return g;
}

struct PairArgs {
  vqvae_codes_pair_desc d; vqvae_codes_pair_tables t;
  const int32_t* a; const int32_t* b;
  int32_t* out0; int32_t* out1;                       // agree, - ; dist, subs
};

__global__ __launch_bounds__(CS_THREADS) void codes_agree_kernel(PairArgs q) {
  __shared__ int s_n[CS_THREADS];
  const int tid = threadIdx.x;
  const long long pair = blockIdx.x;
  const PairGeom g = cs_pair(q.t, q.d, pair);
  if (!g.ok) {                                        // uniform for the workgroup
    if (tid == 0) q.out0[pair] = -1;
    return;
  }
  const int32_t* a = q.a + g.sa;
  const int32_t* b = q.b + g.sb;
  const int overlap = g.La < g.Lb ? g.La : g.Lb;
  int same = 0;
  for (int t = tid; t < overlap; t += CS_THREADS) same += a[t] == b[t] ? 1 : 0;
  s_n[tid] = same;
  __syncthreads();
  for (int h = CS_THREADS / 2; h >= 1; h >>= 1) {
    if (tid < h) s_n[tid] += s_n[tid + h];
    __syncthreads();
  }
  if (tid == 0) q.out0[pair] = s_n[0];
}

__global__ __launch_bounds__(CS_THREADS) void codes_edit_kernel(PairArgs q) {
  extern __shared__ __attribute__((aligned(16))) unsigned char cs_lds[];
  const int tid = threadIdx.x;
  const long long pair = blockIdx.x;
  const PairGeom g = cs_pair(q.t, q.d, pair);
  const bool by_x = g.La <= g.Lb;                           // p is x (along a), else y
  const int S = by_x ? g.La : g.Lb, L = by_x ? g.Lb : g.La;
  if (!g.ok || S > q.d.max_short) {                         // uniform for the workgroup; the LDS holds max_short cells a slot
    if (tid == 0) { q.out0[pair] = -1; q.out1[pair] = 0; }
    return;
  }
  int2* cell = reinterpret_cast<int2*>(cs_lds);             // [3][S] of (D, S)
  const int32_t* a = q.a + g.sa;
  const int32_t* b = q.b + g.sb;
  const int nd = S + L - 1;
  // where the "up" (x - 1, y) and "left" (x, y - 1) neighbours stand in the previous diagonal, relative to p
  const int up_at = by_x ? -1 : 0, left_at = by_x ? 0 : -1;

  int cur = 0, prev = 2, prev2 = 1;                         // slots of diagonals k, k - 1, k - 2
  for (int k = 0; k < nd; ++k) {
    const int pLo = k > L - 1 ? k - (L - 1) : 0;
    const int pHi = k < S - 1 ? k : S - 1;
    const int2* Cp = cell + (size_t)prev * S;
    const int2* Cq = cell + (size_t)prev2 * S;
    for (int p = pLo + tid; p <= pHi; p += CS_THREADS) {
      const int r = k - p;                                  // the coordinate on the longer side
      const int x = by_x ? p : r, y = by_x ? r : p;
      const int ne = a[x] != b[y] ? 1 : 0;
      int2 best = x > 0 && y > 0 ? Cq[p - 1] : make_int2(x > y ? x : y, 0);     // D(i-1, j-1): a border when x or y is 0
      best.x += ne; best.y += ne;
      const int2 up = x > 0 ? Cp[p + up_at] : make_int2(y + 1, 0);              // D(0, j) = j
      if (up.x + 1 < best.x) { best.x = up.x + 1; best.y = up.y; }
      const int2 left = y > 0 ? Cp[p + left_at] : make_int2(x + 1, 0);          // D(i, 0) = i
      if (left.x + 1 < best.x) { best.x = left.x + 1; best.y = left.y; }
      cell[(size_t)cur * S + p] = best;
      if (k == nd - 1) { q.out0[pair] = best.x; q.out1[pair] = best.y; }
    }
    __syncthreads();
    const int f = prev2; prev2 = prev; prev = cur; cur = f;
  }
}

static bool runs_desc_ok(const vqvae_codes_runs_desc* d) { return d && d->n >= 1 && d->max_run >= 1 && d->total >= d->n; }
static bool hist_desc_ok(const vqvae_codes_hist_desc* d) {
  return d && d->n >= 1 && d->k >= 1 && d->groups >= 1 && (d->bigrams == 0 || d->bigrams == 1) &&
         (!d->bigrams || d->k <= VQVAE_CODES_MAX_BIGRAM_K) && (d->accumulate == 0 || d->accumulate == 1) && d->reserved == 0 &&
         d->total >= d->n;
}
static bool pair_desc_ok(const vqvae_codes_pair_desc* d) {
  return d && d->n >= 1 && d->max_short >= 1 && d->max_short <= VQVAE_CODES_MAX_SHORT && d->total_a >= d->n && d->total_b >= d->n;
}

// the one workspace plan of every entry point: nothing
static size_t plan_none() { WsPlan p; return p.total; }

}  // namespace vq

using namespace vq;

extern "C" int vqvae_codes_abi_version(void) { return 1; }

extern "C" size_t vqvae_codes_runs_workspace_bytes(const vqvae_codes_runs_desc* d) { return runs_desc_ok(d) ? plan_none() : (size_t)-1; }
extern "C" size_t vqvae_codes_hist_workspace_bytes(const vqvae_codes_hist_desc* d) { return hist_desc_ok(d) ? plan_none() : (size_t)-1; }
extern "C" size_t vqvae_codes_agree_workspace_bytes(const vqvae_codes_pair_desc* d) { return pair_desc_ok(d) ? plan_none() : (size_t)-1; }
extern "C" size_t vqvae_codes_edit_workspace_bytes(const vqvae_codes_pair_desc* d) { return pair_desc_ok(d) ? plan_none() : (size_t)-1; }

#define CS_REQUIRE_WS(who)                                                                                                 \
  VQ_REQUIRE(ws_bytes >= plan_none() && (ws || !plan_none()), who ": workspace of %zu bytes, %zu needed", ws_bytes, plan_none())

#define CS_REQUIRE_PAIRS(who, d, t)                                                                                        \
  VQ_REQUIRE(d, who ": null descriptor");                                                                                  \
  VQ_REQUIRE(d->n >= 1, who ": n must be at least 1 (got %d)", (int)d->n);                                                 \
  VQ_REQUIRE(d->max_short >= 1 && d->max_short <= VQVAE_CODES_MAX_SHORT, who ": max_short must be in [1, %d] (got %d)",    \
             VQVAE_CODES_MAX_SHORT, (int)d->max_short);                                                                    \
  VQ_REQUIRE(d->total_a >= d->n && d->total_b >= d->n, who ": total_a and total_b must be at least n (got %lld and %lld of %d)", \
             (long long)d->total_a, (long long)d->total_b, (int)d->n);                                                     \
  VQ_REQUIRE(t && t->start_a && t->len_a && t->start_b && t->len_b, who ": null tables")

extern "C" int vqvae_codes_runs(const vqvae_codes_runs_desc* d, const int32_t* codes, const int64_t* start, const int32_t* len,
                                int32_t* u, int32_t* dur, int32_t* m, int64_t* run_hist, void* ws, size_t ws_bytes,
                                vqvae_stream_t stream) {
  VQ_REQUIRE(d, "codes_runs: null descriptor");
  VQ_REQUIRE(d->n >= 1, "codes_runs: n must be at least 1 (got %d)", (int)d->n);
  VQ_REQUIRE(d->max_run >= 1, "codes_runs: max_run must be at least 1 (got %d)", (int)d->max_run);
  VQ_REQUIRE(d->total >= d->n, "codes_runs: total must be at least n (got %lld of %d)", (long long)d->total, (int)d->n);
  VQ_REQUIRE(codes && start && len && u && dur && m, "codes_runs: null codes, start, len, u, dur or m");
  CS_REQUIRE_WS("codes_runs");
  if (run_hist) VQ_CHECK_HIP(hipMemsetAsync(run_hist, 0, sizeof(int64_t) * (size_t)d->max_run, (hipStream_t)stream));
  RunsArgs a{};
  a.d = *d; a.codes = codes; a.start = start; a.len = len; a.u = u; a.dur = dur; a.m = m;
  a.run_hist = reinterpret_cast<unsigned long long*>(run_hist);
  hipLaunchKernelGGL(codes_runs_kernel, dim3((unsigned)d->n), dim3(CS_THREADS), 0, (hipStream_t)stream, a);
  VQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int vqvae_codes_hist(const vqvae_codes_hist_desc* d, const int32_t* codes, const int64_t* start, const int32_t* len,
                                const int32_t* group, int64_t* uni, int64_t* big, int64_t* invalid, void* ws, size_t ws_bytes,
                                vqvae_stream_t stream) {
  VQ_REQUIRE(d, "codes_hist: null descriptor");
  VQ_REQUIRE(d->n >= 1, "codes_hist: n must be at least 1 (got %d)", (int)d->n);
  VQ_REQUIRE(d->k >= 1 && d->groups >= 1, "codes_hist: k and groups must be at least 1 (got %d and %d)", (int)d->k, (int)d->groups);
  VQ_REQUIRE((d->bigrams == 0 || d->bigrams == 1) && (d->accumulate == 0 || d->accumulate == 1) && d->reserved == 0,
             "codes_hist: bigrams and accumulate must be 0 or 1 and reserved 0 (got %d, %d, %d)", (int)d->bigrams,
             (int)d->accumulate, (int)d->reserved);
  VQ_REQUIRE(!d->bigrams || d->k <= VQVAE_CODES_MAX_BIGRAM_K, "codes_hist: bigrams need k of at most %d (got %d)",
             VQVAE_CODES_MAX_BIGRAM_K, (int)d->k);
  VQ_REQUIRE(d->total >= d->n, "codes_hist: total must be at least n (got %lld of %d)", (long long)d->total, (int)d->n);
  VQ_REQUIRE(codes && start && len && group && uni && invalid, "codes_hist: null codes, start, len, group, uni or invalid");
  VQ_REQUIRE((big != nullptr) == (d->bigrams == 1), "codes_hist: big must be given with bigrams = 1 and null with bigrams = 0");
  CS_REQUIRE_WS("codes_hist");
  const hipStream_t s = (hipStream_t)stream;
  if (!d->accumulate) {
    VQ_CHECK_HIP(hipMemsetAsync(uni, 0, sizeof(int64_t) * (size_t)d->groups * (size_t)d->k, s));
    if (big) VQ_CHECK_HIP(hipMemsetAsync(big, 0, sizeof(int64_t) * (size_t)d->k * (size_t)d->k, s));
    VQ_CHECK_HIP(hipMemsetAsync(invalid, 0, sizeof(int64_t), s));
  }
  HistArgs a{};
  a.d = *d; a.codes = codes; a.start = start; a.len = len; a.group = group;
  a.uni = reinterpret_cast<unsigned long long*>(uni); a.big = reinterpret_cast<unsigned long long*>(big);
  a.invalid = reinterpret_cast<unsigned long long*>(invalid);
  hipLaunchKernelGGL(codes_hist_kernel, dim3((unsigned)d->n), dim3(CS_THREADS), 0, s, a);
  VQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int vqvae_codes_agree(const vqvae_codes_pair_desc* d, const vqvae_codes_pair_tables* t, const int32_t* a,
                                 const int32_t* b, int32_t* agree, void* ws, size_t ws_bytes, vqvae_stream_t stream) {
  CS_REQUIRE_PAIRS("codes_agree", d, t);
  VQ_REQUIRE(a && b && agree, "codes_agree: null a, b or agree");
  CS_REQUIRE_WS("codes_agree");
  PairArgs q{};
  q.d = *d; q.t = *t; q.a = a; q.b = b; q.out0 = agree;
  hipLaunchKernelGGL(codes_agree_kernel, dim3((unsigned)d->n), dim3(CS_THREADS), 0, (hipStream_t)stream, q);
  VQ_LAUNCH_CHECK();
  return 0;
}

extern "C" int vqvae_codes_edit(const vqvae_codes_pair_desc* d, const vqvae_codes_pair_tables* t, const int32_t* a,
                                const int32_t* b, int32_t* dist, int32_t* subs, void* ws, size_t ws_bytes,
                                vqvae_stream_t stream) {
  CS_REQUIRE_PAIRS("codes_edit", d, t);
  VQ_REQUIRE(a && b && dist && subs, "codes_edit: null a, b, dist or subs");
  CS_REQUIRE_WS("codes_edit");
  PairArgs q{};
  q.d = *d; q.t = *t; q.a = a; q.b = b; q.out0 = dist; q.out1 = subs;
  const size_t lds = CS_CELL_BYTES * (size_t)d->max_short;
  if (int e = lds_opt_in<codes_edit_kernel>(lds)) return e;
  hipLaunchKernelGGL(codes_edit_kernel, dim3((unsigned)d->n), dim3(CS_THREADS), lds, (hipStream_t)stream, q);
  VQ_LAUNCH_CHECK();
  return 0;
}
