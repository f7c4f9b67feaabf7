// Lockstep generation with refill (include/vqvae_gen_slots.h): the columns of generate_lockstep.hip's step as slots
// of a table in device memory.  A slot whose sequence has finished takes the next one from a queue, so sequences of
// different lengths keep all columns busy; a step costs one weight stream whatever the number of live columns.
//
// The arithmetic is gen_lockstep_body.h's, instantiated with the slot policy: what belongs to a sequence is addressed
// by (slot_seq[column], slot_t[column]), what belongs to the machine by the column, and d->step is a tick that only
// indexes the rings.  Nothing is cleared when a slot changes hands:
//   * ring-age predicate: a ring entry read at tick % dilation was pushed `dilation` ticks ago, by the present tenant
//     only if slot_t >= dilation; younger tenants read 0, the fresh queue of modules.py:58-67.  (One slot's rings are
//     6.3 MB for the default decoder; zero-filling them would cost more than the step.)
//   * the finish launch of a sequence's last step writes zeros to the slot's x_cur and x_prev (the 2-sample embed queue).
// The last launch of a tick is the scheduler: one wavefront, each lane owns slots lane and lane + 64, free slots are
// counted with a ballot and take queue[next + rank] in slot order.  No atomics: one wave reads the table, every lane
// writes its own two slots, lane 0 writes next / live / the tick, so the assignment is a pure function of the inputs.
#include "gen_lockstep_body.h"
#include "gen_step.h"

namespace vq {

__global__ __launch_bounds__(LS_THREADS) void gen_slots_gemm_kernel(LsGemmArgs a, LsSlots p) { ls_gemm_body(a, p); }

__global__ __launch_bounds__(256) void gen_slots_finish_kernel(LsFinishArgs a, LsSlots p) { ls_finish_body(a, p); }

__global__ __launch_bounds__(SMP_THREADS) void gen_slots_sampled_finish_kernel(SampledArgs a, LsSlots p) { smp_finish_body(a, p); }

struct SlotSchedArgs {
  const int* steps; const int* queue;
  int* next; int* slot_seq; int* slot_t; int* live; int* started; int* tick;
  int n_slots, n_queue, max_steps;
};

// Fills the table from the head of the queue and zeroes the tick.
__global__ __launch_bounds__(64) void gen_slots_init_kernel(SlotSchedArgs a) {
  const int lane = threadIdx.x;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int slot = lane + 64 * h;
    if (slot >= a.n_slots) continue;
    int seq = -1;
    if (slot < a.n_queue) {
      seq = a.queue[slot];
      if (a.started) { a.started[2 * seq] = slot; a.started[2 * seq + 1] = 0; }
    }
    a.slot_seq[slot] = seq;
    a.slot_t[slot] = 0;
  }
  if (lane == 0) {
    const int taken = a.n_queue < a.n_slots ? a.n_queue : a.n_slots;
    *a.next = taken;
    *a.live = taken;
    *a.tick = 0;
  }
}

// The end of a tick.  Everything is read before anything is written (one wave, program order).
__global__ __launch_bounds__(64) void gen_slots_schedule_kernel(SlotSchedArgs a) {
  const int tick = *a.tick, live = *a.live, nx = *a.next;
  if (tick >= a.max_steps || live == 0) return;
  const int lane = threadIdx.x;
  const unsigned long long below = (1ull << lane) - 1ull;
  int seq[2], st[2];
  bool freed[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int slot = lane + 64 * h;
    seq[h] = slot < a.n_slots ? a.slot_seq[slot] : -1;
    st[h] = 0;
    freed[h] = false;
    if (seq[h] >= 0) {
      st[h] = a.slot_t[slot] + 1;
      freed[h] = st[h] >= a.steps[seq[h]];
    }
  }
  const unsigned long long f0 = __ballot(freed[0]), f1 = __ballot(freed[1]);
  const int n0 = __popcll(f0), n_free = n0 + __popcll(f1);
  const int waiting = a.n_queue - nx;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int slot = lane + 64 * h;
    if (seq[h] < 0) continue;                       // idle slots stay idle: the queue is exhausted by then
    if (freed[h]) {
      const int rank = (h ? n0 : 0) + __popcll((h ? f1 : f0) & below);
      int s = -1;
      if (rank < waiting) {
        s = a.queue[nx + rank];
        if (a.started) { a.started[2 * s] = slot; a.started[2 * s + 1] = tick + 1; }
      }
      a.slot_seq[slot] = s;
      a.slot_t[slot] = 0;
    } else {
      a.slot_t[slot] = st[h];
    }
  }
  if (lane == 0) {
    const int taken = n_free < waiting ? n_free : waiting;
    *a.next = nx + taken;
    *a.live = live - (n_free - taken);
    *a.tick = tick + 1;
  }
}

static int slots_validate(const vqvae_gen_desc* d, const vqvae_gen_slots* s, const char* who) {
  VQ_REQUIRE(d && s, "%s: null descriptor or slot table", who);
  VQ_REQUIRE(d->n > VQVAE_GEN_MAX_N && d->n <= VQVAE_GEN_MAX_LOCKSTEP, "%s: d->n must be %d..%d slots (got %d)", who,
             VQVAE_GEN_MAX_N + 1, VQVAE_GEN_MAX_LOCKSTEP, d->n);
  VQ_REQUIRE(d->step, "%s: null tick (d->step)", who);
  VQ_REQUIRE(s->steps && s->queue && s->next && s->slot_seq && s->slot_t && s->live, "%s: null slot table member", who);
  VQ_REQUIRE(s->n_seq >= 0 && s->n_queue >= 0 && s->n_queue <= s->n_seq, "%s: n_queue must be 0..n_seq (got %d of %d)", who,
             s->n_queue, s->n_seq);
  return 0;
}

static SlotSchedArgs sched_args(const vqvae_gen_desc* d, const vqvae_gen_slots* s) {
  SlotSchedArgs a{};
  a.steps = s->steps; a.queue = s->queue; a.next = s->next; a.slot_seq = s->slot_seq; a.slot_t = s->slot_t;
  a.live = s->live; a.started = s->started; a.tick = d->step;
  a.n_slots = d->n; a.n_queue = s->n_queue; a.max_steps = d->max_steps;
  return a;
}

}  // namespace vq

using namespace vq;

extern "C" int vqvae_gen_slots_abi_version(void) { return 1; }

extern "C" int vqvae_gen_slots_init(const vqvae_gen_desc* d, const vqvae_gen_slots* slots, vqvae_stream_t stream) {
  const int bad = slots_validate(d, slots, "gen_slots_init");
  if (bad != 0) return bad;
  hipLaunchKernelGGL(gen_slots_init_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, sched_args(d, slots));
  VQ_LAUNCH_CHECK();
  return 0;
}

// One tick.  finish == nullptr: the finishing kernels above read the descriptor's array of uniforms; else `finish`
// launches the finishing kernel (gen_rng.hip: the uniforms drawn on the device; d->uniforms may then be null).
namespace vq {
int gen_step_slots_impl(const vqvae_gen_desc* d, const vqvae_gen_slots* slots, const vqvae_gen_sampling* s, const char* who,
                        SlotsFinish finish, const void* ctx, hipStream_t st) {
  int bad = slots_validate(d, slots, who);
  if (bad != 0) return bad;
  if ((bad = finish ? gen_validate_desc_rng(d) : gen_validate_desc(d)) != 0) return bad;
  const bool controls = gen_controls_set(s);
  VQ_REQUIRE(d->sample_mode != VQVAE_GEN_NONE || d->logits_out, "%s: sample_mode VQVAE_GEN_NONE needs logits_out", who);
  VQ_REQUIRE(!controls || d->sample_mode != VQVAE_GEN_NONE,
             "%s: sampling controls need sample_mode VQVAE_GEN_SOFTMAX or VQVAE_GEN_MOL", who);
  VQ_REQUIRE(!controls || d->sample_mode != VQVAE_GEN_MOL || (!s->top_k && !s->top_p),
             "%s: the mixture of logistics takes a temperature only (top_k and top_p must be NULL)", who);
  VQ_REQUIRE(d->sample_mode != VQVAE_GEN_SOFTMAX || d->out_dim <= LS_MAXOUT, "%s: at most %d classes", who, LS_MAXOUT);
  if ((bad = gen_validate_blocks(d, who)) != 0) return bad;
  LsSlots p{};
  p.slot_seq = slots->slot_seq; p.slot_t = slots->slot_t; p.live_count = slots->live; p.steps = slots->steps;
  p.x_prev = d->x_prev; p.nseq = slots->n_seq;
  const int rc = ls_step_products(d, [&](const LsGemmArgs& g, hipStream_t q) {
    hipLaunchKernelGGL(gen_slots_gemm_kernel, ls_gemm_grid(g), dim3(LS_THREADS), 0, q, g, p);
    VQ_LAUNCH_CHECK();
    return 0;
  }, st);
  if (rc != 0) return rc;
  if (finish) {
    if ((bad = finish(d, controls ? s : nullptr, p, ctx, st)) != 0) return bad;
  } else {
    if (controls) {
      hipLaunchKernelGGL(gen_slots_sampled_finish_kernel, dim3(d->n), dim3(SMP_THREADS), 0, st, smp_finish_args(d, s), p);
    } else {
      hipLaunchKernelGGL(gen_slots_finish_kernel, dim3(d->n), dim3(256), 0, st, ls_finish_args(d), p);
    }
    VQ_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(gen_slots_schedule_kernel, dim3(1), dim3(64), 0, st, sched_args(d, slots));
  VQ_LAUNCH_CHECK();
  return 0;
}
}  // namespace vq

extern "C" int vqvae_wavenet_gen_step_slots(const vqvae_gen_desc* d, const vqvae_gen_slots* slots,
                                            const vqvae_gen_sampling* s, vqvae_stream_t stream) {
  return gen_step_slots_impl(d, slots, s, "gen_step_slots", nullptr, nullptr, (hipStream_t)stream);
}
