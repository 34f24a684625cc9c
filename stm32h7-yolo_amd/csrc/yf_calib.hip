// libyf_calib.so (include/yf_calib.h): the float32 evaluation of the network over a batch of int8 frames on gfx950, with the running extremes
// of the 47 tensors calibration observes.  The arithmetic is csrc/yf_calib_arith.h's, compiled with -ffp-contract=off.
//
// One workgroup of 1024 threads per frame in flight, the frame's activations as float32 in LDS (the arena of yf_calib_arith.h, 156.8 KB of
// the CU's 160 KB: one workgroup per CU), a grid-stride loop over the frames.  A stage's output elements are dealt to the threads round
// robin; every thread keeps the extremes of what it computed, a wave folds them with shuffles, the waves' results meet in LDS, and the
// workgroup carries its running extremes in LDS across its frames.  Each workgroup leaves one partial table in global memory; a second,
// one-workgroup launch folds the partials into the handle's ranges.  Minimum and maximum are exact, so the result does not depend on which
// workgroup saw which frame, and nothing is ordered by arrival: no atomics.
//
// The comparing form (yf_calib_compare_device, csrc/yf_calib_compare.h) is the same evaluation without the extremes: where a stage produces a
// listed tensor every thread reads the int8 value of each element it computed and accumulates the error terms in the defined order (a thread
// is a lane, a wave a group); one record per frame and entry goes to global memory, and a second, one-workgroup launch adds the frames'
// records in ascending frame order.  The entries travel as a kernel argument: a launch refers to nothing a later call rewrites.
//
// The histogram form (yf_calib_histogram_device, csrc/yf_calib_hist.h) is the same evaluation with a bin where the observing form keeps an
// extreme.  A stage's tables (one uint32 count per bin and tensor) live in LDS, in the run of the arena that is dead during that stage
// (yfc_hist_windows: never less than 47 KB, enough for 4096 bins of every tensor a stage has); every lane adds its value's bin with one LDS
// atomic -- activations pile up around zero, and the LDS takes that contention better than a per-wave pre-count does (measured) --; after the
// stage the workgroup adds its non-empty bins to the caller's uint64 counts with vector atomics on consecutive addresses.  Integer sums are exact, so
// this is the one place where an atomic has no numerical meaning.  The axes and the windows travel as a kernel argument.
//
// The general forms (the _hw entries: frames of h x w, multiples of 8 up to 160) are the same bodies with the arena in another place.  Every
// form's loop over frames and stages exists once, as a __forceinline__ function (observe_frames, compare_frames, histogram_frames,
// simulate_frames, channel_sum_frames) of the arena pointer, the LDS scratch and the arena's sizes, and the form's two kernels only say
// where these are: the LDS kernel passes the dynamic LDS and the 56x56 sizes as constants, the slab kernel a slab of global memory -- 800 *
// (h / 8) * (w / 8) floats per workgroup in flight, owned by the handle (1.28 MB at 160x160, which no LDS holds) --, static LDS for the
// scratch and the sizes of `dims`.  So both have one workgroup per frame, a grid-stride loop over the frames and the round-robin deal of a
// stage's elements -- the deal is part of the comparing form's summation order.  The barrier that ends a stage is what hands the slab from
// the threads that wrote it to the threads that read it: the waves of a workgroup run on one CU and share its vector L1, and __syncthreads()
// orders global memory at workgroup scope (every wave's stores are waited for before the barrier); nothing here needs an agent-scope fence,
// because no other workgroup ever reads a slab during a launch.  In the slab kernels LDS holds the reduction scratch only, and in the
// histogram form the stage's tables at a fixed place (3 x 4096 x 4 B): there is no dead arena to borrow.  The LDS no longer limits a CU to
// one workgroup, so the grid comes from an occupancy query at yf_calib_create, not from the CU count alone (as compiled now the kernels'
// registers still allow one 16-wave workgroup per CU: profiles/calib160.txt).  Every size's stage table is uploaded once at creation (400
// sizes, 1 MB): a launch refers to nothing a later call rewrites.  The launches of one handle share its slabs, so each waits for the event
// recorded behind the one before it, whichever stream that went to.  On the host side each operation is one function too (observe, compare,
// ... below) behind its two entries, and `Evaluation` holds what all of them do around the launch.
//
// The simulating form (yf_calib_simulate_device and its _hw form, csrc/yf_calib_sim.h) is the same stage loop over yfc_stage_element_sim, which
// puts the tensors of the enabled entries on their int8 grids; the derived table travels as a kernel argument.  With reference logits every
// thread accumulates the head's error terms of the logits it copies out (a thread is a lane, a wave a group: compare_fold's order for one
// entry), and the frame's count of clipped values goes through a wave reduction and one LDS add per wave.  One body serves both kernels: the
// LDS form calls it with the 56x56 sizes as constants.
//
// The channel-summing form (yf_calib_channel_sums_device and its _hw form, csrc/yf_calib_chan.h) is the simulating form's stage loop with another
// deal of a stage's elements -- free here, because an element's stored bits do not depend on who computes it.  A task is one (channel, chunk
// of 64 consecutive pixels) pair and a wave takes whole tasks: its 64 lanes compute the chunk's pixels of that channel through the two parts
// of yfc_stage_element_sim, store the stage's result in the arena as always, and reduce the raw y = acc + bias in double with __shfl_down
// (wave_join's pattern: s[l] = s[l] + s[l + h]); lane 0 leaves the chunk's value in an LDS scratch [cout][chunks].  Behind the barrier that ends
// the stage thread c < cout adds its channel's chunks in ascending order and writes d_frame_sums[f][first + c].  The scratch alternates
// between two halves from one stage to the next, as `red` does in fold(): 2 x 18 x 13 doubles beside the arena at 56x56, 2 x 18 x 100 in the slab
// form.  Pool stages run as in the simulation.  A second launch, one thread per channel, adds the frames in ascending order.  Nothing is
// ordered by arrival: no atomics, and the result does not depend on the grid.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <new>
#include "../../include/yf_calib.h"
#include "yf_calib_arith.h"
#include "yf_calib_compare.h"
#include "yf_calib_hist.h"
#include "yf_calib_sim.h"
#include "yf_calib_chan.h"
#include "yf_yfw.h"

#ifndef YF_CALIB_BUILD_ID
#define YF_CALIB_BUILD_ID "unknown"
#endif

namespace {

constexpr int kThreads = 1024, kWaves = kThreads / 64, kPerStage = 6;                // a stage observes up to three tensors: 3 x {min, max}
constexpr int kRedFloats = 2 * kWaves * kPerStage, kWgFloats = 2 * YFC_N_RANGES;
constexpr size_t kLdsBytes = sizeof(float) * (YFC_ARENA_FLOATS + kRedFloats + kWgFloats);
constexpr int kParamFloats = YFC_INPUT_TABLE + YF_YFW_FLOATS;
static_assert(kLdsBytes <= 160 * 1024, "the arena and the reduction scratch must fit the CU's LDS");
static_assert(YFC_LOGITS_OFF + YFC_LOGITS <= YFC_ARENA_FLOATS, "logits inside the arena");
// the comparing form: three tensors x 16 waves x one record, double-buffered like `red`, beside the arena (and it would fit beside the
// extremes' scratch as well)
constexpr int kCmpRecords = 2 * 3 * kWaves;
constexpr size_t kCmpLdsBytes = sizeof(float) * YFC_ARENA_FLOATS + sizeof(yfc_cmp_frame) * kCmpRecords;
static_assert(kLdsBytes + sizeof(yfc_cmp_frame) * kCmpRecords <= 160 * 1024, "the arena and both reduction scratches must fit the CU's LDS");
static_assert(sizeof(float) * YFC_ARENA_FLOATS % alignof(yfc_cmp_frame) == 0 && kThreads == YFC_CMP_LANES && kWaves == YFC_CMP_GROUPS, "compare layout");
constexpr int kTotalsThreads = 320;
static_assert(kTotalsThreads >= YFC_CMP_MAX_ENTRIES * YFC_CMP_FIELDS, "one thread per entry and field");

__device__ inline float wave_min(float v) {
  for (int o = 32; o; o >>= 1) { const float t = __shfl_xor(v, o, 64); v = t < v ? t : v; }
  return v;
}
__device__ inline float wave_max(float v) {
  for (int o = 32; o; o >>= 1) { const float t = __shfl_xor(v, o, 64); v = t > v ? t : v; }
  return v;
}

// Folds the threads' extremes of one stage (mn / mx [3], slots[3] with -1 for none) into the workgroup's table.  `red` alternates between two
// halves from one call to the next: the threads that read a half after the barrier are past the NEXT barrier before anybody writes it again.
__device__ inline void fold(const float mn[3], const float mx[3], const int slots[3], float* red, float* wg, int& parity) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* half = red + parity * kWaves * kPerStage;
  for (int j = 0; j < 3; ++j) {
    if (slots[j] < 0) continue;                                                     // uniform
    const float a = wave_min(mn[j]), b = wave_max(mx[j]);
    if (lane == 0) { half[wave * kPerStage + 2 * j] = a; half[wave * kPerStage + 2 * j + 1] = b; }
  }
  __syncthreads();                                                                  // also: the stage's output is in the arena
  const int slot = tid < 2 ? slots[0] : tid < 4 ? slots[1] : slots[2];
  if (tid < kPerStage && slot >= 0) {
    float v = wg[2 * slot + (tid & 1)];
    for (int w = 0; w < kWaves; ++w) {
      const float t = half[w * kPerStage + tid];
      v = (tid & 1) ? (t > v ? t : v) : (t < v ? t : v);
    }
    wg[2 * slot + (tid & 1)] = v;
  }
  parity ^= 1;
}

// The observing form's body: `arena` is the LDS arena or this workgroup's slab; red (kRedFloats floats) and wg (kWgFloats floats) are LDS;
// frame_bytes, n_logits and logits_off describe the arena.
__device__ __forceinline__ void observe_frames(float* arena, float* red, float* wg, const int frame_bytes, const int n_logits, const int logits_off,
                                               const int8_t* __restrict__ frames, long n, const float* __restrict__ params,
                                               const yfc_stage* __restrict__ stages, float* __restrict__ logits, float* __restrict__ partials) {
  const int tid = threadIdx.x;
  const float inf = __builtin_inff();
  if (tid < kWgFloats) wg[tid] = (tid & 1) ? -inf : inf;
  __syncthreads();
  int parity = 0;
  for (long f = blockIdx.x; f < n; f += gridDim.x) {
    {
      const int8_t* q = frames + (size_t)f * (size_t)frame_bytes;
      float mn[3] = {inf, inf, inf}, mx[3] = {-inf, -inf, -inf};
      const int slots[3] = {0, -1, -1};
      for (int i = tid; i < frame_bytes; i += kThreads) {
        const float v = params[(int)q[i] + 128];
        arena[i] = v;
        mn[0] = v < mn[0] ? v : mn[0];
        mx[0] = v > mx[0] ? v : mx[0];
      }
      fold(mn, mx, slots, red, wg, parity);
    }
    for (int s = 0; s < YFC_N_STAGES; ++s) {
      const yfc_stage* g = &stages[s];
      const int count = g->oh * g->ow * g->cout;
      const int slots[3] = {g->r_conv, g->r_leaky, g->r_add};
      float mn[3] = {inf, inf, inf}, mx[3] = {-inf, -inf, -inf};
      for (int idx = tid; idx < count; idx += kThreads) {
        float v[3] = {0.0f, 0.0f, 0.0f};
        yfc_stage_element(g, arena, params, idx, v);
        for (int j = 0; j < 3; ++j) {
          if (slots[j] < 0) continue;
          mn[j] = v[j] < mn[j] ? v[j] : mn[j];
          mx[j] = v[j] > mx[j] ? v[j] : mx[j];
        }
      }
      fold(mn, mx, slots, red, wg, parity);                                           // (its barrier: the stage's output is in the arena)
    }
    // (the logits stay where they are until the next frame's third stage writes T54 over them, several barriers from here)
    if (logits)
      for (int i = tid; i < n_logits; i += kThreads) logits[(size_t)f * (size_t)n_logits + i] = arena[logits_off + i];
  }
  __syncthreads();
  if (tid < kWgFloats) partials[(size_t)blockIdx.x * kWgFloats + tid] = wg[tid];
}

__global__ __launch_bounds__(kThreads) void yfc_observe_kernel(const int8_t* __restrict__ frames, long n, const float* __restrict__ params,
                                                                const yfc_stage* __restrict__ stages, float* __restrict__ logits,
                                                                float* __restrict__ partials) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* red = lds + YFC_ARENA_FLOATS;
  observe_frames(lds, red, red + kRedFloats, YFC_FRAME_BYTES, YFC_LOGITS, YFC_LOGITS_OFF, frames, n, params, stages, logits, partials);
}

__global__ __launch_bounds__(kThreads) void yfc_observe_hw_kernel(const int8_t* __restrict__ frames, long n, const float* __restrict__ params,
                                                                   const yfc_stage* __restrict__ stages, const yfc_dims dims, float* slabs,
                                                                   float* __restrict__ logits, float* __restrict__ partials) {
  __shared__ float red[kRedFloats];
  __shared__ float wg[kWgFloats];
  float* arena = slabs + (size_t)blockIdx.x * (size_t)dims.arena_floats;
  observe_frames(arena, red, wg, dims.frame_bytes, dims.logits, dims.logits_off, frames, n, params, stages, logits, partials);
}

// ranges[t] = min / max (even / odd t) of ranges[t] and partials[0 .. parts)[t]
__global__ __launch_bounds__(128) void yfc_merge_kernel(const float* __restrict__ partials, int parts, float* __restrict__ ranges) {
  const int t = threadIdx.x;
  if (t >= kWgFloats) return;
  float v = ranges[t];
  for (int p = 0; p < parts; ++p) {
    const float x = partials[(size_t)p * kWgFloats + t];
    v = (t & 1) ? (x > v ? x : v) : (x < v ? x : v);
  }
  ranges[t] = v;
}

// s[l] = s[l] + s[l + h] for l < h, h = 32 .. 1: lane 0 ends with the group's value (the other lanes' values are not used)
__device__ inline void wave_join(yfc_cmp_frame& a) {
  for (int h = 32; h; h >>= 1) {
    yfc_cmp_frame b;
    b.sum_err = __shfl_down(a.sum_err, h, 64);
    b.sum_sq_err = __shfl_down(a.sum_sq_err, h, 64);
    b.sum_sq_ref = __shfl_down(a.sum_sq_ref, h, 64);
    b.max_abs_err = __shfl_down(a.max_abs_err, h, 64);
    b.saturated = __shfl_down(a.saturated, h, 64);
    yfc_cmp_join(&a, &b);
  }
}

// The threads' accumulators of one stage (acc[3], entries[3] with -1 for none) -> the frame's records row[entry]: the 16 wave values meet in
// LDS and one thread per tensor adds them in wave order.  `red` alternates between two halves as in fold().
__device__ inline void compare_fold(const yfc_cmp_frame acc[3], const int entries[3], yfc_cmp_frame* red, yfc_cmp_frame* row, int& parity) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  yfc_cmp_frame* half = red + parity * 3 * kWaves;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    if (entries[j] < 0) continue;                                                   // uniform
    yfc_cmp_frame a = acc[j];
    wave_join(a);
    if (lane == 0) half[j * kWaves + wave] = a;
  }
  __syncthreads();                                                                  // also: the stage's output is in the arena
  const int entry = tid == 0 ? entries[0] : tid == 1 ? entries[1] : entries[2];
  if (tid < 3 && entry >= 0) {
    yfc_cmp_frame a = half[tid * kWaves];
    for (int w = 1; w < kWaves; ++w) yfc_cmp_join(&a, &half[tid * kWaves + w]);
    row[entry] = a;
  }
  parity ^= 1;
}

// ... and the comparing form's.  red: kCmpRecords records (LDS)
__device__ __forceinline__ void compare_frames(float* arena, yfc_cmp_frame* red, const int frame_bytes, const int8_t* __restrict__ frames, long n,
                                               const float* __restrict__ params, const yfc_stage* __restrict__ stages, const yfc_cmp_plan& plan,
                                               yfc_cmp_frame* __restrict__ frame_stats) {
  const int tid = threadIdx.x;
  int parity = 0;
  for (long f = blockIdx.x; f < n; f += gridDim.x) {
    const int8_t* q = frames + (size_t)f * (size_t)frame_bytes;
    for (int i = tid; i < frame_bytes; i += kThreads) arena[i] = params[(int)q[i] + 128];
    __syncthreads();
    for (int s = 0; s < YFC_N_STAGES; ++s) {
      const yfc_stage* g = &stages[s];
      const int count = g->oh * g->ow * g->cout;
      const int entries[3] = {plan.entry[s][0], plan.entry[s][1], plan.entry[s][2]};
      const int8_t* qt[3] = {nullptr, nullptr, nullptr};
      float scale[3] = {0.0f, 0.0f, 0.0f};
      int zp[3] = {0, 0, 0};
      yfc_cmp_frame acc[3];                                                         // (per frame and stage: every frame starts from +0)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        yfc_cmp_zero(&acc[j]);
        if (entries[j] < 0) continue;
        qt[j] = plan.q[entries[j]] + (size_t)f * plan.frame_stride[entries[j]];
        scale[j] = plan.scale[entries[j]];
        zp[j] = plan.zero_point[entries[j]];
      }
      for (int idx = tid; idx < count; idx += kThreads) {
        float v[3] = {0.0f, 0.0f, 0.0f};
        yfc_stage_element(g, arena, params, idx, v);
#pragma unroll
        for (int j = 0; j < 3; ++j)
          if (entries[j] >= 0) yfc_cmp_add(&acc[j], qt[j][idx], zp[j], scale[j], v[j]);
      }
      compare_fold(acc, entries, red, frame_stats + (size_t)f * plan.count, parity);
    }
  }
}

__global__ __launch_bounds__(kThreads) void yfc_compare_kernel(const int8_t* __restrict__ frames, long n, const float* __restrict__ params,
                                                                const yfc_stage* __restrict__ stages, const yfc_cmp_plan plan,
                                                                yfc_cmp_frame* __restrict__ frame_stats) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  compare_frames(lds, reinterpret_cast<yfc_cmp_frame*>(lds + YFC_ARENA_FLOATS), YFC_FRAME_BYTES, frames, n, params, stages, plan, frame_stats);
}

__global__ __launch_bounds__(kThreads) void yfc_compare_hw_kernel(const int8_t* __restrict__ frames, long n, const float* __restrict__ params,
                                                                   const yfc_stage* __restrict__ stages, const yfc_dims dims, float* slabs,
                                                                   const yfc_cmp_plan plan, yfc_cmp_frame* __restrict__ frame_stats) {
  __shared__ yfc_cmp_frame red[kCmpRecords];
  float* arena = slabs + (size_t)blockIdx.x * (size_t)dims.arena_floats;
  compare_frames(arena, red, dims.frame_bytes, frames, n, params, stages, plan, frame_stats);
}

// totals[entry] = the frames' records added in ascending frame order: one thread per entry and field
__global__ __launch_bounds__(kTotalsThreads) void yfc_totals_kernel(const yfc_cmp_frame* __restrict__ frame_stats, long n, const yfc_cmp_plan plan,
                                                                     yfc_cmp_total* __restrict__ totals) {
  const int entry = threadIdx.x / YFC_CMP_FIELDS, field = threadIdx.x % YFC_CMP_FIELDS;
  if (entry < plan.count) yfc_cmp_total_field(frame_stats, n, plan.count, entry, plan.elements[entry], field, &totals[entry]);
}

// ---- the histogram form ----
constexpr size_t kHistLdsBytes = sizeof(float) * YFC_ARENA_FLOATS;
// Bins a wave adds as one atomic each (the lanes that share a bin counted with a ballot) before its lanes go one by one.  0: every lane adds
// for itself, which is what ships -- the LDS absorbs 64 adds to one address better than the wave can pre-count them: measured at 1, 4 and 8
// bins, every one slower (profiles/calib_histogram.txt (b); tools/calib_histogram_bench.py --variant-lib times such builds).
#ifndef YFC_HIST_PEEL
#define YFC_HIST_PEEL 0
#endif
constexpr int kHistPeel = YFC_HIST_PEEL;

struct yfc_hist_plan {
  yfc_hist_axes axes;
  int32_t off[YFC_N_STAGES + 1];                                                      // arena floats: the tables of the input's step and of every stage
  int32_t bins;
};

// table[bin] += 1 for every calling lane.  With kHistPeel > 0 the lanes that share the first pending lane's bin are counted with a ballot and
// added by one of them, kHistPeel times over; what is left adds for itself.  Any split gives the same sums.
__device__ inline void hist_add(uint32_t* table, int bin) {
  bool todo = true;
  for (int k = 0; k < kHistPeel; ++k) {
    if (todo) {
      const int first = __builtin_amdgcn_readfirstlane(bin);
      const bool same = bin == first;
      const unsigned long long m = __ballot(same);
      if (same) {
        if ((int)(threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(&table[first], (uint32_t)__popcll(m));
        todo = false;
      }
    }
  }
  if (todo) atomicAdd(&table[bin], 1u);
}

__device__ inline void hist_clear(uint32_t* table, int entries) {
  for (int i = threadIdx.x; i < entries; i += kThreads) table[i] = 0;
  __syncthreads();
}

// The stage's tables (tables x bins, all threads past their adds) -> counts[slot][bin]; a barrier on either side
__device__ inline void hist_flush(const uint32_t* table, const int slots[3], int bins, unsigned long long* __restrict__ counts) {
  __syncthreads();                                                                  // also: the stage's output is in the arena
  int at = 0;
  for (int j = 0; j < 3; ++j) {
    if (slots[j] < 0) continue;                                                     // uniform
    unsigned long long* row = counts + (size_t)slots[j] * bins;
    for (int i = threadIdx.x; i < bins; i += kThreads) {
      const uint32_t k = table[at * bins + i];
      if (k) atomicAdd(&row[i], (unsigned long long)k);
    }
    ++at;
  }
  __syncthreads();                                                                  // the next step may write where the tables were
}

// ... and the histogram form's.  tables: the LDS the steps' tables are placed in, uint32 counts; off: where each step's tables start in it (the input's step, then every
// stage), or nullptr for "at `tables`, every step" -- a constant at the call, so that the choice is made when the body is inlined.  The tables
// are reached as `tables` plus an offset, never through a pointer kept per tensor: the adds stay LDS instructions.
__device__ __forceinline__ void histogram_frames(float* arena, uint32_t* tables, const int32_t* off, const int frame_bytes,
                                                 const int8_t* __restrict__ frames, long n, const float* __restrict__ params,
                                                 const yfc_stage* __restrict__ stages, const yfc_hist_axes& axes, const int bins,
                                                 unsigned long long* __restrict__ counts) {
  const int tid = threadIdx.x;
  for (long f = blockIdx.x; f < n; f += gridDim.x) {
    {
      const int8_t* q = frames + (size_t)f * (size_t)frame_bytes;
      uint32_t* table = off ? tables + off[0] : tables;
      const int slots[3] = {0, -1, -1};
      const float lo = axes.lo[0], inv = axes.inv[0];
      hist_clear(table, bins);
      for (int i = tid; i < frame_bytes; i += kThreads) {
        const float v = params[(int)q[i] + 128];
        arena[i] = v;
        hist_add(table, yfc_hist_bin(v, lo, inv, bins));
      }
      hist_flush(table, slots, bins, counts);
    }
    for (int s = 0; s < YFC_N_STAGES; ++s) {
      const yfc_stage* g = &stages[s];
      const int count = g->oh * g->ow * g->cout;
      const int slots[3] = {g->r_conv, g->r_leaky, g->r_add};
      uint32_t* table = off ? tables + off[s + 1] : tables;
      int tab[3] = {0, 0, 0};
      float lo[3] = {0.0f, 0.0f, 0.0f}, inv[3] = {0.0f, 0.0f, 0.0f};
      int n_tables = 0;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        if (slots[j] < 0) continue;
        tab[j] = n_tables * bins;
        lo[j] = axes.lo[slots[j]];
        inv[j] = axes.inv[slots[j]];
        ++n_tables;
      }
      hist_clear(table, n_tables * bins);
      for (int idx = tid; idx < count; idx += kThreads) {
        float v[3] = {0.0f, 0.0f, 0.0f};
        yfc_stage_element(g, arena, params, idx, v);
#pragma unroll
        for (int j = 0; j < 3; ++j)
          if (slots[j] >= 0) hist_add(table, tab[j] + yfc_hist_bin(v[j], lo[j], inv[j], bins));
      }
      hist_flush(table, slots, bins, counts);                                         // (its first barrier: the stage's output is in the arena)
    }
  }
}

// the tables in the run of the arena that is dead during the step (plan.off, in arena floats: a count is as wide as a float)
__global__ __launch_bounds__(kThreads) void yfc_histogram_kernel(const int8_t* __restrict__ frames, long n, const float* __restrict__ params,
                                                                  const yfc_stage* __restrict__ stages, const yfc_hist_plan plan,
                                                                  unsigned long long* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  histogram_frames(lds, reinterpret_cast<uint32_t*>(lds), plan.off, YFC_FRAME_BYTES, frames, n, params, stages, plan.axes, plan.bins, counts);
}

struct yfc_hist_hw_plan {                                                             // (the LDS form's plan without the offsets)
  yfc_hist_axes axes;
  int32_t bins;
  yfc_hist_hw_plan(const yfc_hist_plan& p) : axes(p.axes), bins(p.bins) {}
};

// the tables at a fixed place: a slab leaves no dead arena to borrow
__global__ __launch_bounds__(kThreads) void yfc_histogram_hw_kernel(const int8_t* __restrict__ frames, long n, const float* __restrict__ params,
                                                                     const yfc_stage* __restrict__ stages, const yfc_dims dims, float* slabs,
                                                                     const yfc_hist_hw_plan plan, unsigned long long* __restrict__ counts) {
  __shared__ uint32_t table[3 * YFC_HIST_MAX_BINS];                                   // a stage has up to three tensors
  float* arena = slabs + (size_t)blockIdx.x * (size_t)dims.arena_floats;
  histogram_frames(arena, table, nullptr, dims.frame_bytes, frames, n, params, stages, plan.axes, plan.bins, counts);
}

// ---- the simulating form: one body, the arena in LDS (the 56x56 sizes as constants) or in this workgroup's slab ----
constexpr int kSimRecords = kWaves;
constexpr size_t kSimLdsBytes = sizeof(float) * YFC_ARENA_FLOATS + sizeof(yfc_cmp_frame) * kSimRecords + sizeof(int32_t) * 2;
static_assert(kSimLdsBytes <= kCmpLdsBytes && kSimLdsBytes <= 160 * 1024, "the arena, the head's reduction scratch and the clip count must fit the CU's LDS");

__device__ inline int wave_sum(int v) {
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// red: kSimRecords records; clip: one count (both LDS).  frame_bytes, n_logits and logits_off describe the arena.
__device__ __forceinline__ void simulate_frames(float* arena, yfc_cmp_frame* red, int32_t* clip, const int frame_bytes, const int n_logits,
                                                const int logits_off, const int8_t* __restrict__ frames, long n, const float* __restrict__ params,
                                                const yfc_stage* __restrict__ stages, const yfc_sim_plan& plan, const float* __restrict__ ref,
                                                float* __restrict__ logits, yfc_cmp_frame* __restrict__ frame_stats) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (long f = blockIdx.x; f < n; f += gridDim.x) {
    const int8_t* q = frames + (size_t)f * (size_t)frame_bytes;
    int32_t clipped = 0;
    for (int i = tid; i < frame_bytes; i += kThreads) arena[i] = yfc_sim_input(&plan, params[(int)q[i] + 128], &clipped);
    if (tid == 0) *clip = 0;                                                          // (read last behind the barrier that ended the frame before)
    __syncthreads();
    for (int s = 0; s < YFC_N_STAGES; ++s) {
      const yfc_stage* g = &stages[s];
      const int count = g->oh * g->ow * g->cout;
      for (int idx = tid; idx < count; idx += kThreads) yfc_stage_element_sim(g, s, arena, params, idx, &plan, &clipped);
      __syncthreads();                                                                // the stage's output is in the arena
    }
    // (the logits stay where they are until the next frame's second stage writes T54 over them, two barriers from here)
    yfc_cmp_frame acc;
    yfc_cmp_zero(&acc);
    for (int i = tid; i < n_logits; i += kThreads) {
      const float y = arena[logits_off + i];
      if (logits) logits[(size_t)f * (size_t)n_logits + i] = y;
      if (ref) yfc_sim_cmp_add(&acc, y, ref[(size_t)f * (size_t)n_logits + i]);
    }
    if (ref) {                                                                        // uniform
      wave_join(acc);
      const int k = wave_sum(clipped);
      if (lane == 0) { red[wave] = acc; atomicAdd(clip, k); }
      __syncthreads();
      if (tid == 0) {
        yfc_cmp_frame a = red[0];
        for (int w = 1; w < kWaves; ++w) yfc_cmp_join(&a, &red[w]);
        a.saturated = *clip;
        frame_stats[f] = a;
      }
      // (red and clip are written again only behind the next frame's barriers)
    }
  }
}

__global__ __launch_bounds__(kThreads) void yfc_simulate_kernel(const int8_t* __restrict__ frames, long n, const float* __restrict__ params,
                                                                 const yfc_stage* __restrict__ stages, const yfc_sim_plan plan,
                                                                 const float* __restrict__ ref, float* __restrict__ logits,
                                                                 yfc_cmp_frame* __restrict__ frame_stats) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  yfc_cmp_frame* red = reinterpret_cast<yfc_cmp_frame*>(lds + YFC_ARENA_FLOATS);
  int32_t* clip = reinterpret_cast<int32_t*>(red + kSimRecords);
  simulate_frames(lds, red, clip, YFC_FRAME_BYTES, YFC_LOGITS, YFC_LOGITS_OFF, frames, n, params, stages, plan, ref, logits, frame_stats);
}

__global__ __launch_bounds__(kThreads) void yfc_simulate_hw_kernel(const int8_t* __restrict__ frames, long n, const float* __restrict__ params,
                                                                    const yfc_stage* __restrict__ stages, const yfc_dims dims, float* slabs,
                                                                    const yfc_sim_plan plan, const float* __restrict__ ref,
                                                                    float* __restrict__ logits, yfc_cmp_frame* __restrict__ frame_stats) {
  __shared__ yfc_cmp_frame red[kSimRecords];
  __shared__ int32_t clip;
  float* arena = slabs + (size_t)blockIdx.x * (size_t)dims.arena_floats;
  simulate_frames(arena, red, &clip, dims.frame_bytes, dims.logits, dims.logits_off, frames, n, params, stages, plan, ref, logits, frame_stats);
}

// ---- the channel-summing form: one body, the arena in LDS (the 56x56 sizes as constants) or in this workgroup's slab ----
constexpr size_t kChanLdsBytes = sizeof(float) * YFC_ARENA_FLOATS + sizeof(double) * 2 * YFC_CHAN_SCRATCH_56;
static_assert(sizeof(double) * 2 * YFC_CHAN_SCRATCH_56 == 3744 && kChanLdsBytes <= 160 * 1024,
              "the arena and both halves of the chunk scratch (18 channels x 13 chunks of doubles each) must fit the CU's LDS");
static_assert(sizeof(float) * YFC_ARENA_FLOATS % alignof(double) == 0, "the chunk scratch behind the arena is aligned");
static_assert(YFC_CHAN_SCRATCH_MAX == 18 * (((YFC_MAX_SIDE / 2) * (YFC_MAX_SIDE / 2) + YFC_CHAN_CHUNK - 1) / YFC_CHAN_CHUNK) && YFC_CHAN_CHUNK == 64,
              "the slab form's scratch is the 18-channel stage at the largest size; a chunk is a wave");
constexpr int kChanTotalsThreads = 256;

// scratch: two halves of half_doubles doubles (LDS).  frame_bytes, n_logits and logits_off describe the arena.
__device__ __forceinline__ void channel_sum_frames(float* arena, double* scratch, const int half_doubles, const int frame_bytes, const int n_logits,
                                                   const int logits_off, const int8_t* __restrict__ frames, long n, const float* __restrict__ params,
                                                   const yfc_stage* __restrict__ stages, const yfc_chan_plan& plan, double* __restrict__ frame_sums,
                                                   float* __restrict__ logits) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);                          // (uniform: a task's channel and chunk are scalars)
  int parity = 0;
  for (long f = blockIdx.x; f < n; f += gridDim.x) {
    const int8_t* q = frames + (size_t)f * (size_t)frame_bytes;
    int32_t clipped = 0;                                                              // (counted by the element function; not reported here)
    for (int i = tid; i < frame_bytes; i += kThreads) arena[i] = yfc_sim_input(&plan.sim, params[(int)q[i] + 128], &clipped);
    __syncthreads();
    for (int s = 0; s < YFC_N_STAGES; ++s) {
      const yfc_stage* g = &stages[s];
      const int pixels = g->oh * g->ow, cout = g->cout;
      if (g->kind != YFC_CONV) {                                                      // uniform: a pool, as the simulation runs it
        for (int idx = tid; idx < pixels * cout; idx += kThreads) yfc_stage_element_sim(g, s, arena, params, idx, &plan.sim, &clipped);
        __syncthreads();
        continue;
      }
      const int chunks = yfc_chan_chunks(pixels);
      double* half = scratch + parity * half_doubles;
      for (int task = wave; task < cout * chunks; task += kWaves) {
        const int co = task / chunks, chunk = task - co * chunks;
        const int px = chunk * YFC_CHAN_CHUNK + lane;
        double v = 0.0;
        if (px < pixels) {
          const int idx = px * cout + co;
          const float y = yfc_stage_element_sim_raw(g, arena, params, idx);
          yfc_stage_element_sim_finish(g, s, arena, idx, y, &plan.sim, &clipped);
          v = (double)y;
        }
        for (int h = 32; h; h >>= 1) v = v + __shfl_down(v, h, 64);                   // lane 0 ends with the chunk's value
        if (lane == 0) half[co * chunks + chunk] = v;
      }
      __syncthreads();                                                                // the stage's output is in the arena, its chunks in `half`
      if (tid < cout) {
        double a = half[tid * chunks];
        for (int k = 1; k < chunks; ++k) a = a + half[tid * chunks + k];
        frame_sums[(size_t)f * YFC_CHANNELS + plan.first[s] + tid] = a;
      }
      parity ^= 1;                                                                    // (this half is written again two stages, and so two barriers, on)
    }
    // (the logits stay where they are until the next frame's second stage writes T54 over them, two barriers from here)
    if (logits)
      for (int i = tid; i < n_logits; i += kThreads) logits[(size_t)f * (size_t)n_logits + i] = arena[logits_off + i];
  }
}

__global__ __launch_bounds__(kThreads) void yfc_channel_sums_kernel(const int8_t* __restrict__ frames, long n, const float* __restrict__ params,
                                                                     const yfc_stage* __restrict__ stages, const yfc_chan_plan plan,
                                                                     double* __restrict__ frame_sums, float* __restrict__ logits) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  double* scratch = reinterpret_cast<double*>(lds + YFC_ARENA_FLOATS);
  channel_sum_frames(lds, scratch, YFC_CHAN_SCRATCH_56, YFC_FRAME_BYTES, YFC_LOGITS, YFC_LOGITS_OFF, frames, n, params, stages, plan, frame_sums, logits);
}

__global__ __launch_bounds__(kThreads) void yfc_channel_sums_hw_kernel(const int8_t* __restrict__ frames, long n, const float* __restrict__ params,
                                                                        const yfc_stage* __restrict__ stages, const yfc_dims dims, float* slabs,
                                                                        const yfc_chan_plan plan, double* __restrict__ frame_sums,
                                                                        float* __restrict__ logits) {
  __shared__ double scratch[2 * YFC_CHAN_SCRATCH_MAX];
  float* arena = slabs + (size_t)blockIdx.x * (size_t)dims.arena_floats;
  channel_sum_frames(arena, scratch, YFC_CHAN_SCRATCH_MAX, dims.frame_bytes, dims.logits, dims.logits_off, frames, n, params, stages, plan, frame_sums,
                     logits);
}

// sums[c] = the frames' rows added in ascending frame order: one thread per channel
__global__ __launch_bounds__(kChanTotalsThreads) void yfc_channel_totals_kernel(const double* __restrict__ frame_sums, long n, double* __restrict__ sums) {
  const int c = blockIdx.x * kChanTotalsThreads + threadIdx.x;
  if (c < YFC_CHANNELS) sums[c] = yfc_chan_total(frame_sums, n, c);
}

thread_local char g_err[320];

#define set_error(...) snprintf(g_err, sizeof g_err, __VA_ARGS__)

bool hip_ok(hipError_t e, const char* what) {
  if (e == hipSuccess) return true;
  set_error("%s: %s", what, hipGetErrorString(e));
  return false;
}

// the caller's current device is restored when a call ends
struct DeviceScope {
  int prev = -1;
  bool ok = false;
  explicit DeviceScope(int device) {
    if (!hip_ok(hipGetDevice(&prev), "hipGetDevice")) { prev = -1; return; }
    ok = prev == device || hip_ok(hipSetDevice(device), "hipSetDevice");
    if (!ok || prev == device) prev = -1;
  }
  ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
};

}  // namespace

struct yf_calib {
  int device = 0, grid_max = 0;
  long frames = 0;
  float* d_params = nullptr;
  yfc_stage* d_stages = nullptr;
  float* d_partials = nullptr;
  float* d_ranges = nullptr;
  int32_t tensors[YFC_N_RANGES];
  yfc_stage stages[YFC_N_STAGES];
  int32_t hist_off[YFC_N_STAGES + 1];                      // where each step's histogram tables live in the arena (yfc_hist_windows)
  // the general forms
  int hw_grid = 0;                                         // workgroups of a general launch = slabs: CUs x resident workgroups per CU
  yfc_stage* d_stages_hw = nullptr;                        // [YFC_N_SIDES][YFC_N_SIDES][YFC_N_STAGES]: the table of every admitted size
  float* d_slabs = nullptr;
  size_t slab_bytes = 0;
  hipEvent_t slabs_free = nullptr;                         // recorded behind the last general launch
  bool slabs_used = false;
};

// The windows of the histogram kernel's tables; every one must hold YFC_HIST_MAX_BINS bins of each tensor its step has.
static bool place_histogram_tables(yf_calib* c) {
  int8_t* writer = new (std::nothrow) int8_t[YFC_ARENA_FLOATS];
  uint32_t* busy = new (std::nothrow) uint32_t[YFC_ARENA_FLOATS];
  int32_t floats[YFC_N_STAGES + 1];
  bool ok = writer && busy;
  if (!ok) set_error("yf_calib_create: out of memory");
  if (ok) yfc_hist_windows(c->stages, c->hist_off, floats, writer, busy);
  for (int step = 0; step <= YFC_N_STAGES && ok; ++step) {
    const yfc_stage* g = step ? &c->stages[step - 1] : nullptr;
    const int tables = g ? (g->r_conv >= 0) + (g->r_leaky >= 0) + (g->r_add >= 0) : 1;
    ok = c->hist_off[step] >= 0 && floats[step] >= tables * YFC_HIST_MAX_BINS && c->hist_off[step] + floats[step] <= YFC_ARENA_FLOATS;
    if (!ok) set_error("yf_calib_create: step %d leaves %d dead arena floats at %d, its %d histogram tables need %d", step, (int)floats[step],
                       (int)c->hist_off[step], tables, tables * YFC_HIST_MAX_BINS);
  }
  delete[] writer;
  delete[] busy;
  return ok;
}

// The evaluation kernels, a row per form.  The LDS kernels: the dynamic LDS yf_calib_create allows each, and what it says if it cannot ...
static const struct { const void* kernel; size_t lds_bytes; const char* what; } kLdsKernels[] = {
    {(const void*)yfc_observe_kernel, kLdsBytes, "hipFuncSetAttribute(max dynamic LDS)"},
    {(const void*)yfc_compare_kernel, kCmpLdsBytes, "hipFuncSetAttribute(max dynamic LDS, compare)"},
    {(const void*)yfc_histogram_kernel, kHistLdsBytes, "hipFuncSetAttribute(max dynamic LDS, histogram)"},
    {(const void*)yfc_simulate_kernel, kSimLdsBytes, "hipFuncSetAttribute(max dynamic LDS, simulate)"},
    {(const void*)yfc_channel_sums_kernel, kChanLdsBytes, "hipFuncSetAttribute(max dynamic LDS, channel sums)"}};
// ... and the slab kernels, for general_setup's occupancy query
static const void* const kSlabKernels[] = {(const void*)yfc_observe_hw_kernel, (const void*)yfc_compare_hw_kernel, (const void*)yfc_histogram_hw_kernel,
                                           (const void*)yfc_simulate_hw_kernel, (const void*)yfc_channel_sums_hw_kernel};
constexpr int kForms = sizeof kSlabKernels / sizeof kSlabKernels[0];
static_assert(sizeof kLdsKernels / sizeof kLdsKernels[0] == kForms, "every form has an LDS and a slab kernel");

// The general forms' share of yf_calib_create (the device is current): the grid from an occupancy query, every size's stage table, the event.
static bool general_setup(yf_calib* c, int cus) {
  int per_cu = 0;
  for (int k = 0; k < kForms; ++k) {                       // one slab count for all: the fewest resident workgroups any of them has
    int blocks = 0;
    if (!hip_ok(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, kSlabKernels[k], kThreads, 0), "hipOccupancyMaxActiveBlocksPerMultiprocessor"))
      return false;
    if (blocks < 1) { set_error("yf_calib_create: general kernel %d: the occupancy query gives %d resident workgroups", k, blocks); return false; }
    per_cu = k == 0 || blocks < per_cu ? blocks : per_cu;
  }
  c->hw_grid = cus * per_cu;
  const size_t tables = (size_t)YFC_N_SIDES * YFC_N_SIDES;
  yfc_stage* all = new (std::nothrow) yfc_stage[tables * YFC_N_STAGES];
  if (!all) { set_error("yf_calib_create: out of memory"); return false; }
  int32_t ids[YFC_N_RANGES];
  for (int i = 0; i < YFC_N_SIDES; ++i)
    for (int j = 0; j < YFC_N_SIDES; ++j)
      yfc_build_stages_hw(all + ((size_t)i * YFC_N_SIDES + j) * YFC_N_STAGES, ids, (i + 1) * YFC_SIDE_STEP, (j + 1) * YFC_SIDE_STEP);
  const size_t bytes = sizeof(yfc_stage) * tables * YFC_N_STAGES;
  const bool ok = hip_ok(hipMalloc((void**)&c->d_stages_hw, bytes), "hipMalloc(stage tables)")
               && hip_ok(hipMemcpy(c->d_stages_hw, all, bytes, hipMemcpyHostToDevice), "hipMemcpy(stage tables)")
               && hip_ok(hipEventCreateWithFlags(&c->slabs_free, hipEventDisableTiming), "hipEventCreateWithFlags");
  delete[] all;
  return ok;
}

static bool upload_empty_ranges(yf_calib* c) {
  float init[kWgFloats];
  for (int t = 0; t < kWgFloats; ++t) init[t] = (t & 1) ? -INFINITY : INFINITY;
  return hip_ok(hipMemcpy(c->d_ranges, init, sizeof init, hipMemcpyHostToDevice), "hipMemcpy(ranges)");
}

// the one check of a frame size, for every _hw entry: true and the text when it is refused
static bool size_refused(const char* name, int h, int w) {
  if (yfc_size_ok(h, w)) return false;
  set_error("%s: the frame size is h = %d, w = %d, expected " YFC_SIZE_RULE " each", name, h, w);
  return true;
}

// What a general call does before it launches, at an admitted size: the stage table, slabs enough for it, and the launch before it out of
// the way.  0, or a negative value with the text set and nothing launched.
static int general_begin(yf_calib* c, const yfc_dims& dims, hipStream_t s, const yfc_stage** d_stages) {
  *d_stages = c->d_stages_hw + ((size_t)(dims.h / YFC_SIDE_STEP - 1) * YFC_N_SIDES + (size_t)(dims.w / YFC_SIDE_STEP - 1)) * YFC_N_STAGES;
  const size_t need = (size_t)c->hw_grid * (size_t)dims.arena_floats * sizeof(float);
  if (need > c->slab_bytes) {                              // the one place where a general call synchronises and allocates
    if (!hip_ok(hipDeviceSynchronize(), "hipDeviceSynchronize (growing the scratch)")) return -2;
    (void)hipFree(c->d_slabs);
    c->d_slabs = nullptr;
    c->slab_bytes = 0;
    if (!hip_ok(hipMalloc((void**)&c->d_slabs, need), "hipMalloc(scratch slabs)")) return -2;
    c->slab_bytes = need;
    c->slabs_used = false;                                 // (the device is idle: nothing to wait for)
  }
  // (unconditional: behind a launch on the same stream the wait is already satisfied, and a stream handle's value says nothing -- a
  // destroyed stream's successor may carry it)
  if (c->slabs_used && !hip_ok(hipStreamWaitEvent(s, c->slabs_free, 0), "hipStreamWaitEvent(slabs)")) return -2;
  return 0;
}

// ... and after it: the event the next general launch waits for
static bool general_end(yf_calib* c, hipStream_t s) {
  if (!hip_ok(hipEventRecord(c->slabs_free, s), "hipEventRecord(slabs)")) return false;
  c->slabs_used = true;
  return true;
}

// What the ten evaluating entries share around their launch.  Made: the handle's device is current until the entry returns, the grid is one
// workgroup per frame up to grid_max (the LDS kernels, hw false: the size is 56x56) or hw_grid (the slab kernels, at an admitted h x w), and
// for the slab kernels the size's stage table is chosen and the stream waits for the slabs; rc is then 0, or what the entry returns.
// launch(): the evaluation and its check.  launched(): the check of any later launch.  record(): the slab kernels' event; the LDS kernels
// touch neither the event nor the slabs.
struct Evaluation {
  const char* name;
  yf_calib* c;
  bool hw;
  DeviceScope scope;
  hipStream_t s;
  int grid;
  yfc_dims dims;
  const yfc_stage* d_stages;
  long rc = 0;

  Evaluation(const char* name, yf_calib* c, bool hw, int h, int w, long n, void* stream)
      : name(name), c(c), hw(hw), scope(c->device), s((hipStream_t)stream), grid((int)(n < (hw ? c->hw_grid : c->grid_max) ? n : hw ? c->hw_grid : c->grid_max)),
        d_stages(c->d_stages) {
    yfc_dims_of(h, w, &dims);
    if (!scope.ok) rc = -1;
    else if (hw) rc = general_begin(c, dims, s, &d_stages);
  }
  // args: what follows `stages` in the LDS kernel's parameters and `slabs` in the slab kernel's
  template <class Lds, class Slab, class... Args>
  bool launch(Lds lds_kernel, size_t lds_bytes, Slab slab_kernel, const void* d_frames, long n, Args... args) {
    if (hw) hipLaunchKernelGGL(slab_kernel, dim3(grid), dim3(kThreads), 0, s, (const int8_t*)d_frames, n, (const float*)c->d_params, d_stages, dims, c->d_slabs, args...);
    else hipLaunchKernelGGL(lds_kernel, dim3(grid), dim3(kThreads), lds_bytes, s, (const int8_t*)d_frames, n, (const float*)c->d_params, d_stages, args...);
    return launched("evaluation");
  }
  bool launched(const char* what) {
    char text[96];
    snprintf(text, sizeof text, "%s: launch of the %s", name, what);
    return hip_ok(hipGetLastError(), text);
  }
  bool record() { return !hw || general_end(c, s); }
};

// totals[entry] of the frames' records, behind the evaluation on its stream
static bool launch_totals(Evaluation& e, const void* d_frame_stats, long n, const yfc_cmp_plan& plan, void* d_totals) {
  hipLaunchKernelGGL(yfc_totals_kernel, dim3(1), dim3(kTotalsThreads), 0, e.s, (const yfc_cmp_frame*)d_frame_stats, n, plan, (yfc_cmp_total*)d_totals);
  return e.launched("totals");
}

static bool launch_channel_totals(Evaluation& e, const double* d_frame_sums, long n, double* d_sums) {
  hipLaunchKernelGGL(yfc_channel_totals_kernel, dim3((YFC_CHANNELS + kChanTotalsThreads - 1) / kChanTotalsThreads), dim3(kChanTotalsThreads), 0, e.s,
                     d_frame_sums, n, d_sums);
  return e.launched("totals");
}

// the totals of a simulate call are those of a comparison with one entry: the head
static yfc_cmp_plan head_totals_plan(int logits) {
  yfc_cmp_plan plan;
  memset(&plan, 0, sizeof plan);
  plan.count = 1;
  plan.elements[0] = logits;
  return plan;
}

// ---- the five operations, each once: `name` is the entry's own, for its texts; hw: the _hw entry, at h x w (else 56x56) ----
static long observe(const char* name, yf_calib* c, bool hw, int h, int w, const void* d_frames, long n, void* d_logits, void* stream) {
  g_err[0] = 0;
  if (!c || !d_frames) { set_error("%s: NULL %s", name, c ? "d_frames" : "handle"); return -1; }
  if (n < 1) { set_error("%s: n is %ld, expected at least 1", name, n); return -1; }
  if (hw && size_refused(name, h, w)) return -1;
  Evaluation e(name, c, hw, h, w, n, stream);
  if (e.rc) return e.rc;
  if (!e.launch(yfc_observe_kernel, kLdsBytes, yfc_observe_hw_kernel, d_frames, n, (float*)d_logits, c->d_partials)) return -2;
  hipLaunchKernelGGL(yfc_merge_kernel, dim3(1), dim3(128), 0, e.s, (const float*)c->d_partials, e.grid, c->d_ranges);
  if (!e.launched("merge") || !e.record()) return -2;        // (the merge reads the handle's partials: the event comes behind it)
  c->frames += n;
  return n;
}

static long compare(const char* name, yf_calib* c, bool hw, int h, int w, const void* d_frames, long n, const yf_calib_qtensor* entries, int count,
                    void* d_frame_stats, void* d_totals, void* stream) {
  g_err[0] = 0;
  if (!c) { set_error("%s: NULL handle", name); return -1; }
  if (hw && size_refused(name, h, w)) return -1;
  yfc_stage stages[YFC_N_STAGES];
  int32_t ids[YFC_N_RANGES];
  if (hw) yfc_build_stages_hw(stages, ids, h, w);
  yfc_cmp_plan plan;
  if (yfc_cmp_validate(hw ? stages : c->stages, entries, count, n, &plan, g_err, sizeof g_err)) return -1;
  if (!d_frames || !d_frame_stats) { set_error("%s: NULL %s", name, d_frames ? "d_frame_stats" : "d_frames"); return -1; }
  Evaluation e(name, c, hw, h, w, n, stream);
  if (e.rc) return e.rc;
  if (!e.launch(yfc_compare_kernel, kCmpLdsBytes, yfc_compare_hw_kernel, d_frames, n, plan, (yfc_cmp_frame*)d_frame_stats) || !e.record()) return -2;
  if (d_totals && !launch_totals(e, d_frame_stats, n, plan, d_totals)) return -2;
  return n;
}

static long histogram(const char* name, yf_calib* c, bool hw, int h, int w, const void* d_frames, long n, const float* minmax, int bins,
                      uint64_t* d_counts, void* stream) {
  g_err[0] = 0;
  if (!c) { set_error("%s: NULL handle", name); return -1; }
  if (hw && size_refused(name, h, w)) return -1;
  yfc_hist_plan plan;                                      // (the slab kernel takes it without the offsets)
  if (yfc_hist_validate(d_frames, n, minmax, bins, d_counts, &plan.axes, g_err, sizeof g_err)) return -1;
  if ((uintptr_t)d_counts % sizeof(uint64_t)) { set_error("histogram: counts is at %p, expected an address aligned to 8 bytes", (void*)d_counts); return -1; }
  memcpy(plan.off, c->hist_off, sizeof plan.off);
  plan.bins = bins;
  Evaluation e(name, c, hw, h, w, n, stream);
  if (e.rc) return e.rc;
  if (!e.launch(yfc_histogram_kernel, kHistLdsBytes, yfc_histogram_hw_kernel, d_frames, n, plan, (unsigned long long*)d_counts) || !e.record()) return -2;
  return n;
}

static long simulate(const char* name, yf_calib* c, bool hw, int h, int w, const void* d_frames, long n, const yf_calib_sim_entry* table,
                     const void* d_ref_logits, void* d_logits, void* d_frame_stats, void* d_totals, void* stream) {
  g_err[0] = 0;
  if (!c) { set_error("%s: NULL handle", name); return -1; }
  if (hw && size_refused(name, h, w)) return -1;
  yfc_sim_plan plan;
  if (yfc_sim_validate(name, c->stages, d_frames, n, table, d_ref_logits, d_frame_stats, d_totals, &plan, g_err, sizeof g_err)) return -1;
  Evaluation e(name, c, hw, h, w, n, stream);
  if (e.rc) return e.rc;
  if (!e.launch(yfc_simulate_kernel, kSimLdsBytes, yfc_simulate_hw_kernel, d_frames, n, plan, (const float*)d_ref_logits, (float*)d_logits,
                (yfc_cmp_frame*)d_frame_stats) || !e.record())
    return -2;
  if (d_totals && !launch_totals(e, d_frame_stats, n, head_totals_plan(e.dims.logits), d_totals)) return -2;
  return n;
}

static long channel_sums(const char* name, yf_calib* c, bool hw, int h, int w, const void* d_frames, long n, const yf_calib_sim_entry* table,
                         double* d_frame_sums, double* d_sums, void* d_logits, void* stream) {
  g_err[0] = 0;
  if (!c) { set_error("%s: NULL handle", name); return -1; }
  if (hw && size_refused(name, h, w)) return -1;
  yfc_stage stages[YFC_N_STAGES];
  int32_t ids[YFC_N_RANGES];
  if (hw) yfc_build_stages_hw(stages, ids, h, w);
  yfc_chan_plan plan;
  if (yfc_chan_validate(name, hw ? stages : c->stages, d_frames, n, table, d_frame_sums, &plan, g_err, sizeof g_err)) return -1;
  if (hw && yfc_chan_scratch_doubles(stages) > YFC_CHAN_SCRATCH_MAX) {      // (the 56x56 scratch was checked at yf_calib_create)
    set_error("%s: h = %d, w = %d needs a chunk scratch of %d doubles, the kernel has %d", name, h, w, yfc_chan_scratch_doubles(stages),
              (int)YFC_CHAN_SCRATCH_MAX);
    return -1;
  }
  Evaluation e(name, c, hw, h, w, n, stream);
  if (e.rc) return e.rc;
  if (!e.launch(yfc_channel_sums_kernel, kChanLdsBytes, yfc_channel_sums_hw_kernel, d_frames, n, plan, d_frame_sums, (float*)d_logits) || !e.record())
    return -2;
  if (d_sums && !launch_channel_totals(e, d_frame_sums, n, d_sums)) return -2;
  return n;
}

extern "C" {

YF_CALIB_API const char* yf_calib_last_error_text(void) { return g_err; }
YF_CALIB_API const char* yf_calib_build_id(void) { return YF_CALIB_BUILD_ID; }

YF_CALIB_API void yf_calib_destroy(yf_calib* c) {
  if (!c) return;
  {
    DeviceScope scope(c->device);
    if (scope.ok) (void)hipDeviceSynchronize();
    (void)hipFree(c->d_params); (void)hipFree(c->d_stages); (void)hipFree(c->d_partials); (void)hipFree(c->d_ranges);
    (void)hipFree(c->d_stages_hw); (void)hipFree(c->d_slabs);
    if (c->slabs_free) (void)hipEventDestroy(c->slabs_free);
  }
  delete c;
}

YF_CALIB_API yf_calib* yf_calib_create(const void* yfw, size_t bytes, int device) {
  g_err[0] = 0;
  float* p = new (std::nothrow) float[kParamFloats];
  if (!p) { set_error("yf_calib_create: out of memory"); return nullptr; }
  yfc_input_table(p);
  if (yf_yfw_parse(yfw, bytes, p + YFC_INPUT_TABLE, g_err, sizeof g_err)) { delete[] p; return nullptr; }
  yf_calib* c = new (std::nothrow) yf_calib;
  if (!c) { delete[] p; set_error("yf_calib_create: out of memory"); return nullptr; }
  c->device = device;
  yfc_stage (&stages)[YFC_N_STAGES] = c->stages;
  yfc_build_stages(stages, c->tensors);
  const yfc_stage& last = stages[YFC_N_STAGES - 1];
  bool ok = last.b_off + last.cout == kParamFloats && last.out_off == YFC_LOGITS_OFF;
  if (!ok) set_error("yf_calib_create: the stage table gives %d parameter floats, the graph %d", last.b_off + last.cout, kParamFloats);
  ok = ok && place_histogram_tables(c);
  if (ok) {
    int32_t first[YFC_N_CONVS], cout[YFC_N_CONVS], pixels[YFC_N_CONVS];
    const int channels = yfc_chan_layout(stages, first, cout, pixels), scratch = yfc_chan_scratch_doubles(stages);
    ok = channels == YFC_CHANNELS && scratch == YFC_CHAN_SCRATCH_56;
    if (!ok) set_error("yf_calib_create: the stage table gives %d channels and a chunk scratch of %d doubles, expected %d of the graph and %d", channels,
                       scratch, (int)YFC_CHANNELS, (int)YFC_CHAN_SCRATCH_56);
  }
  if (ok) {
    DeviceScope scope(device);
    int cus = 0;
    ok = scope.ok && hip_ok(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device), "hipDeviceGetAttribute(multiprocessors)");
    if (ok && cus < 1) { ok = false; set_error("yf_calib_create: device %d reports %d compute units", device, cus); }
    c->grid_max = cus;                                     // 156.8 KB of LDS: one workgroup per CU
    for (int k = 0; k < kForms && ok; ++k)
      ok = hip_ok(hipFuncSetAttribute(kLdsKernels[k].kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsKernels[k].lds_bytes), kLdsKernels[k].what);
    ok = ok && hip_ok(hipMalloc((void**)&c->d_params, sizeof(float) * kParamFloats), "hipMalloc(params)")
         && hip_ok(hipMalloc((void**)&c->d_stages, sizeof stages), "hipMalloc(stages)")
         && general_setup(c, cus)
         && hip_ok(hipMalloc((void**)&c->d_partials, sizeof(float) * kWgFloats * (size_t)(c->hw_grid > cus ? c->hw_grid : cus)), "hipMalloc(partials)")
         && hip_ok(hipMalloc((void**)&c->d_ranges, sizeof(float) * kWgFloats), "hipMalloc(ranges)")
         && hip_ok(hipMemcpy(c->d_params, p, sizeof(float) * kParamFloats, hipMemcpyHostToDevice), "hipMemcpy(params)")
         && hip_ok(hipMemcpy(c->d_stages, stages, sizeof stages, hipMemcpyHostToDevice), "hipMemcpy(stages)")
         && upload_empty_ranges(c) && hip_ok(hipDeviceSynchronize(), "hipDeviceSynchronize");
  }
  delete[] p;
  if (!ok) {
    char keep[sizeof g_err];
    memcpy(keep, g_err, sizeof keep);
    yf_calib_destroy(c);
    memcpy(g_err, keep, sizeof keep);
    return nullptr;
  }
  return c;
}

YF_CALIB_API long yf_calib_observe_device(yf_calib* c, const void* d_frames, long n, void* d_logits, void* stream) {
  return observe("yf_calib_observe_device", c, false, 56, 56, d_frames, n, d_logits, stream);
}
YF_CALIB_API long yf_calib_observe_hw_device(yf_calib* c, int h, int w, const void* d_frames, long n, void* d_logits, void* stream) {
  return observe("yf_calib_observe_hw_device", c, true, h, w, d_frames, n, d_logits, stream);
}

YF_CALIB_API long yf_calib_compare_device(yf_calib* c, const void* d_frames, long n, const yf_calib_qtensor* entries, int count,
                                          void* d_frame_stats, void* d_totals, void* stream) {
  return compare("yf_calib_compare_device", c, false, 56, 56, d_frames, n, entries, count, d_frame_stats, d_totals, stream);
}
YF_CALIB_API long yf_calib_compare_hw_device(yf_calib* c, int h, int w, const void* d_frames, long n, const yf_calib_qtensor* entries, int count,
                                             void* d_frame_stats, void* d_totals, void* stream) {
  return compare("yf_calib_compare_hw_device", c, true, h, w, d_frames, n, entries, count, d_frame_stats, d_totals, stream);
}

YF_CALIB_API long yf_calib_histogram_device(yf_calib* c, const void* d_frames, long n, const float* minmax, int bins, uint64_t* d_counts,
                                            void* stream) {
  return histogram("yf_calib_histogram_device", c, false, 56, 56, d_frames, n, minmax, bins, d_counts, stream);
}
YF_CALIB_API long yf_calib_histogram_hw_device(yf_calib* c, int h, int w, const void* d_frames, long n, const float* minmax, int bins,
                                               uint64_t* d_counts, void* stream) {
  return histogram("yf_calib_histogram_hw_device", c, true, h, w, d_frames, n, minmax, bins, d_counts, stream);
}

YF_CALIB_API long yf_calib_simulate_device(yf_calib* c, const void* d_frames, long n, const yf_calib_sim_entry* table, const void* d_ref_logits,
                                           void* d_logits, void* d_frame_stats, void* d_totals, void* stream) {
  return simulate("yf_calib_simulate_device", c, false, 56, 56, d_frames, n, table, d_ref_logits, d_logits, d_frame_stats, d_totals, stream);
}
YF_CALIB_API long yf_calib_simulate_hw_device(yf_calib* c, int h, int w, const void* d_frames, long n, const yf_calib_sim_entry* table,
                                              const void* d_ref_logits, void* d_logits, void* d_frame_stats, void* d_totals, void* stream) {
  return simulate("yf_calib_simulate_hw_device", c, true, h, w, d_frames, n, table, d_ref_logits, d_logits, d_frame_stats, d_totals, stream);
}

YF_CALIB_API long yf_calib_channel_sums_device(yf_calib* c, const void* d_frames, long n, const yf_calib_sim_entry* table, double* d_frame_sums,
                                               double* d_sums, void* d_logits, void* stream) {
  return channel_sums("yf_calib_channel_sums_device", c, false, 56, 56, d_frames, n, table, d_frame_sums, d_sums, d_logits, stream);
}
YF_CALIB_API long yf_calib_channel_sums_hw_device(yf_calib* c, int h, int w, const void* d_frames, long n, const yf_calib_sim_entry* table,
                                                  double* d_frame_sums, double* d_sums, void* d_logits, void* stream) {
  return channel_sums("yf_calib_channel_sums_hw_device", c, true, h, w, d_frames, n, table, d_frame_sums, d_sums, d_logits, stream);
}

YF_CALIB_API int yf_calib_channel_layout(int32_t first[YF_CALIB_N_CONVS], int32_t cout[YF_CALIB_N_CONVS], int32_t pixels56[YF_CALIB_N_CONVS]) {
  yfc_stage stages[YFC_N_STAGES];
  int32_t ids[YFC_N_RANGES];
  if (!first || !cout || !pixels56) return -1;
  yfc_build_stages(stages, ids);
  return yfc_chan_layout(stages, first, cout, pixels56);
}

YF_CALIB_API int yf_calib_workgroups(const yf_calib* c, int h, int w) {
  g_err[0] = 0;
  if (!c) { set_error("yf_calib_workgroups: NULL handle"); return -1; }
  if (size_refused("yf_calib_workgroups", h, w)) return -1;
  return c->hw_grid;
}

YF_CALIB_API size_t yf_calib_scratch_bytes(const yf_calib* c) { return c ? c->slab_bytes : 0; }

YF_CALIB_API int yf_calib_ranges(yf_calib* c, float* minmax, int32_t* tensors) {
  g_err[0] = 0;
  if (!c || !minmax || !tensors) { set_error("yf_calib_ranges: NULL argument"); return -1; }
  if (c->frames < 1) { set_error("yf_calib_ranges: no frame has been observed yet: there are no ranges"); return -1; }
  DeviceScope scope(c->device);
  if (!scope.ok) return -2;
  if (!hip_ok(hipDeviceSynchronize(), "yf_calib_ranges: hipDeviceSynchronize") ||
      !hip_ok(hipMemcpy(minmax, c->d_ranges, sizeof(float) * kWgFloats, hipMemcpyDeviceToHost), "yf_calib_ranges: hipMemcpy"))
    return -2;
  for (int t = 0; t < kWgFloats; ++t) minmax[t] = minmax[t] + 0.0f;                 // (a zero comes out as +0 whichever sign was met first)
  memcpy(tensors, c->tensors, sizeof c->tensors);
  return YFC_N_RANGES;
}

YF_CALIB_API int yf_calib_reset(yf_calib* c) {
  g_err[0] = 0;
  if (!c) { set_error("yf_calib_reset: NULL handle"); return -1; }
  DeviceScope scope(c->device);
  if (!scope.ok) return -2;
  if (!hip_ok(hipDeviceSynchronize(), "yf_calib_reset: hipDeviceSynchronize") || !upload_empty_ranges(c) ||
      !hip_ok(hipDeviceSynchronize(), "yf_calib_reset: hipDeviceSynchronize"))
    return -2;
  c->frames = 0;
  return 0;
}

YF_CALIB_API long yf_calib_frames_observed(const yf_calib* c) { return c ? c->frames : -1; }

}  // extern "C"
