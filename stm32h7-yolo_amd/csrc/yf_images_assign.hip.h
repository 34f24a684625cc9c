// The kernel of the tracker with a motion model and optimal assignment (yf_images_track_motion_assign_device with YF_ASSIGN_OPTIMAL);
// the definition is csrc/yf_images_assign.h.  Included by yf_images.hip.
//
// The plan is yfmotion::step_kernel's (yf_images_motion.hip.h, which is not touched: its kernel keeps its instructions): one wave per
// stream, lane = slot, a slot's 28 words in its lane's registers over the stream's steps; predict, update and emit are that kernel's code,
// restated here.  New is the match:
//   weights   the m x 64 table once per step, by the scan of the greedy's first round -- detection i's edges and area broadcast, lane j
//             computes its IoU --, kept as int32 in 16 KB of LDS, row i contiguous: lane j reads and writes word i * 64 + j, one word per
//             bank and lane, free of bank conflicts.  A step without an eligible pair skips the search.
//   search    lane-parallel by column: v, minv, way, used and the assigned row p of column j live in lane j; u and "visited" of row r in
//             lane r.  i0 and j0 are wave-uniform (scalar registers); u[i0] and p[j0] are read with readlane.  0 <= minv <= 2^31 + 2
//             (the header's bound) for every column relaxed, and every unused column is relaxed before the minimum is taken, so the
//             minimum is a 32-bit unsigned butterfly with used columns at 0xFFFFFFFF -- at most 63 columns are used, so one candidate is
//             always left --, and the lowest lane attaining it is the lowest bit of a ballot.
//   result    lane j's detection is p if w[p][j] > 0, read back from the table (p is a row this search assigned: 0 <= p < m).
// Every branch is wave-uniform; the lanes differ only in selects, so every cross-lane read runs with all 64 lanes active.  Nothing is
// indexed by a value read from the state.  The LDS is the wave's own (one-wave workgroups) and lane j reads only the words it wrote
// itself (column j of every row): no barrier is needed.
#pragma once
#include "yf_images_assign.h"

namespace yfassign {

constexpr int kSlotWords = YFI_MOTION_SLOT_WORDS, kStateWords = YFI_MOTION_STATE_WORDS;
static_assert(YF_TRACK_SLOTS == 64 && YF_TRACK_MAX_DETS == 64, "one lane per slot and per detection");

struct AssignArgs {
  const yf_det* dets;
  const int* counts;
  long streams, steps;
  int layout, cap;
  double match_iou;
  int min_hits, max_misses;
  int alpha, beta, damp, smooth;
  uint32_t* state;
  yf_det* out;
  yf_track_info* info;
  int* out_counts;
  int out_cap;
  int* status;
};

__device__ __forceinline__ int bcast(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }

__device__ __forceinline__ double bcast(double v, int lane) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}

__device__ __forceinline__ int64_t bcast(int64_t v, int lane) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), lane);
  return (int64_t)((uint64_t)hi << 32 | lo);
}

// the search of yf_images_assign.h on the table w (row i at w + 64 i) -> this lane's (column's) detection, -1 for none
__device__ __forceinline__ int solve(const int32_t* w, int m, int lane) {
  int64_t u = 0, v = 0;
  int p = -1;
  for (int i = 0; i < m; ++i) {
    int64_t minv = YFI_ASSIGN_INF;
    int way = -1;
    bool used = false, visited = lane == i;
    int i0 = i, j0 = -1;
    for (;;) {
      const int64_t cur = (YFI_ASSIGN_TOP - (int64_t)w[i0 * 64 + lane]) - bcast(u, i0) - v;
      if (!used && cur < minv) { minv = cur; way = j0; }
      uint32_t low = used ? 0xFFFFFFFFu : (uint32_t)minv;          // an unused column has been relaxed: minv <= 2^31 + 2
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t other = __shfl_xor(low, d);
        low = other < low ? other : low;
      }
      low = (uint32_t)__builtin_amdgcn_readfirstlane((int)low);    // every lane holds the minimum: say so
      const int j1 = __builtin_ctzll(__ballot(!used && (uint32_t)minv == low));      // the lowest column attaining it
      const int64_t delta = (int64_t)low;
      u += visited ? delta : 0;
      v -= used ? delta : 0;
      minv -= used ? 0 : delta;
      j0 = j1;
      const int pj = bcast(p, j0);
      if (pj < 0) break;
      used = used || lane == j0;
      i0 = pj;
      visited = visited || lane == i0;
    }
    while (j0 >= 0) {
      const int j1 = bcast(way, j0);
      const int np = j1 >= 0 ? bcast(p, j1 & 63) : i;
      if (lane == j0) p = np;
      j0 = j1;
    }
  }
  const int row = p >= 0 ? p : 0;
  return p >= 0 && w[row * 64 + lane] > 0 ? p : -1;
}

__global__ void __launch_bounds__(64) step_kernel(AssignArgs a) {
  __shared__ int32_t weights[YF_TRACK_MAX_DETS * YF_TRACK_SLOTS];  // 16 KB: [detection][slot]
  const int lane = threadIdx.x;
  const uint64_t below = (1ull << lane) - 1ull;
  for (long s = blockIdx.x; s < a.streams; s += gridDim.x) {
    uint32_t* st = a.state + (size_t)s * kStateWords;
    uint32_t issued = st[0];
    uint32_t* mine = st + 2 + lane * kSlotWords;                   // 8 + 112 * lane bytes into an 8-byte aligned state
    int64_t* mine64 = (int64_t*)(mine + 12);
    uint32_t id = mine[0];
    int hits = (int)mine[1], misses = (int)mine[2], age = (int)mine[3];
    int tw[7];
#pragma unroll
    for (int q = 0; q < 7; ++q) tw[q] = (int)mine[4 + q];
    uint32_t pad = mine[11];
    int64_t pos[4], vel[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int64_t p = mine64[e], v = mine64[4 + e];
      pos[e] = id != 0 ? yfi_motion_sat(p) : p;
      vel[e] = id != 0 ? yfi_motion_sat(v) : v;
    }

    for (long t = 0; t < a.steps; ++t) {
      const long f = a.layout == YF_TRACK_TIME_MAJOR ? t * a.streams + s : s * a.steps + t;
      const int c = a.counts[f];
      const int m = __builtin_amdgcn_readfirstlane(yfi_track_clamp(c, a.cap));
      int bits = yfi_track_clipped(c, a.cap) ? YFI_TRACK_ST_CLIPPED : 0;
      const int* in = (const int*)(a.dets + (size_t)f * a.cap);
      int dw[7] = {0, 0, 0, 0, 0, 0, 0};
      if (lane < m) {
#pragma unroll
        for (int q = 0; q < 7; ++q) dw[q] = in[lane * 7 + q];
      }
      const double darea = yfi_nms_area(dw[3], dw[4], dw[5], dw[6]);

      // ---- predict ----
      const bool occupied = id != 0;
      int64_t pp[4];
      int pb[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        pp[e] = occupied ? pos[e] + vel[e] : 0;
        pb[e] = yfi_motion_box(pp[e]);
      }
      const double sarea = yfi_nms_area(pb[0], pb[1], pb[2], pb[3]);

      // ---- match: the weights, then the search ----
      uint64_t dfree = m >= 64 ? ~0ull : (1ull << m) - 1ull;       // the detections still unmatched (wave-uniform)
      int matched = -1;
      bool any = false;
      for (int i = 0; i < m; ++i) {
        double iou;
        const int ok = yfi_track_iou(pb[0], pb[1], pb[2], pb[3], sarea, bcast(dw[3], i), bcast(dw[4], i), bcast(dw[5], i), bcast(dw[6], i),
                                     bcast(darea, i), a.match_iou, &iou);
        const int32_t wt = yfi_assign_weight(ok && occupied, iou);
        weights[i * 64 + lane] = wt;
        any = any || wt != 0;
      }
      if (__ballot(any) != 0) {
        matched = solve(weights, m, lane);
        uint32_t lo = matched >= 0 && matched < 32 ? 1u << matched : 0u, hi = matched >= 32 ? 1u << (matched - 32) : 0u;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { lo |= __shfl_xor(lo, d); hi |= __shfl_xor(hi, d); }
        lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)lo); hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)hi);
        dfree &= ~((uint64_t)hi << 32 | lo);
      }

      // ---- update ----
      if (occupied) {
        age = yfi_track_inc(age);
        if (matched >= 0) { hits = yfi_track_inc(hits); misses = 0; }
        else misses = yfi_track_inc(misses);
      }
      const bool removed = occupied && matched < 0 && misses > a.max_misses;
      if (removed) {
        id = 0; hits = 0; misses = 0; age = 0; pad = 0;
#pragma unroll
        for (int q = 0; q < 7; ++q) tw[q] = 0;
      }
      const uint64_t free_slots = __ballot(id == 0);
      const int births = min(__popcll(dfree), __popcll(free_slots));
      if (__popcll(dfree) > __popcll(free_slots)) bits |= YFI_TRACK_ST_DROPPED;
      int born = -1;
      for (uint64_t u = dfree, fs = free_slots; u != 0 && fs != 0; u &= u - 1, fs &= fs - 1)
        if (lane == __builtin_ctzll(fs)) born = __builtin_ctzll(u);
      const int src = matched >= 0 ? matched : (born >= 0 ? born : lane);
#pragma unroll
      for (int q = 0; q < 7; ++q) {
        const int v = __shfl(dw[q], src);
        if (matched >= 0 || born >= 0) tw[q] = v;
      }
      if (born >= 0) {
        id = yfi_track_next_id(issued, __popcll(free_slots & below));
        hits = 1; misses = 0; age = 1; pad = 0;
      }
      if (births > 0) issued = yfi_track_next_id(issued, births - 1);
      // the filter: a matched lane corrects, a held-over lane coasts, a removed lane is zero, a born lane starts at its detection; a lane
      // that was free and stays free keeps its bytes
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t z = 256ll * (int64_t)tw[3 + e];
        if (matched >= 0) {
          const int64_t r = z - pp[e];
          pos[e] = yfi_motion_sat(pp[e] + yfi_motion_mul(a.alpha, r));
          vel[e] = yfi_motion_sat(vel[e] + yfi_motion_mul(a.beta, r));
        } else if (born >= 0) {                                     // (a slot freed in this step included)
          pos[e] = z; vel[e] = 0;
        } else if (removed) {
          pos[e] = 0; vel[e] = 0;
        } else if (occupied) {
          pos[e] = yfi_motion_sat(pp[e]);
          vel[e] = yfi_motion_mul(a.damp, vel[e]);
        }
      }

      // ---- emit ----
      const bool emit = id != 0 && hits >= a.min_hits;
      const uint64_t emitting = __ballot(emit);
      int place = 0;
      for (uint64_t e = emitting; e != 0; e &= e - 1) {
        const int k = __builtin_ctzll(e);
        const uint32_t idk = (uint32_t)bcast((int)id, k);
        place += idk < id || (idk == id && k < lane);
      }
      if (emit && place < a.out_cap) {
        const size_t at = (size_t)f * a.out_cap + place;
        const bool filtered = misses > 0 || a.smooth != 0;
        int* o = (int*)(a.out + at);
        o[0] = (int)f;
        o[1] = tw[1]; o[2] = tw[2];
#pragma unroll
        for (int e = 0; e < 4; ++e) o[3 + e] = filtered ? yfi_motion_box(pos[e]) : tw[3 + e];
        int* fo = (int*)(a.info + at);
        fo[0] = (int)id; fo[1] = hits; fo[2] = misses; fo[3] = age;
      }
      if (lane == 0) {
        a.out_counts[f] = __popcll(emitting);
        if (a.status) a.status[f] = bits;
      }
    }

    if (lane == 0) st[0] = issued;
    mine[0] = id; mine[1] = (uint32_t)hits; mine[2] = (uint32_t)misses; mine[3] = (uint32_t)age;
#pragma unroll
    for (int q = 0; q < 7; ++q) mine[4 + q] = (uint32_t)tw[q];
    mine[11] = pad;
#pragma unroll
    for (int e = 0; e < 4; ++e) { mine64[e] = pos[e]; mine64[4 + e] = vel[e]; }
  }
}

}  // namespace yfassign
