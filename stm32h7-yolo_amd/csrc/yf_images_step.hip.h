// The three trackers' kernels -- yftrack::step_kernel (yf_images_track_device, csrc/yf_images_track.h), yfmotion::step_kernel (with the
// motion model, yf_images_track_motion_device, csrc/yf_images_motion.h) and yfassign::step_kernel (with the motion model and the optimal
// assignment, yf_images_track_motion_assign_device with YF_ASSIGN_OPTIMAL, csrc/yf_images_assign.h) -- as three instantiations of one
// step body, yfstep::run<kMotion, kOptimal>.  Included by yf_images.hip.
//
// One wave per stream, lane = slot.  The stream's state is loaded once -- `issued` wave-uniform, a slot's words in its lane's registers:
// eleven, or with kMotion all 28 (pad, pos[4], vel[4]) --, kept there over the stream's steps and stored once at the end; a workgroup
// that takes another stream loads that stream's.  Nothing is indexed by a value read from the state.  Every branch is wave-uniform (the
// grid stride, the steps, the loops over the bits of ballot masks, the searches): the lanes differ only in selects, so every cross-lane
// read below runs with all 64 lanes active.
//   detections  lane j holds record j of the frame (j < m) and its area.
//   predict     (kMotion) pos + vel per edge, a chain of 64-bit integer operations; its box is what the match sees in the place of the
//               slot's last record.  pos and vel of an occupied slot pass yfi_motion_sat when they are loaded and whenever they are
//               written; a free slot's are carried as the bytes they are and take part in nothing.
//   match       greedy: every occupied lane keeps its best eligible unmatched detection (IoU bits, index; a scan over the bits of the
//               wave-uniform mask of unmatched detections, each detection's edges and area broadcast by v_readlane).  A round: the winner
//               is the cross-lane maximum of the key (IoU bits, then lower detection, then lower slot -- a positive double orders as its
//               bits do), a six-step butterfly; winner slot and detection leave the game; only the lanes whose best was that detection
//               scan again.  At most min(m, occupied) rounds.
//               optimal (kOptimal):
//     weights   the m x 64 table once per step, by the scan of the greedy's first round -- detection i's edges and area broadcast, lane j
//               computes its IoU --, kept as int32 in 16 KB of LDS, row i contiguous: lane j reads and writes word i * 64 + j, one word
//               per bank and lane, free of bank conflicts.  A step without an eligible pair skips the search.
//     search    lane-parallel by column: v, minv, way, used and the assigned row p of column j live in lane j; u and "visited" of row r
//               in lane r.  i0 and j0 are wave-uniform (scalar registers, which is why m passes readfirstlane); u[i0] and p[j0] are read
//               with readlane.  0 <= minv <= 2^31 + 2 (the header's bound) for every column relaxed, and every unused column is relaxed
//               before the minimum is taken, so the minimum is a 32-bit unsigned butterfly with used columns at 0xFFFFFFFF -- at most 63
//               columns are used, so one candidate is always left --, and the lowest lane attaining it is the lowest bit of a ballot.
//     result    lane j's detection is p if w[p][j] > 0, read back from the table (p is a row this search assigned: 0 <= p < m).
//               The LDS is the wave's own (one-wave workgroups) and lane j reads only the words it wrote itself in this step (column j
//               of the rows below m): no barrier is needed, within a step, between steps or between a workgroup's streams.
//   update      counters per lane; the free slots after the removals and the unmatched detections are two 64-bit masks whose set bits
//               are paired in ascending order (a scalar loop); one gather (ds_bpermute) brings a matched or born slot its record; then
//               (kMotion) the filter per edge.
//   emit        a lane's place is the number of emitting lanes with a smaller (id, slot).
#pragma once
#include <type_traits>

#include "yf_images_assign.h"

namespace yfstep {

static_assert(YF_TRACK_SLOTS == 64 && YF_TRACK_MAX_DETS == 64, "one lane per slot and per detection");

// workgroups of each kernel a CU holds at once, the measure of its grid (the 16 KB of LDS halve the last); tests/track_support.py reads
// this line, so that the tests of a workgroup's second stream follow the launcher
constexpr int kPerCuTrack = 16, kPerCuMotion = 16, kPerCuAssign = 8;

struct Args {
  const yf_det* dets;
  const int* counts;
  long streams, steps;
  int layout, cap;
  double match_iou;
  int min_hits, max_misses;
  uint32_t* state;
  yf_det* out;
  yf_track_info* info;
  int* out_counts;
  int out_cap;
  int* status;
};

struct MotionArgs : Args {
  int alpha, beta, damp, smooth;
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

// the greedy match of this lane's box against the detections in dfree -> this lane's detection, -1 for none; dfree loses the matched
__device__ __forceinline__ int greedy(const int (&box)[4], double sarea, const int (&dw)[7], double darea, bool occupied, double match_iou,
                                      int lane, uint64_t& dfree) {
  bool sfree = occupied;                                         // this slot is occupied and still unmatched
  bool need = occupied;                                          // ... and has to scan
  int matched = -1;
  uint64_t best = 0;                                             // the IoU's bits; 0: no eligible detection
  int best_j = 0;
  for (;;) {
    if (__ballot(need) != 0) {
      if (need) best = 0;
      for (uint64_t r = dfree; r != 0; r &= r - 1) {
        const int j = __builtin_ctzll(r);
        double iou;
        const int ok = yfi_track_iou(box[0], box[1], box[2], box[3], sarea, bcast(dw[3], j), bcast(dw[4], j), bcast(dw[5], j),
                                     bcast(dw[6], j), bcast(darea, j), match_iou, &iou);
        const uint64_t u = (uint64_t)__double_as_longlong(iou);
        if (need && ok && u > best) { best = u; best_j = j; }    // ascending j and a strict comparison: ties keep the lower detection
      }
    }
    const bool cand = sfree && best != 0;
    uint32_t hi = cand ? (uint32_t)(best >> 32) : 0u, lo = cand ? (uint32_t)best : 0u;
    uint32_t pair = cand ? (uint32_t)((63 - best_j) << 6 | (63 - lane)) : 0u;            // larger: lower detection, then lower slot
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t ohi = __shfl_xor(hi, d), olo = __shfl_xor(lo, d), opair = __shfl_xor(pair, d);
      const bool take = ohi > hi || (ohi == hi && (olo > lo || (olo == lo && opair > pair)));
      hi = take ? ohi : hi; lo = take ? olo : lo; pair = take ? opair : pair;
    }
    hi = __builtin_amdgcn_readfirstlane(hi); lo = __builtin_amdgcn_readfirstlane(lo);     // every lane holds the maximum: say so
    pair = __builtin_amdgcn_readfirstlane(pair);
    if ((hi | lo) == 0) break;
    const int J = 63 - (int)(pair >> 6), W = 63 - (int)(pair & 63u);
    if (lane == W) { matched = J; sfree = false; }
    dfree &= ~(1ull << J);
    need = sfree && best != 0 && best_j == J;                    // the lanes that lost their detection
  }
  return matched;
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

// the optimal match with `greedy`'s arguments and the table's place: the weights, then the search
__device__ __forceinline__ int optimal(int32_t* weights, const int (&box)[4], double sarea, const int (&dw)[7], double darea, bool occupied,
                                       double match_iou, int m, int lane, uint64_t& dfree) {
  int matched = -1;
  int32_t any = 0;                                               // the OR of this lane's weights, none of which is negative
  for (int i = 0; i < m; ++i) {
    double iou;
    const int ok = yfi_track_iou(box[0], box[1], box[2], box[3], sarea, bcast(dw[3], i), bcast(dw[4], i), bcast(dw[5], i), bcast(dw[6], i),
                                 bcast(darea, i), match_iou, &iou);
    const int32_t wt = occupied ? yfi_assign_weight(ok, iou) : 0;  // every pair of a free slot weighs 0
    weights[i * 64 + lane] = wt;
    any |= wt;
  }
  if (__ballot(any != 0) != 0) {
    matched = solve(weights, m, lane);
    uint32_t lo = matched >= 0 && matched < 32 ? 1u << matched : 0u, hi = matched >= 32 ? 1u << (matched - 32) : 0u;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { lo |= __shfl_xor(lo, d); hi |= __shfl_xor(hi, d); }
    lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)lo); hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)hi);
    dfree &= ~((uint64_t)hi << 32 | lo);
  }
  return matched;
}

// a workgroup's streams, each over its steps.  kMotion: the 28-word slot, predict, the filter and the filtered emit; kOptimal: the
// optimal match on `weights`, int32[64][64] of LDS (not read otherwise)
template <bool kMotion, bool kOptimal>
__device__ __forceinline__ void run(const std::conditional_t<kMotion, MotionArgs, Args>& a, int32_t* weights) {
  static_assert(kMotion || !kOptimal, "the optimal match comes with the motion model");
  constexpr int kSlotWords = kMotion ? YFI_MOTION_SLOT_WORDS : YFI_TRACK_SLOT_WORDS;
  constexpr int kStateWords = kMotion ? YFI_MOTION_STATE_WORDS : YFI_TRACK_STATE_WORDS;
  const int lane = threadIdx.x;
  const uint64_t below = (1ull << lane) - 1ull;
  for (long s = blockIdx.x; s < a.streams; s += gridDim.x) {
    uint32_t* st = a.state + (size_t)s * kStateWords;
    uint32_t issued = st[0];
    uint32_t* mine = st + 2 + lane * kSlotWords;                   // kMotion: 8 + 112 * lane bytes into an 8-byte aligned state
    int64_t* mine64 = (int64_t*)(mine + 12);
    uint32_t id = mine[0];
    int hits = (int)mine[1], misses = (int)mine[2], age = (int)mine[3];
    int tw[7];
#pragma unroll
    for (int q = 0; q < 7; ++q) tw[q] = (int)mine[4 + q];
    uint32_t pad = 0;                                              // these nine are the motion model's alone
    int64_t pos[4] = {0, 0, 0, 0}, vel[4] = {0, 0, 0, 0};
    if constexpr (kMotion) {
      pad = mine[11];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t p = mine64[e], v = mine64[4 + e];
        pos[e] = id != 0 ? yfi_motion_sat(p) : p;
        vel[e] = id != 0 ? yfi_motion_sat(v) : v;
      }
    }

    for (long t = 0; t < a.steps; ++t) {
      const long f = a.layout == YF_TRACK_TIME_MAJOR ? t * a.streams + s : s * a.steps + t;
      const int c = a.counts[f];
      int m = yfi_track_clamp(c, a.cap);
      if constexpr (kOptimal) m = __builtin_amdgcn_readfirstlane(m);
      int bits = yfi_track_clipped(c, a.cap) ? YFI_TRACK_ST_CLIPPED : 0;
      const int* in = (const int*)(a.dets + (size_t)f * a.cap);
      int dw[7] = {0, 0, 0, 0, 0, 0, 0};
      if (lane < m) {
#pragma unroll
        for (int q = 0; q < 7; ++q) dw[q] = in[lane * 7 + q];
      }
      const double darea = yfi_nms_area(dw[3], dw[4], dw[5], dw[6]);

      // ---- predict ----  the box the match sees
      const bool occupied = id != 0;
      int64_t pp[4] = {0, 0, 0, 0};
      int box[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if constexpr (kMotion) {
          pp[e] = occupied ? pos[e] + vel[e] : 0;
          box[e] = yfi_motion_box(pp[e]);
        } else {
          box[e] = tw[3 + e];
        }
      }
      const double sarea = yfi_nms_area(box[0], box[1], box[2], box[3]);

      // ---- match ----
      uint64_t dfree = m >= 64 ? ~0ull : (1ull << m) - 1ull;       // the detections still unmatched (wave-uniform)
      int matched;
      if constexpr (kOptimal) matched = optimal(weights, box, sarea, dw, darea, occupied, a.match_iou, m, lane, dfree);
      else matched = greedy(box, sarea, dw, darea, occupied, a.match_iou, lane, dfree);

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
      if constexpr (kMotion) {
        // the filter: a matched lane corrects, a held-over lane coasts, a removed lane is zero, a born lane starts at its detection; a
        // lane that was free and stays free keeps its bytes
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int64_t z = 256ll * (int64_t)tw[3 + e];
          if (matched >= 0) {
            const int64_t r = z - pp[e];
            pos[e] = yfi_motion_sat(pp[e] + yfi_motion_mul(a.alpha, r));
            vel[e] = yfi_motion_sat(vel[e] + yfi_motion_mul(a.beta, r));
          } else if (born >= 0) {                                   // (a slot freed in this step included)
            pos[e] = z; vel[e] = 0;
          } else if (removed) {
            pos[e] = 0; vel[e] = 0;
          } else if (occupied) {
            pos[e] = yfi_motion_sat(pp[e]);
            vel[e] = yfi_motion_mul(a.damp, vel[e]);
          }
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
        bool filtered = false;                                     // the box that moved on, or the smoothed one
        if constexpr (kMotion) filtered = misses > 0 || a.smooth != 0;
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
    if constexpr (kMotion) {
      mine[11] = pad;
#pragma unroll
      for (int e = 0; e < 4; ++e) { mine64[e] = pos[e]; mine64[4 + e] = vel[e]; }
    }
  }
}

}  // namespace yfstep

// the kernels, by the names the resource tests count them by
namespace yftrack {
__global__ void __launch_bounds__(64) step_kernel(yfstep::Args a) { yfstep::run<false, false>(a, nullptr); }
}  // namespace yftrack

namespace yfmotion {
__global__ void __launch_bounds__(64) step_kernel(yfstep::MotionArgs a) { yfstep::run<true, false>(a, nullptr); }
}  // namespace yfmotion

namespace yfassign {
__global__ void __launch_bounds__(64) step_kernel(yfstep::MotionArgs a) {
  __shared__ int32_t weights[YF_TRACK_MAX_DETS * YF_TRACK_SLOTS];  // 16 KB: [detection][slot]
  yfstep::run<true, true>(a, weights);
}
}  // namespace yfassign
