// The kernel of the tracker with a motion model (yf_images_track_motion_device); the definition is csrc/yf_images_motion.h.  Included
// by yf_images.hip.
//
// The plan is yftrack::step_kernel's (yf_images_track.hip.h): one wave per stream, lane = slot; the stream's state is loaded once --
// `issued` wave-uniform, a slot's 28 words in its lane's registers --, kept there over the stream's steps and stored once at the end.
// Nothing is indexed by a value read from the state.  Every branch is wave-uniform; the lanes differ only in selects, so every cross-lane
// read runs with all 64 lanes active.  The match loop, the pairing of the births and the placement of the output are that kernel's logic,
// restated here on the PREDICTED boxes (that file is not touched: its kernel keeps its instructions); new is the filter, a chain of
// 64-bit integer operations per edge before the match (predict) and after it (update).
//   pos and vel of an occupied slot pass yfi_motion_sat when they are loaded and whenever they are written; a free slot's are carried as
//   the bytes they are and take part in nothing.
#pragma once
#include "yf_images_motion.h"

namespace yfmotion {

constexpr int kSlotWords = YFI_MOTION_SLOT_WORDS, kStateWords = YFI_MOTION_STATE_WORDS;
static_assert(YF_TRACK_SLOTS == 64 && YF_TRACK_MAX_DETS == 64, "one lane per slot and per detection");

struct Args {
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

__global__ void __launch_bounds__(64) step_kernel(Args a) {
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
      const int m = yfi_track_clamp(c, a.cap);
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

      // ---- match ----
      uint64_t dfree = m >= 64 ? ~0ull : (1ull << m) - 1ull;       // the detections still unmatched (wave-uniform)
      bool sfree = occupied;                                       // this slot is occupied and still unmatched
      bool need = occupied;                                        // ... and has to scan
      int matched = -1;
      uint64_t best = 0;                                           // the IoU's bits; 0: no eligible detection
      int best_j = 0;
      for (;;) {
        if (__ballot(need) != 0) {
          if (need) best = 0;
          for (uint64_t r = dfree; r != 0; r &= r - 1) {
            const int j = __builtin_ctzll(r);
            double iou;
            const int ok = yfi_track_iou(pb[0], pb[1], pb[2], pb[3], sarea, bcast(dw[3], j), bcast(dw[4], j), bcast(dw[5], j),
                                         bcast(dw[6], j), bcast(darea, j), a.match_iou, &iou);
            const uint64_t u = (uint64_t)__double_as_longlong(iou);
            if (need && ok && u > best) { best = u; best_j = j; }  // ascending j and a strict comparison: ties keep the lower detection
          }
        }
        const bool cand = sfree && best != 0;
        uint32_t hi = cand ? (uint32_t)(best >> 32) : 0u, lo = cand ? (uint32_t)best : 0u;
        uint32_t pair = cand ? (uint32_t)((63 - best_j) << 6 | (63 - lane)) : 0u;          // larger: lower detection, then lower slot
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const uint32_t ohi = __shfl_xor(hi, d), olo = __shfl_xor(lo, d), opair = __shfl_xor(pair, d);
          const bool take = ohi > hi || (ohi == hi && (olo > lo || (olo == lo && opair > pair)));
          hi = take ? ohi : hi; lo = take ? olo : lo; pair = take ? opair : pair;
        }
        hi = __builtin_amdgcn_readfirstlane(hi); lo = __builtin_amdgcn_readfirstlane(lo);   // every lane holds the maximum: say so
        pair = __builtin_amdgcn_readfirstlane(pair);
        if ((hi | lo) == 0) break;
        const int J = 63 - (int)(pair >> 6), W = 63 - (int)(pair & 63u);
        if (lane == W) { matched = J; sfree = false; }
        dfree &= ~(1ull << J);
        need = sfree && best != 0 && best_j == J;                  // the lanes that lost their detection
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

}  // namespace yfmotion
