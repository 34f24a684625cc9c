// The kernel of the re-identification -- yfreid::stream_kernel (yf_images_reid_device, csrc/yf_images_reid.h): the ids of a tracker's
// output rewritten, per stream over the steps of a call.  Included by yf_images.hip after yf_images_step.hip.h, whose broadcasts
// (yfstep::bcast) it uses as they are.
//
// One wave per stream with a grid stride over the streams; lane e = entry e of the stream's table, and also lane r = record r of the
// frame.  The entry's 20 words -- id, alias, seen, flags and the 16 words of its descriptor -- are loaded once, kept in registers over the
// stream's steps and stored once at the end; the clock is wave-uniform; a workgroup that takes another stream loads that stream's.
// Nothing is indexed by a value read from the state: an entry is reached by a ballot of the lanes whose registers say so.  Every branch
// is wave-uniform (the grid stride, the steps, the loops over the bits of ballot masks); the lanes differ only in selects, so every
// cross-lane read runs with all 64 lanes active.
//   records     lane r holds record r's tracker id, hits, misses, age and its descriptor's flags (r < m).  A record's 16 descriptor words
//               are loaded where they are needed, at a wave-uniform address.
//   bind        a scalar loop over the records that are not void, ascending: "the lowest entry with that alias" is the lowest bit of a
//               ballot; its lane takes seen = now and, for a record detected with a valid descriptor, the blend.
//   expire      per lane.
//   re-identify skipped unless an unbound candidate record and a candidate entry exist -- a frame without an unbound record computes no
//               distance.  Row r of the table: lane e computes d(record r, entry e) and keeps it as int32 in 16 KB of LDS, word r * 64
//               + e: one word per bank and lane.  A lane reads only the words it wrote itself, so no barrier is needed, within a step,
//               between steps or between a workgroup's streams.  Then the greedy: every lane's best key (d << 12 | r << 6 | e) over
//               the records still in play, the wave's minimum by cross-lane moves, the pair taken, until none is eligible.
//   births      a scalar loop over the records still unbound: the lowest free entry is the lowest bit of a ballot; without one, the
//               wave's maximum age among the unbound entries and the lowest lane that has it.
#pragma once

#include "yf_images_reid.h"
#include "yf_images_step.hip.h"

namespace yfreid {

// workgroups of the kernel a CU holds at once, the measure of its grid (16 KB of LDS each); tests/reid_support.py reads this line, so
// that the test of a workgroup's second stream follows the launcher
constexpr int kPerCuReid = 8;
constexpr int kWords = YF_DESC_BYTES / 4;
static_assert(YFI_REID_MAX_DISTANCE < (1 << 20), "a distance, a record and an entry in one 32-bit key");

struct Args {
  const yf_track_info* info;
  const int* out_counts;
  const yf_face_desc* desc;
  int out_cap;
  long streams, steps;
  int layout;
  int max_distance, max_age, blend;
  yf_reid_state* state;
  yf_track_info* info_out;
  int* what;
  int* status;
};

using yfstep::bcast;

// the 16 descriptor words of a record, at a wave-uniform address; live = false: zeros, nothing is loaded.  The address is handed to the
// compiler as a per-lane value, so that the words arrive in vector registers: sixteen more scalars would not fit beside the masks
__device__ __forceinline__ void load_desc(const yf_face_desc* d, bool live, uint32_t (&w)[kWords]) {
  const uint32_t* p = (const uint32_t*)d;
  asm volatile("" : "+v"(p));
#pragma unroll
  for (int k = 0; k < kWords; ++k) w[k] = live ? p[1 + k] : 0u;
}

__device__ __forceinline__ int32_t byte_sum(const uint32_t (&w)[kWords]) {
  uint32_t s = 0;
#pragma unroll
  for (int k = 0; k < kWords; ++k) s += (w[k] & 255u) + (w[k] >> 8 & 255u) + (w[k] >> 16 & 255u) + (w[k] >> 24);
  return (int32_t)s;
}

// yfi_reid_update in the lane that says `mine`: the entry's descriptor after it has met the valid descriptor nw
__device__ __forceinline__ void meet(uint32_t (&v)[kWords], uint32_t& flags, const uint32_t (&nw)[kWords], int blend, bool mine) {
  const bool has = (flags & YFI_REID_HAS_DESC) != 0;
#pragma unroll
  for (int k = 0; k < kWords; ++k) {
    uint32_t b = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) b |= yfi_reid_blend(v[k] >> (8 * q) & 255u, nw[k] >> (8 * q) & 255u, blend) << (8 * q);
    v[k] = mine ? (has ? b : nw[k]) : v[k];
  }
  flags = mine ? flags | YFI_REID_HAS_DESC : flags;
}

// yfi_reid_distance of this lane's entry (sum A) and a record's words (sum B)
__device__ __forceinline__ int32_t distance(const uint32_t (&v)[kWords], int32_t A, const uint32_t (&nw)[kWords], int32_t B) {
  int32_t d = 0;
#pragma unroll
  for (int k = 0; k < kWords; ++k)
#pragma unroll
    for (int q = 0; q < 4; ++q) d += yfi_reid_term((int32_t)(nw[k] >> (8 * q) & 255u), B, (int32_t)(v[k] >> (8 * q) & 255u), A);
  return d;
}

__global__ void __launch_bounds__(64) stream_kernel(Args a) {
  __shared__ int32_t dist[YF_REID_ENTRIES * YF_REID_ENTRIES];       // 16 KB: [record][entry]
  const int lane = threadIdx.x;
  for (long s = blockIdx.x; s < a.streams; s += gridDim.x) {
    uint32_t* sw = (uint32_t*)(a.state + s);
    uint32_t* ew = sw + 2 + lane * YFI_REID_ENTRY_WORDS;
    uint32_t clock = (uint32_t)__builtin_amdgcn_readfirstlane((int)sw[0]);
    uint32_t id = ew[0], alias = ew[1], seen = ew[2], flags = ew[3], v[kWords];
#pragma unroll
    for (int k = 0; k < kWords; ++k) v[k] = ew[4 + k];

    for (long t = 0; t < a.steps; ++t) {
      const long f = a.layout == YF_TRACK_TIME_MAJOR ? t * a.streams + s : s * a.steps + t;
      const size_t at = (size_t)f * (size_t)a.out_cap;
      const int cnt = a.out_counts[f];
      const int m = __builtin_amdgcn_readfirstlane(yfi_track_clamp(cnt, a.out_cap));
      int bits = yfi_track_clipped(cnt, a.out_cap) ? YFI_REID_ST_CLIPPED : 0;

      // ---- records ----
      uint32_t tid = 0, hits = 0, misses = 0, age = 0, dflags = 0;
      if (lane < m) {
        const uint32_t* in = (const uint32_t*)(a.info + at + lane);
        tid = in[0]; hits = in[1]; misses = in[2]; age = in[3];
        dflags = ((const uint32_t*)(a.desc + at + lane))[0];
      }
      const bool live = lane < m && tid != 0;
      const uint64_t valid_mask = __ballot(lane < m && (dflags & YF_DESC_VALID) != 0);
      const uint64_t fresh_mask = __ballot(live && misses == 0 && (dflags & YF_DESC_VALID) != 0);
      if (__ballot(lane < m && tid == 0) != 0) bits |= YFI_REID_ST_VOID;
      const uint32_t now = ++clock;
      uint32_t out_id = 0;
      int kind = 0;
      bool bound = false;                                              // this lane's entry
      uint32_t nw[kWords];

      // ---- bind ----
      for (uint64_t rm = __ballot(live); rm != 0; rm &= rm - 1) {
        const int r = __builtin_ctzll(rm);
        const uint32_t tr = (uint32_t)bcast((int)tid, r);
        const uint64_t em = __ballot(id != 0 && alias == tr);
        if (em == 0) continue;
        const int e = __builtin_ctzll(em);
        const bool mine = lane == e;
        const uint32_t eid = (uint32_t)bcast((int)id, e);
        bound = bound || mine;
        seen = mine ? now : seen;
        if (lane == r) { kind = YF_REID_KNOWN; out_id = eid; }
        if ((fresh_mask >> r & 1) != 0) {
          load_desc(a.desc + at + r, true, nw);
          meet(v, flags, nw, a.blend, mine);
        }
      }

      // ---- expire ----
      if (id != 0 && !bound && (uint32_t)(now - seen) > (uint32_t)a.max_age) {
        id = 0; alias = 0; seen = 0; flags = 0;
#pragma unroll
        for (int k = 0; k < kWords; ++k) v[k] = 0;
      }

      // ---- re-identify ----
      uint64_t rc = fresh_mask & __ballot(kind == 0);
      bool ecand = !bound && id != 0 && (flags & YFI_REID_HAS_DESC) != 0;
      if (rc != 0 && __ballot(ecand) != 0) {
        const int32_t A = byte_sum(v);
        for (uint64_t rm = rc; rm != 0; rm &= rm - 1) {
          const int r = __builtin_ctzll(rm);
          load_desc(a.desc + at + r, true, nw);
          dist[r * 64 + lane] = distance(v, A, nw, byte_sum(nw));
        }
        while (rc != 0) {
          uint32_t key = 0xFFFFFFFFu;
          for (uint64_t rm = rc; rm != 0; rm &= rm - 1) {
            const int r = __builtin_ctzll(rm);
            const int32_t d = dist[r * 64 + lane];
            const uint32_t k = ecand && d <= a.max_distance ? (uint32_t)d << 12 | (uint32_t)r << 6 | (uint32_t)lane : 0xFFFFFFFFu;
            key = k < key ? k : key;
          }
#pragma unroll
          for (int d = 1; d < 64; d <<= 1) {
            const uint32_t other = __shfl_xor(key, d);
            key = other < key ? other : key;
          }
          key = (uint32_t)__builtin_amdgcn_readfirstlane((int)key);
          if (key == 0xFFFFFFFFu) break;
          const int r = (int)(key >> 6 & 63u), e = (int)(key & 63u);
          const bool mine = lane == e;
          const uint32_t tr = (uint32_t)bcast((int)tid, r), eid = (uint32_t)bcast((int)id, e);
          alias = mine ? tr : alias;
          seen = mine ? now : seen;
          load_desc(a.desc + at + r, true, nw);
          meet(v, flags, nw, a.blend, mine);
          bound = bound || mine;
          ecand = ecand && !mine;
          if (lane == r) { kind = YF_REID_REIDENTIFIED; out_id = eid; }
          rc &= ~(1ull << r);
        }
      }

      // ---- births ----
      for (uint64_t rm = __ballot(live && kind == 0); rm != 0; rm &= rm - 1) {
        const int r = __builtin_ctzll(rm);
        const uint64_t fm = __ballot(id == 0);
        int e;
        if (fm != 0) {
          e = __builtin_ctzll(fm);
        } else {
          const uint32_t mine_age = now - seen;
          uint32_t top = bound ? 0u : mine_age;
#pragma unroll
          for (int d = 1; d < 64; d <<= 1) {
            const uint32_t other = __shfl_xor(top, d);
            top = other > top ? other : top;
          }
          top = (uint32_t)__builtin_amdgcn_readfirstlane((int)top);
          const uint64_t om = __ballot(!bound && mine_age == top);
          if (om == 0) continue;                                       // not reached: fewer than 64 entries are bound here
          e = __builtin_ctzll(om);
        }
        const bool mine = lane == e, has = (valid_mask >> r & 1) != 0;
        const uint32_t tr = (uint32_t)bcast((int)tid, r);
        load_desc(a.desc + at + r, has, nw);
        id = mine ? tr : id;
        alias = mine ? tr : alias;
        seen = mine ? now : seen;
        flags = mine ? (has ? YFI_REID_HAS_DESC : 0u) : flags;
#pragma unroll
        for (int k = 0; k < kWords; ++k) v[k] = mine ? nw[k] : v[k];
        bound = bound || mine;
        if (lane == r) { kind = YF_REID_BORN; out_id = tid; }
      }

      // ---- output ----
      if (lane < m) {
        uint32_t* o = (uint32_t*)(a.info_out + at + lane);
        o[0] = out_id; o[1] = hits; o[2] = misses; o[3] = age;
        if (a.what) a.what[at + lane] = kind;
      }
      const int all = cnt < 0 ? 0 : (cnt > a.out_cap ? a.out_cap : cnt);
      for (int r = m + lane; r < all; r += 64) {                       // beyond the 64 that count: as they are
        const uint32_t* in = (const uint32_t*)(a.info + at + r);
        const uint32_t w0 = in[0], w1 = in[1], w2 = in[2], w3 = in[3];
        uint32_t* o = (uint32_t*)(a.info_out + at + r);
        o[0] = w0; o[1] = w1; o[2] = w2; o[3] = w3;
        if (a.what) a.what[at + r] = 0;
      }
      if (lane == 0 && a.status) a.status[f] = bits;
    }

    if (lane == 0) sw[0] = clock;
    ew[0] = id; ew[1] = alias; ew[2] = seen; ew[3] = flags;
#pragma unroll
    for (int k = 0; k < kWords; ++k) ew[4 + k] = v[k];
  }
}

}  // namespace yfreid
