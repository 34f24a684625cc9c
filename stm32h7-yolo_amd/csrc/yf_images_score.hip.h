// The kernel of the CLEAR-MOT score -- yfscore::clip_kernel (yf_images_score_tracks_device, csrc/yf_images_score.h): a tracker's reported
// records against ground-truth tracks, per stream over the steps of a clip.  Included by yf_images.hip after yf_images_step.hip.h, whose
// search (yfstep::solve) and broadcasts (yfstep::bcast) it uses as they are.
//
// One wave per stream with a grid stride over the streams, lane i = ground-truth row i, lane j = hypothesis column j.  The stream's state
// is loaded once -- the eight counters wave-uniform, entry e of the three per-object tables (last, present, tracked) in register e / 64 of
// lane e % 64 --, kept there over the stream's steps and stored once at the end; a workgroup that takes another stream loads that
// stream's.  Nothing is indexed by a value read from the state, and no memory is addressed by an id at all: an entry is reached by a
// readlane of a register chosen by wave-uniform selects.  Every branch is wave-uniform (the grid stride, the steps, the loops over the
// rows and over the bits of ballot masks, the search): the lanes differ only in selects, so every cross-lane read runs with all 64 lanes
// active.
//   rows        lane i holds row i of the frame (i < g), its area, and whether it is void: its id out of range, or an earlier row's id
//               (a scan of the ids broadcast one by one).  The rows that count are a wave-uniform mask.
//   columns     lane j holds the box and the id of record j (j < h) and its area.
//   weights     the g x 64 table as the assign kernel lays it out: row i's edges and area broadcast, lane j computes its IoU and
//               keeps the weight as int32 in 16 KB of LDS, word i * 64 + j: one word per bank and lane.  Lane j reads only the words it
//               wrote itself (column j of the rows below g); where another lane's word is wanted it comes by readlane from its owner.
//               So no barrier is needed, within a step, between steps or between a workgroup's streams.
//   continuity  a scalar loop over the rows that count, ascending: last[o - 1] by readlane, "the lowest column of that id" the lowest bit
//               of a ballot, "no lower row kept it" a bit of the wave-uniform mask of kept columns, w[i][j] from lane j.
//   the rest    the weights of kept rows and columns zeroed in place, then yfstep::solve on all g rows (skipped when no weight is left).
//   counting    a second scalar loop over the rows that count: the row's column is the ballot of the lanes that hold it (a kept pair
//               or the search's), the switch test and the sums run on wave-uniform values, and the owner lane of entry o - 1 updates
//               its registers.
#pragma once

#include "yf_images_score.h"
#include "yf_images_step.hip.h"

namespace yfscore {

static_assert(YF_SCORE_MAX_IDS == 4 * 64, "four entries of every per-object table per lane");

// workgroups of the kernel a CU holds at once, the measure of its grid (16 KB of LDS each); tests/score_support.py reads this line, so
// that the test of a workgroup's second stream follows the launcher
constexpr int kPerCuScore = 8;

struct Args {
  const yf_det* out;
  const yf_track_info* info;
  const int* out_counts;
  int out_cap;
  const yf_gt_track* gt;
  const int* gt_counts;
  int gt_cap;
  long streams, steps;
  int layout;
  double score_iou;
  yf_score_state* state;
  int* match;
  int* status;
};

using yfstep::bcast;

// entry q (wave-uniform) of a lane's four
__device__ __forceinline__ uint32_t pick(const uint32_t (&r)[4], int q) { return q == 0 ? r[0] : q == 1 ? r[1] : q == 2 ? r[2] : r[3]; }

// ... and v into it, in the lane that says `mine`; a q outside 0 .. 3 writes nothing
__device__ __forceinline__ void put(uint32_t (&r)[4], int q, bool mine, uint32_t v) {
#pragma unroll
  for (int k = 0; k < 4; ++k) r[k] = mine && q == k ? v : r[k];
}

__global__ void __launch_bounds__(64) clip_kernel(Args a) {
  __shared__ int32_t weights[YF_SCORE_MAX_ROWS * YF_TRACK_SLOTS];    // 16 KB: [row][column]
  const int lane = threadIdx.x;
  for (long s = blockIdx.x; s < a.streams; s += gridDim.x) {
    yf_score_state* st = a.state + s;
    uint64_t* c64 = (uint64_t*)st;
    uint64_t cnt[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) cnt[k] = c64[k];
    uint32_t last[4], present[4], tracked[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      last[q] = st->last[q * 64 + lane];
      present[q] = (uint32_t)st->present[q * 64 + lane];
      tracked[q] = (uint32_t)st->tracked[q * 64 + lane];
    }

    for (long t = 0; t < a.steps; ++t) {
      const long f = a.layout == YF_TRACK_TIME_MAJOR ? t * a.streams + s : s * a.steps + t;
      const int cg = a.gt_counts[f], ch = a.out_counts[f];
      const int g = __builtin_amdgcn_readfirstlane(yfi_track_clamp(cg, a.gt_cap));
      const int h = __builtin_amdgcn_readfirstlane(yfi_track_clamp(ch, a.out_cap));
      int bits = (yfi_track_clipped(cg, a.gt_cap) ? YFI_SCORE_ST_GT_CLIPPED : 0) | (yfi_track_clipped(ch, a.out_cap) ? YFI_SCORE_ST_HYP_CLIPPED : 0);

      // ---- rows ----
      uint32_t rid = 0;
      int rb[4] = {0, 0, 0, 0};
      if (lane < g) {
        const int* in = (const int*)(a.gt + (size_t)f * a.gt_cap) + lane * 5;
        rid = (uint32_t)in[0];
#pragma unroll
        for (int e = 0; e < 4; ++e) rb[e] = in[1 + e];
      }
      const double rarea = yfi_nms_area(rb[0], rb[1], rb[2], rb[3]);
      bool repeat = false;                                           // an earlier row of the frame has this id
      for (int i = 0; i < g; ++i) {
        const uint32_t o = (uint32_t)bcast((int)rid, i);
        repeat = repeat || (i < lane && o == rid);
      }
      const bool row_ok = lane < g && yfi_score_id_ok(rid) && !repeat;
      const uint64_t rows_mask = __ballot(row_ok);
      if (__ballot(lane < g && !row_ok) != 0) bits |= YFI_SCORE_ST_GT_VOID;

      // ---- columns ----
      uint32_t hid = 0;
      int cb[4] = {0, 0, 0, 0};
      if (lane < h) {
        const int* o = (const int*)(a.out + (size_t)f * a.out_cap) + lane * 7;
#pragma unroll
        for (int e = 0; e < 4; ++e) cb[e] = o[3 + e];
        hid = ((const uint32_t*)(a.info + (size_t)f * a.out_cap))[lane * 4];
      }
      const double carea = yfi_nms_area(cb[0], cb[1], cb[2], cb[3]);
      const bool col_ok = lane < h && hid != 0;
      const uint64_t cols_mask = __ballot(col_ok);
      if (__ballot(lane < h && hid == 0) != 0) bits |= YFI_SCORE_ST_HYP_VOID;

      // ---- weights ----
      for (int i = 0; i < g; ++i) {
        double iou;
        const int ok = yfi_track_iou(bcast(rb[0], i), bcast(rb[1], i), bcast(rb[2], i), bcast(rb[3], i), bcast(rarea, i), cb[0], cb[1], cb[2],
                                     cb[3], carea, a.score_iou, &iou);
        weights[i * 64 + lane] = (rows_mask >> i & 1) != 0 && col_ok ? yfi_assign_weight(ok, iou) : 0;
      }

      // ---- continuity ----
      uint64_t kept_rows = 0, kept_cols = 0;                         // wave-uniform
      int krow = -1;                                                 // this column's kept row, and the pair's weight
      int32_t kw = 0;
      for (uint64_t r = rows_mask; r != 0; r &= r - 1) {
        const int i = __builtin_ctzll(r);
        const int e = bcast((int)rid, i) - 1;                        // 0 .. 255: row i is not void
        const uint32_t k = (uint32_t)bcast((int)pick(last, e >> 6), e & 63);
        if (k == 0) continue;
        const uint64_t cm = __ballot(col_ok && hid == k);
        if (cm == 0) continue;
        const int j = __builtin_ctzll(cm);                           // the lowest column of that id
        const int32_t wij = bcast(weights[i * 64 + lane], j);
        if ((kept_cols >> j & 1) != 0 || wij <= 0) continue;
        kept_rows |= 1ull << i;
        kept_cols |= 1ull << j;
        if (lane == j) { krow = i; kw = wij; }
      }

      // ---- the rest ----
      const bool col_kept = (kept_cols >> lane & 1) != 0;
      int32_t any = 0;                                               // the OR of this lane's weights, none of which is negative
      for (int i = 0; i < g; ++i) {
        const int32_t wt = (kept_rows >> i & 1) != 0 || col_kept ? 0 : weights[i * 64 + lane];
        weights[i * 64 + lane] = wt;
        any |= wt;
      }
      int p = -1;
      if (__ballot(any != 0) != 0) p = yfstep::solve(weights, g, lane);
      const int prow = krow >= 0 ? krow : p;                         // this column's row, kept or new, -1 for none
      const int32_t pw = krow >= 0 ? kw : (p >= 0 ? weights[(p >= 0 ? p : 0) * 64 + lane] : 0);

      // ---- switches, counters, tables ----
      int mcol = -1;                                                 // this row's column
      uint64_t matches = 0, switches = 0, overlap = 0;
      for (uint64_t r = rows_mask; r != 0; r &= r - 1) {
        const int i = __builtin_ctzll(r);
        const int e = bcast((int)rid, i) - 1, q = e >> 6;
        const bool mine = lane == (e & 63);                          // the lane that holds entry e
        const uint64_t cm = __ballot(prow == i);
        if (cm != 0) {
          const int j = __builtin_ctzll(cm);
          const uint32_t hj = (uint32_t)bcast((int)hid, j);
          const uint32_t k = (uint32_t)bcast((int)pick(last, q), e & 63);
          switches += (kept_rows >> i & 1) == 0 && k != 0 && k != hj;
          matches += 1;
          overlap += (uint64_t)(uint32_t)bcast((int)pw, j);
          if (lane == i) mcol = j;
          put(last, q, mine, hj);
          put(tracked, q, mine, (uint32_t)yfi_track_inc((int32_t)pick(tracked, q)));
        }
        put(present, q, mine, (uint32_t)yfi_track_inc((int32_t)pick(present, q)));
      }
      const uint64_t rows = (uint64_t)__popcll(rows_mask), cols = (uint64_t)__popcll(cols_mask);
      cnt[0] += 1; cnt[1] += rows; cnt[2] += cols; cnt[3] += matches; cnt[4] += rows - matches; cnt[5] += cols - matches;
      cnt[6] += switches; cnt[7] += overlap;

      if (a.match && lane < g) a.match[(size_t)f * a.gt_cap + lane] = mcol;
      if (lane == 0 && a.status) a.status[f] = bits;
    }

    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < 8; ++k) c64[k] = cnt[k];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      st->last[q * 64 + lane] = last[q];
      st->present[q * 64 + lane] = (int32_t)present[q];
      st->tracked[q * 64 + lane] = (int32_t)tracked[q];
    }
  }
}

}  // namespace yfscore
