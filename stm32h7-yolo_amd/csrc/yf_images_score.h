/* Scoring tracks against labelled identities: the CLEAR-MOT score (K. Bernardin, R. Stiefelhagen, "Evaluating Multiple Object Tracking
 * Performance: The CLEAR MOT Metrics", EURASIP J. Image and Video Processing, 2008) of a tracker's reported records against ground-truth
 * tracks, per stream over the steps of a clip (yf_images_score_tracks_device), shared by the device kernel (yf_images_score.hip.h), the
 * host entry in yf_images.hip, a host build (yf_images_host.c, which tests/test_track_score_host.py checks against ptq.track_score_step)
 * and a sanitizer program (tests/csrc/track_score_sanitize_main.c).  Plain C.
 *
 * The reference has no tracker and no such score: the definition is the library's own.  It is what tells whether the motion model of
 * yf_images_motion.h or the optimal assignment of yf_images_assign.h keeps identities better: misses, false positives, identity switches
 * and MOTA.  Everything after the IoU is integers: the kernel, the host build and Python agree bit for bit.
 *
 * STATE.  yf_score_state per stream (3136 bytes, 8-byte aligned): eight uint64 counters -- frames, gt, hyp, matches, misses,
 * false_positives, switches, overlap -- and three tables indexed by a ground-truth id o - 1 (valid ids 1 .. YF_SCORE_MAX_IDS = 256, an id
 * names one object of its stream): last[o - 1], the hypothesis id object o was last matched to (0: never); present[o - 1], the frames
 * that held object o; tracked[o - 1], those of them on which it was matched.  All zero is the empty state.  The bytes are untrusted:
 * whatever they hold, a step reads and writes only inside them -- THE ONLY VALUE THAT INDEXES THE STATE IS A GROUND-TRUTH ID, AFTER ITS
 * RANGE CHECK.  The counters add modulo 2^64 (unsigned), present and tracked saturate at INT32_MAX (yfi_track_inc), last is only ever
 * compared.
 *
 * ONE STEP: one stream, one frame f with the ground truth gt[f][0 .. gt_cap) / gt_counts[f] and the hypotheses out[f][0 .. out_cap),
 * info[f][0 .. out_cap) (only `id` is read) / out_counts[f], a tracker's output as it lies.
 *  1. Rows: the first g = min(max(gt_count, 0), gt_cap, 64) ground-truth entries (yfi_track_clamp), in the order they lie.  A larger
 *     count sets status bit 0 (YFI_SCORE_ST_GT_CLIPPED).  A row is VOID if its id is 0 or above 256, or if an earlier row of the frame
 *     has the same id: status bit 2 (YFI_SCORE_ST_GT_VOID).  A void row has weight 0 everywhere and counts for nothing: it is not
 *     counted in `gt` and is not a miss.
 *  2. Columns: the first h = min(max(out_count, 0), out_cap, 64) records with their ids.  A larger count sets status bit 1
 *     (YFI_SCORE_ST_HYP_CLIPPED).  A record of id 0 is void in the same way: status bit 3 (YFI_SCORE_ST_HYP_VOID); the trackers never
 *     emit one.
 *  3. Weights: w[i][j] = yfi_assign_weight(yfi_track_iou(row i, column j, score_iou)): the tracker's own float64 IoU with the + 1 pixel
 *     convention and its eligibility rule (inter > 0.0 and iou >= score_iou), unchanged; 1 + (int64)(iou * 2^30) for an eligible pair.  0
 *     for void rows and columns, and for the columns at or beyond h.
 *  4. Continuity, CLEAR-MOT's rule that a valid correspondence is kept.  For the rows in ascending order: o the row's id,
 *     k = last[o - 1]; if k != 0, j the LOWEST column whose id is k; if there is one, no lower row has kept it and w[i][j] > 0, the pair
 *     (i, j) is KEPT.
 *  5. The rest: every weight of a kept row or a kept column is set to 0 and the table with all g rows goes to yfi_assign_solve
 *     (yf_images_assign.h), unchanged, ties and all; its pairs are the NEW matches.  (A table without a positive weight may skip the
 *     search: nothing is matched either way.)
 *  6. Switches: a new match (i, j) whose last[o - 1] is neither 0 nor the id of column j is one identity switch; a kept pair never is
 *     one.  After the counting last[o - 1] = the id of column j for every matched row.  `last` outlives the frames on which its object
 *     is unmatched or absent, as in the paper: an object that returns under another id is one switch.
 *  7. Counters: frames + 1; gt + the rows that are not void; hyp + the columns that are not void; matches + kept + new; misses + rows -
 *     matches; false_positives + columns - matches; switches + those of step 6; overlap + the sum of the matched pairs' weights.  Every
 *     row that is not void: present[o - 1]++; every matched row also tracked[o - 1]++.
 *  8. match[f][i] (if given) for every i < g: the column of row i's hypothesis, -1 for an unmatched and for a void row; the places at
 *     and beyond g are not written.  status[f] (if given): 0 or the bits above.
 *
 * A CALL: n = streams * steps frames in the tracker's layouts (yf_images_track.h); the steps of stream s are taken in order on
 * state[s], which is read before the first and written after the last.
 *
 * THE SUMMARY (yfi_score_summary, host only): the sums of the eight counters over the streams (modulo 2^64); objects, the entries with
 * present > 0, counted per stream; mostly_tracked, those with 5 * tracked >= 4 * present, and mostly_lost, 5 * tracked <= present (int64);
 *   mota = gt ? 1.0 - (double)(misses + false_positives + switches) / (double)gt : 0.0
 *   motp = matches ? ((double)overlap / (double)matches) / 1073741824.0 : 0.0
 * each a chain of single IEEE operations.  motp is the mean IoU of the matched pairs at 2^-30 resolution; EACH WEIGHT CARRIES THE + 1 OF
 * yfi_assign_weight, so motp is above the truncated mean by exactly 2^-30.
 *
 * OUT OF SCOPE.  IDF1 and HOTA: they need one assignment over the whole clip and over hypothesis ids without a bound.  Fragmentations.
 * More than 256 labelled objects per stream or 64 per frame.  Any figure for real labelled video: none is at hand; the figures that exist
 * are those of synthetic clips (profiles/track_score_bench.txt). */
#ifndef YF_IMAGES_SCORE_H
#define YF_IMAGES_SCORE_H
#include <string.h>
#include "yf_images_assign.h"

#define YF_SCORE_MAX_ROWS 64            /* ground-truth rows (and hypothesis columns) of a frame that count: one lane of a wave each */
#define YFI_SCORE_ST_GT_CLIPPED 1       /* status bit 0: gt_count above min(gt_cap, 64) */
#define YFI_SCORE_ST_HYP_CLIPPED 2      /* status bit 1: out_count above min(out_cap, 64) */
#define YFI_SCORE_ST_GT_VOID 4          /* status bit 2: a ground-truth row of id 0, above 256 or repeated */
#define YFI_SCORE_ST_HYP_VOID 8         /* status bit 3: a record of id 0 */
#define YFI_SCORE_STATE_WORDS 784       /* sizeof(yf_score_state) / 4 */

#ifdef __cplusplus
static_assert(sizeof(yf_gt_track) == 20 && sizeof(yf_score_state) == 4 * YFI_SCORE_STATE_WORDS && sizeof(yf_score_state) == 3136 &&
              sizeof(yf_score_summary) == 104 && YF_SCORE_MAX_ROWS == YF_TRACK_SLOTS && YF_SCORE_MAX_ROWS == YF_TRACK_MAX_DETS,
              "the layout include/yf_images.h states");
#else
_Static_assert(sizeof(yf_gt_track) == 20 && sizeof(yf_score_state) == 4 * YFI_SCORE_STATE_WORDS && sizeof(yf_score_state) == 3136 &&
               sizeof(yf_score_summary) == 104 && YF_SCORE_MAX_ROWS == YF_TRACK_SLOTS && YF_SCORE_MAX_ROWS == YF_TRACK_MAX_DETS,
               "the layout include/yf_images.h states");
#endif

/* 1 for an id that names an object: 1 .. YF_SCORE_MAX_IDS */
YFI_HD int yfi_score_id_ok(uint32_t id) { return id >= 1u && id <= (uint32_t)YF_SCORE_MAX_IDS; }

/* THE step, sequentially: steps 1-8 above on one stream's state.  gt and hyp / info are the frame's rows */
static inline void yfi_score_step(yf_score_state* st, const yf_gt_track* gt, int32_t gt_count, int gt_cap, const yf_det* hyp,
                                  const yf_track_info* info, int32_t out_count, int out_cap, double score_iou, int32_t* match,
                                  int32_t* status) {
  int32_t w[YF_SCORE_MAX_ROWS * YF_TRACK_SLOTS];
  const int g = yfi_track_clamp(gt_count, gt_cap), h = yfi_track_clamp(out_count, out_cap);
  int bits = (yfi_track_clipped(gt_count, gt_cap) ? YFI_SCORE_ST_GT_CLIPPED : 0) | (yfi_track_clipped(out_count, out_cap) ? YFI_SCORE_ST_HYP_CLIPPED : 0);
  int row_ok[YF_SCORE_MAX_ROWS], col_ok[YF_TRACK_SLOTS], row_col[YF_SCORE_MAX_ROWS], row_kept[YF_SCORE_MAX_ROWS], col_kept[YF_TRACK_SLOTS];
  int32_t row_w[YF_SCORE_MAX_ROWS];
  uint64_t rows = 0, cols = 0, matches = 0, switches = 0, overlap = 0;
  for (int i = 0; i < g; ++i) {
    row_ok[i] = yfi_score_id_ok(gt[i].id);
    for (int e = 0; e < i; ++e) if (gt[e].id == gt[i].id) row_ok[i] = 0;
    if (!row_ok[i]) bits |= YFI_SCORE_ST_GT_VOID;
    rows += (uint64_t)row_ok[i];
    row_col[i] = -1; row_kept[i] = 0; row_w[i] = 0;
  }
  for (int j = 0; j < YF_TRACK_SLOTS; ++j) {
    col_ok[j] = j < h && info[j].id != 0;
    if (j < h && !col_ok[j]) bits |= YFI_SCORE_ST_HYP_VOID;
    cols += (uint64_t)col_ok[j];
    col_kept[j] = 0;
  }
  for (int i = 0; i < g; ++i) {
    const double area_a = yfi_nms_area(gt[i].x1, gt[i].y1, gt[i].x2, gt[i].y2);
    for (int j = 0; j < YF_TRACK_SLOTS; ++j) {
      int32_t wt = 0;
      if (row_ok[i] && col_ok[j]) {
        double iou;
        const int ok = yfi_track_iou(gt[i].x1, gt[i].y1, gt[i].x2, gt[i].y2, area_a, hyp[j].x1, hyp[j].y1, hyp[j].x2, hyp[j].y2,
                                     yfi_nms_area(hyp[j].x1, hyp[j].y1, hyp[j].x2, hyp[j].y2), score_iou, &iou);
        wt = yfi_assign_weight(ok, iou);
      }
      w[i * YF_TRACK_SLOTS + j] = wt;
    }
  }
  /* continuity */
  for (int i = 0; i < g; ++i) {
    if (!row_ok[i]) continue;
    const uint32_t k = st->last[gt[i].id - 1u];
    if (k == 0) continue;
    int j = 0;
    while (j < h && info[j].id != k) ++j;                             /* the lowest column of that id */
    if (j == h || col_kept[j] || w[i * YF_TRACK_SLOTS + j] <= 0) continue;
    row_kept[i] = 1; col_kept[j] = 1; row_col[i] = j; row_w[i] = w[i * YF_TRACK_SLOTS + j];
  }
  /* the rest */
  int any = 0;
  for (int i = 0; i < g; ++i)
    for (int j = 0; j < YF_TRACK_SLOTS; ++j) {
      if (row_kept[i] || col_kept[j]) w[i * YF_TRACK_SLOTS + j] = 0;
      any |= w[i * YF_TRACK_SLOTS + j] > 0;
    }
  if (any) {
    int slot_det[YF_TRACK_SLOTS], det_slot[YF_TRACK_MAX_DETS];
    yfi_assign_solve(w, g, slot_det, det_slot);
    for (int i = 0; i < g; ++i)
      if (det_slot[i] >= 0) {
        const int j = det_slot[i];
        const uint32_t k = st->last[gt[i].id - 1u];                     /* a matched row has a positive weight: it is not void */
        switches += (uint64_t)(k != 0 && k != info[j].id);
        row_col[i] = j; row_w[i] = w[i * YF_TRACK_SLOTS + j];
      }
  }
  for (int i = 0; i < g; ++i) {
    if (!row_ok[i]) continue;
    const uint32_t o = gt[i].id - 1u;
    st->present[o] = yfi_track_inc(st->present[o]);
    if (row_col[i] < 0) continue;
    st->tracked[o] = yfi_track_inc(st->tracked[o]);
    st->last[o] = info[row_col[i]].id;
    matches += 1u; overlap += (uint64_t)row_w[i];
  }
  st->frames += 1u; st->gt += rows; st->hyp += cols; st->matches += matches; st->misses += rows - matches;
  st->false_positives += cols - matches; st->switches += switches; st->overlap += overlap;
  if (match) for (int i = 0; i < g; ++i) match[i] = row_col[i];
  if (status) *status = bits;
}

/* a call behind its check, on host memory: stream by stream, step by step.  Returns n */
static inline long yfi_score_run(const void* out, const void* info, const void* out_counts, int out_cap, const void* gt, const void* gt_counts,
                                 int gt_cap, long streams, long steps, int layout, double score_iou, void* state, int32_t* match,
                                 int32_t* status) {
  for (long s = 0; s < streams; ++s)
    for (long t = 0; t < steps; ++t) {
      const long f = layout == YF_TRACK_TIME_MAJOR ? t * streams + s : s * steps + t;
      yfi_score_step((yf_score_state*)state + s, (const yf_gt_track*)gt + (size_t)f * (size_t)gt_cap, ((const int32_t*)gt_counts)[f], gt_cap,
                     (const yf_det*)out + (size_t)f * (size_t)out_cap, (const yf_track_info*)info + (size_t)f * (size_t)out_cap,
                     ((const int32_t*)out_counts)[f], out_cap, score_iou, match ? match + (size_t)f * (size_t)gt_cap : NULL,
                     status ? status + f : NULL);
    }
  return streams * steps;
}

/* the summary of `streams` states on host memory; 0, or -1 for a NULL pointer or streams < 0 */
static inline int yfi_score_summary(const void* host_states, long streams, yf_score_summary* out) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  if (!out || streams < 0 || (streams > 0 && !host_states)) return -1;
  yf_score_summary r;
  memset(&r, 0, sizeof r);
  for (long s = 0; s < streams; ++s) {
    yf_score_state st;
    memcpy(&st, (const char*)host_states + (size_t)s * sizeof st, sizeof st);       /* any alignment */
    r.frames += st.frames; r.gt += st.gt; r.hyp += st.hyp; r.matches += st.matches; r.misses += st.misses;
    r.false_positives += st.false_positives; r.switches += st.switches; r.overlap += st.overlap;
    for (int o = 0; o < YF_SCORE_MAX_IDS; ++o) {
      if (st.present[o] <= 0) continue;
      r.objects += 1;
      r.mostly_tracked += 5 * (int64_t)st.tracked[o] >= 4 * (int64_t)st.present[o];
      r.mostly_lost += 5 * (int64_t)st.tracked[o] <= (int64_t)st.present[o];
    }
  }
  const uint64_t errors = r.misses + r.false_positives + r.switches;
  r.mota = 0.0; r.motp = 0.0;
  if (r.gt) { const double q = (double)errors / (double)r.gt; r.mota = 1.0 - q; }
  if (r.matches) { const double q = (double)r.overlap / (double)r.matches; r.motp = q / 1073741824.0; }
  *out = r;
  return 0;
}

/* what the host can see of a call's arguments, in the order the entry points check them; NULL, or the text of the first fault */
static inline const char* yfi_score_check(const void* out, const void* info, const void* out_counts, int out_cap, const void* gt,
                                          const void* gt_counts, int gt_cap, long streams, long steps, int layout, double score_iou,
                                          const void* state, const void* match, const void* status) {
  if (!out || !info || !out_counts || !gt || !gt_counts || !state) return "d_out, d_info, d_out_counts, d_gt, d_gt_counts or d_state is NULL";
  if ((((uintptr_t)out | (uintptr_t)info | (uintptr_t)out_counts | (uintptr_t)gt | (uintptr_t)gt_counts | (uintptr_t)match | (uintptr_t)status) & 3) != 0)
    return "d_out, d_info, d_out_counts, d_gt, d_gt_counts, d_match and d_status must be 4-byte aligned";
  if (((uintptr_t)state & 7) != 0) return "d_state must be 8-byte aligned";
  if (out_cap < 1) return "out_cap must be >= 1";
  if (gt_cap < 1 || gt_cap > YF_SCORE_MAX_ROWS) return "gt_cap must be in [1, 64]";
  if (score_iou != score_iou) return "score_iou is NaN";
  if (layout != YF_TRACK_TIME_MAJOR && layout != YF_TRACK_STREAM_MAJOR) return "layout must be YF_TRACK_TIME_MAJOR or YF_TRACK_STREAM_MAJOR";
  if (streams < 0 || steps < 0) return "streams and steps must be >= 0";
  if (streams > 0 && steps > 2147483646l / streams) return "streams * steps must be in [0, 2^31 - 2]";
  return NULL;
}

#endif
