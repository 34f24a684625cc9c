/* Optimal assignment of detections to tracks: the tracker with a motion model of yf_images_motion.h with the match of its step 3 replaced
 * by a maximum-weight assignment over the eligible pairs (yf_images_track_motion_assign_device), shared by the device kernel
 * (yf_images_step.hip.h), the host entry in yf_images.hip, a host build (yf_images_host.c, which tests/test_track_assign_host.py checks
 * against ptq.track_assign_match and ptq.track_motion_step(assign="optimal")) and a sanitizer program
 * (tests/csrc/track_assign_sanitize_main.c).  Plain C.
 *
 * EVERYTHING OF yf_images_motion.h STAYS: the state (7176 bytes per stream), predict, update, emit, the layouts, the status bits.  Only
 * the match differs, and only with assign = YF_ASSIGN_OPTIMAL; YF_ASSIGN_GREEDY is that header's match, literally.
 *
 * WHY.  The greedy match takes the eligible pair of the largest IoU again and again.  When two faces pass each other one detection
 * overlaps both tracks; greedy gives it to the track it overlaps most and may strand the other detection: one new id, one track held
 * over.  Tracks A = (0,0,99,99), B = (58,0,157,99), detections d0 = (25,0,124,99), d1 = (-33,0,66,99) at match_iou 0.3: IoU(A,d0) = 0.6,
 * IoU(B,d0) = IoU(A,d1) = 6700/13300, IoU(B,d1) = 900/19100 (not eligible).  Greedy: A-d0, d1 is born, B misses (total 0.6).  Optimal:
 * B-d0 and A-d1 (total 1.008): both identities kept.
 *
 * THE MATCH, with the predicted box of every occupied slot and the first m detections (steps 0-2 of yf_images_motion.h):
 *  - Eligibility and IoU: yfi_track_iou, unchanged.
 *  - Weight: an eligible pair has w = 1 + (int64)(iou * 1073741824.0) (yfi_assign_weight): the product by 2^30 is exact, the conversion
 *    truncates, iou is in (0, 1], so w is in [1, 2^30 + 1].  An ineligible pair, and every pair of a free slot, has w = 0.  From here on
 *    everything is integers: the kernel, the host build and Python agree bit for bit.
 *  - Objective: maximise the sum of w over the matched pairs; a pair of weight 0 is never a match.  That is "maximum total IoU at 2^-30
 *    resolution over the eligible pairs".  IT IS NOT CARDINALITY FIRST: one pair of IoU 0.9 beats two pairs of IoU 0.4 that exclude it.
 *  - THE ALGORITHM IS THE DEFINITION.  The optimum is often not unique, so the ties are settled by one prescribed procedure, the
 *    shortest-augmenting-path method (Kuhn-Munkres in the form of Jonker-Volgenant), yfi_assign_solve below:
 *      rows are the detections 0 .. m-1 in ascending order, columns the 64 slots; cost c[i][j] = (2^30 + 1) - w[i][j] (YFI_ASSIGN_TOP - w);
 *      row potentials u[i], column potentials v[j] are int64 and start at 0; p[j] is the row assigned to column j, -1 at the start.
 *      For row i: minv[j] = INF, way[j] = -1, no column used, the rows visited = {i}; i0 = i, j0 = -1 (none).  Repeat:
 *        1. every unused column j: cur = c[i0][j] - u[i0] - v[j]; if cur < minv[j] (strict): minv[j] = cur, way[j] = j0;
 *        2. delta = the minimum of minv over the unused columns, j1 = THE LOWEST j attaining it;
 *        3. u[r] += delta for every visited row r (row i included); v[j] -= delta for every used column; minv[j] -= delta for every
 *           unused column;
 *        4. j0 = j1.  If p[j0] is -1: stop.  Else column j0 is used, i0 = p[j0], row i0 is visited.
 *      Augment: while j0 is a column: j1 = way[j0]; p[j0] = (j1 a column ? p[j1] : i); j0 = j1.
 *    After the last row, detection p[j] is matched to slot j iff p[j] >= 0 and w[p[j]][j] > 0: a detection assigned to a column of
 *    weight 0 is unmatched.  (Each row ends on a column, since i < 64 columns are assigned when row i starts.)
 *
 * THE BOUND.  With W = 2^30 + 1: 0 <= c <= W, and at every point 0 <= u[i] <= W, -W <= v[j] <= 0, 0 <= cur <= 2 W, 0 <= delta <= 2 W and
 * 0 <= minv[j] <= 2 W for every column that has been relaxed; so every quantity is below 2^32 in magnitude and no signed 64-bit
 * operation can overflow.  The argument, by induction over the repetitions, with F: "u[r] + v[j] <= c[r][j] for every row r <= i that
 * has been started and every column j":
 *  (a) delta >= 0, so u only grows from 0 and v only falls from 0.  F holds at the start of row i: u[i] = 0, v[j] <= 0 <= c.
 *  (b) cur >= 0 by F.  minv[j] of an unused column is the minimum of c[r][j] - u[r] - v[j] over the visited rows r relaxed so far, as of
 *      now: step 3 lowers it by the delta it adds to those u[r], v[j] of an unused column does not change.  So minv >= 0, delta >= 0.
 *  (c) Step 3 keeps F: visited r, used j: u[r] + v[j] unchanged; visited r, unused j: delta <= minv[j] <= c[r][j] - u[r] - v[j];
 *      unvisited r: u[r] unchanged, v[j] not larger.  (A row visited in step 4 is relaxed in the next step 1 before the next step 3.)
 *  (d) A column that is not assigned has never been used, so its v is 0.  While row i is searched such a column j exists (at most i < 64
 *      are assigned), so F gives u[r] <= c[r][j] <= W for every started row, after every step 3.  An assigned pair is tight,
 *      u[p[j]] + v[j] = c[p[j]][j] (the augmenting path runs over tight pairs; (c) keeps used pairs tight), so v[j] >= 0 - W.
 *  (e) cur = c - u - v <= W - 0 + W.
 * The work: row i repeats at most i + 1 times, 64 * 65 / 2 = 2080 repetitions at most per step.
 *
 * TWO SETTINGS.  Gains (256, 0) with YF_ASSIGN_OPTIMAL is "the base tracker with optimal assignment": no entry on the 2824-byte state
 * is added.  Where every detection and every slot has at most one eligible partner the two matches are the same pairs.
 *
 * STILL OUT OF SCOPE.  No covariance.  No appearance features.  No re-identification after a track is removed.  A predicted box is not
 * clamped to the picture.  No identity-switch figure on labelled video stands behind either match.  What exists since: a score of tracks against labelled identities (yf_images_score.h,
 * yf_images_score_tracks_device: misses, false positives, identity switches, MOTA) and its figures on SYNTHETIC clips
 * (profiles/track_score_bench.txt); what still does not: any figure on labelled video.
 * On those clips the optimal assignment WITHOUT the motion model exchanges two faces that pass each other where the greedy match does
 * not; with the motion model neither does. */
#ifndef YF_IMAGES_ASSIGN_H
#define YF_IMAGES_ASSIGN_H
#include "yf_images_motion.h"

#define YFI_ASSIGN_TOP ((1ll << 30) + 1)          /* W: the largest weight; cost = W - weight */
#define YFI_ASSIGN_INF (1ll << 62)                /* minv of a column not yet relaxed */

/* the weight of a pair: ok and iou as yfi_track_iou gave them */
YFI_HD int32_t yfi_assign_weight(int ok, double iou) { return ok ? (int32_t)(1 + (int64_t)(iou * 1073741824.0)) : 0; }

/* THE match on a table of weights: w[i * 64 + j] of detection i < m and slot j -> det_slot[i < m] and slot_det[64] (-1: none); returns
 * the matching's total weight.  The sequential form of the procedure above: only the minimum's tie rule crosses columns. */
static inline int64_t yfi_assign_solve(const int32_t* w, int m, int* slot_det, int* det_slot) {
  int64_t u[YF_TRACK_MAX_DETS], v[YF_TRACK_SLOTS], minv[YF_TRACK_SLOTS];
  int p[YF_TRACK_SLOTS], way[YF_TRACK_SLOTS], used[YF_TRACK_SLOTS], visited[YF_TRACK_MAX_DETS];
  for (int j = 0; j < YF_TRACK_SLOTS; ++j) { v[j] = 0; p[j] = -1; slot_det[j] = -1; }
  for (int i = 0; i < m; ++i) { u[i] = 0; det_slot[i] = -1; }
  for (int i = 0; i < m; ++i) {
    for (int j = 0; j < YF_TRACK_SLOTS; ++j) { minv[j] = YFI_ASSIGN_INF; way[j] = -1; used[j] = 0; }
    for (int r = 0; r < m; ++r) visited[r] = r == i;
    int i0 = i, j0 = -1;
    for (;;) {
      int64_t delta = YFI_ASSIGN_INF;
      int j1 = -1;
      for (int j = 0; j < YF_TRACK_SLOTS; ++j) {
        if (used[j]) continue;
        const int64_t cur = (YFI_ASSIGN_TOP - (int64_t)w[i0 * YF_TRACK_SLOTS + j]) - u[i0] - v[j];
        if (cur < minv[j]) { minv[j] = cur; way[j] = j0; }
        if (minv[j] < delta) { delta = minv[j]; j1 = j; }           /* ascending j and a strict comparison: the lowest column */
      }
      for (int r = 0; r < m; ++r) if (visited[r]) u[r] += delta;
      for (int j = 0; j < YF_TRACK_SLOTS; ++j) { if (used[j]) v[j] -= delta; else minv[j] -= delta; }
      j0 = j1;
      if (p[j0] < 0) break;
      used[j0] = 1; i0 = p[j0]; visited[i0] = 1;
    }
    while (j0 >= 0) { const int j1 = way[j0]; p[j0] = j1 >= 0 ? p[j1] : i; j0 = j1; }
  }
  int64_t total = 0;
  for (int j = 0; j < YF_TRACK_SLOTS; ++j)
    if (p[j] >= 0 && w[p[j] * YF_TRACK_SLOTS + j] > 0) { slot_det[j] = p[j]; det_slot[p[j]] = j; total += w[p[j] * YF_TRACK_SLOTS + j]; }
  return total;
}

/* what the host can see of a call's arguments: yfi_motion_check's faults in its order, then assign; NULL, or the text of the first */
static inline const char* yfi_assign_check(const void* dets, const void* counts, long streams, long steps, int layout, int cap,
                                           const yf_track_motion_params* params, int assign, const void* state, const void* out,
                                           const void* info, const void* out_counts, int out_cap, const void* status) {
  const char* t = yfi_motion_check(dets, counts, streams, steps, layout, cap, params, state, out, info, out_counts, out_cap, status);
  if (t) return t;
  if (assign != YF_ASSIGN_GREEDY && assign != YF_ASSIGN_OPTIMAL) return "assign must be YF_ASSIGN_GREEDY or YF_ASSIGN_OPTIMAL";
  return NULL;
}

#endif
