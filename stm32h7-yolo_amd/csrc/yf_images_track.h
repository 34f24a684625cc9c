/* Tracking: the detection records of the frames of a video stream associated with per-stream track state -- identities and a hold-over
 * (yf_images_track_device), shared by the device kernel (yf_images_step.hip.h), the host entry in yf_images.hip and a host build
 * (yf_images_host.c, libyf_images_host.so, which tests/test_track_host.py checks against ptq.track_step).  Plain C.
 *
 * The reference has no tracker: its detect_video (yoloface/tensorflow/yoloface_test.py:318-385) treats every frame alone.  The
 * definition is the library's own.
 *
 * STATE.  yf_track_state per stream: `issued` (the last id given out), `reserved` (carried, never read) and YF_TRACK_SLOTS slots of
 * yf_track {id, hits, misses, age, det}; id 0 is a free slot.  An all-zero state is the empty state.  The state is untrusted bytes:
 * whatever it holds, a step reads and writes only inside it -- a slot is addressed by its place alone, nothing is indexed by a value
 * read from the state.  A free slot's other bytes are neither read nor written until a track is born there.  Every counter increment
 * saturates at INT32_MAX (yfi_track_inc).
 *
 * ONE STEP: one stream, one frame f with records dets[f][0 .. cap) and counts[f].
 *  1. Detections: the first m = yfi_track_clamp(count, cap) = min(max(count, 0), cap, 64) records, in the order they lie (after the
 *     suppression: descending confidence).  count > min(cap, 64) sets status bit 0 (YFI_TRACK_ST_CLIPPED).
 *  2. IoU of an occupied slot's box and a detection (yfi_track_iou): the suppression's arithmetic -- yfi_nms_area, the + 1 pixel
 *     convention of yoloface_test.py:165-190 -- in float64, one IEEE operation per step, no contraction:
 *       xx1 = max(x1), yy1 = max(y1), xx2 = min(x2), yy2 = min(y2); w = max(0.0, xx2 - xx1 + 1), h likewise; inter = w * h;
 *       uni = (area_a + area_b) - inter; iou = inter / uni
 *     A pair is eligible iff inter > 0.0 and iou >= match_iou.  NO NaN ARISES: inter > 0 means min(x2) >= max(x1) and min(y2) >=
 *     max(y1), so both boxes are proper (x2 >= x1, y2 >= y1); w <= each box's width and h <= each box's height, the edge differences
 *     are exact in double and rounding is monotone, so inter <= area_a and inter <= area_b as rounded; then area_a + area_b rounds to
 *     at least 2 * inter and uni >= inter > 0.  The quotient is a positive double in (0, 1], which orders as its bits do.  Empty and
 *     inverted boxes (and int32 extremes that make them so) are never eligible: they are born, never matched, and age out.
 *  3. Match, global greedy: repeatedly the eligible pair of the largest IoU among the slots and detections still unmatched; ties go to
 *     the lower detection index, then the lower slot; until no pair is left.
 *  4. Update, in this order.  A matched slot: det = the detection (all 28 bytes), hits + 1, misses = 0, age + 1.  An unmatched occupied
 *     slot: misses + 1, age + 1; if then misses > max_misses the whole slot is zeroed (the bytes stay canonical).  The unmatched
 *     detections in ascending index each take the lowest free slot, slots freed in this step included: id = ++issued (0 is skipped
 *     when it wraps: yfi_track_next_id), hits = 1, misses = 0, age = 1.  With no free slot the detection is dropped and status bit 1
 *     (YFI_TRACK_ST_DROPPED) is set; a dropped detection takes no id.
 *  5. Emit: every slot with id != 0 and hits >= min_hits, in ascending id (unsigned; equal ids, which only a crafted state has, in
 *     ascending slot): the slot's det with its `frame` field set to f, beside its yf_track_info {id, hits, misses, age}.  A held-over
 *     track (misses > 0) is emitted with its last box.  out_counts[f] is the true number; only the first out_cap are written, and the
 *     places beyond min(count, out_cap) are not touched.  status[f] (if given) is written: 0 or the bits above.
 *
 * A CALL: n = streams * steps frames; YF_TRACK_TIME_MAJOR: f = t * streams + s; YF_TRACK_STREAM_MAJOR: f = s * steps + t.  The steps of
 * stream s are taken in order t = 0 .. steps - 1 on state[s], which is read before the first and written after the last.
 *
 * OUT OF SCOPE.  No motion model HERE: a held-over box stays where it was last seen; the entry beside this one, yf_images_motion.h
 * (yf_images_track_motion_device), adds a constant-velocity filter per edge.  No appearance features.  No re-identification after a
 * track is removed: the face gets a new id.  No optimal assignment HERE: the match is the greedy one above; yf_images_assign.h
 * (yf_images_track_motion_assign_device) puts a maximum-weight assignment in its place, on the motion entry's state. */
#ifndef YF_IMAGES_TRACK_H
#define YF_IMAGES_TRACK_H
#include <stddef.h>
#include <stdint.h>
#include "../../include/yf_images.h"
#include "yf_images_nms.h"

/* YF_TRACK_SLOTS 64 (include/yf_images.h): one lane of a wave per slot */
#define YF_TRACK_MAX_DETS 64
#define YFI_TRACK_ST_CLIPPED 1      /* status bit 0: count above min(cap, 64) */
#define YFI_TRACK_ST_DROPPED 2      /* status bit 1: a detection found no free slot */
#define YFI_TRACK_STATE_WORDS 706   /* sizeof(yf_track_state) / 4 */
#define YFI_TRACK_SLOT_WORDS 11     /* sizeof(yf_track) / 4 */

#ifdef __cplusplus
static_assert(sizeof(yf_det) == 28 && sizeof(yf_track) == 4 * YFI_TRACK_SLOT_WORDS && sizeof(yf_track_info) == 16 &&
              sizeof(yf_track_state) == 4 * YFI_TRACK_STATE_WORDS && sizeof(yf_track_state) == 8 + YF_TRACK_SLOTS * sizeof(yf_track),
              "the layout include/yf_images.h states");
#else
_Static_assert(sizeof(yf_det) == 28 && sizeof(yf_track) == 4 * YFI_TRACK_SLOT_WORDS && sizeof(yf_track_info) == 16 &&
               sizeof(yf_track_state) == 4 * YFI_TRACK_STATE_WORDS && sizeof(yf_track_state) == 8 + YF_TRACK_SLOTS * sizeof(yf_track),
               "the layout include/yf_images.h states");
#endif

/* the detections of a frame that count */
YFI_HD int yfi_track_clamp(int32_t count, int cap) {
  const int lim = cap < YF_TRACK_MAX_DETS ? cap : YF_TRACK_MAX_DETS;
  return count < 0 ? 0 : (count > lim ? lim : count);
}

YFI_HD int yfi_track_clipped(int32_t count, int cap) { return count > (cap < YF_TRACK_MAX_DETS ? cap : YF_TRACK_MAX_DETS); }

/* THE increment */
YFI_HD int32_t yfi_track_inc(int32_t v) { return v == INT32_MAX ? v : v + 1; }

/* the id of the k-th track (k = 0, 1, ... < 64) born after `issued`: ++issued k + 1 times, 0 skipped */
YFI_HD uint32_t yfi_track_next_id(uint32_t issued, int k) {
  const uint64_t t = (uint64_t)issued + (uint64_t)k + 1u;
  return (uint32_t)(t > 0xFFFFFFFFull ? t + 1u : t);
}

/* 1 if the slot's box a and the detection b are eligible at match_iou, with the IoU in *iou; 0 (and *iou = 0.0) if not */
YFI_HD int yfi_track_iou(int32_t ax1, int32_t ay1, int32_t ax2, int32_t ay2, double area_a, int32_t bx1, int32_t by1, int32_t bx2,
                         int32_t by2, double area_b, double match_iou, double* iou) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double xx1 = (double)(ax1 > bx1 ? ax1 : bx1), yy1 = (double)(ay1 > by1 ? ay1 : by1);
  const double xx2 = (double)(ax2 < bx2 ? ax2 : bx2), yy2 = (double)(ay2 < by2 ? ay2 : by2);
  const double wv = xx2 - xx1 + 1.0, hv = yy2 - yy1 + 1.0;
  const double w = wv > 0.0 ? wv : 0.0, h = hv > 0.0 ? hv : 0.0;
  const double inter = w * h;
  *iou = 0.0;
  if (!(inter > 0.0)) return 0;
  const double uni = (area_a + area_b) - inter;
  const double q = inter / uni;
  if (!(q >= match_iou)) return 0;
  *iou = q;
  return 1;
}

/* what the host can see of a call's arguments, in the order the entry points check them; NULL, or the text of the first fault */
static inline const char* yfi_track_check(const void* dets, const void* counts, long streams, long steps, int layout, int cap,
                                          const yf_track_params* params, const void* state, const void* out, const void* info,
                                          const void* out_counts, int out_cap, const void* status) {
  if (streams < 0 || steps < 0) return "streams and steps must be >= 0";
  if (streams > 0 && steps > 2147483646l / streams) return "streams * steps must be in [0, 2^31 - 2]";
  if (layout != YF_TRACK_TIME_MAJOR && layout != YF_TRACK_STREAM_MAJOR) return "layout must be YF_TRACK_TIME_MAJOR or YF_TRACK_STREAM_MAJOR";
  if (cap < 1 || cap > YF_IMAGES_NMS_WIDE_MAX_CAP) return "cap must be in [1, 1200]";
  if (out_cap < 1) return "out_cap must be >= 1";
  if (!params) return "params is NULL";
  if (params->match_iou != params->match_iou) return "match_iou is NaN";
  if (params->min_hits < 1) return "min_hits must be >= 1";
  if (params->max_misses < 0) return "max_misses must be >= 0";
  if (!dets || !counts || !state || !out || !info || !out_counts) return "d_dets, d_counts, d_state, d_out, d_info or d_out_counts is NULL";
  if ((((uintptr_t)dets | (uintptr_t)counts | (uintptr_t)out | (uintptr_t)info | (uintptr_t)out_counts | (uintptr_t)status) & 3) != 0)
    return "d_dets, d_counts, d_out, d_info, d_out_counts and d_status must be 4-byte aligned";
  if (((uintptr_t)state & 7) != 0) return "d_state must be 8-byte aligned";
  return NULL;
}

#endif
