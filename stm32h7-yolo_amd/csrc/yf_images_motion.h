/* Tracking with a motion model: the tracker of yf_images_track.h with a constant-velocity g-h (alpha-beta) filter on every edge of a
 * track's box, so that a held-over box moves on with its face (yf_images_track_motion_device), shared by the device kernel
 * (yf_images_step.hip.h), the host entry in yf_images.hip, a host build (yf_images_host.c, which tests/test_track_motion_host.py checks
 * against ptq.track_motion_step) and a sanitizer program (tests/csrc/track_motion_sanitize_main.c).  Plain C.
 *
 * The reference has no tracker; the definition is the library's own.  The filter is in integers -- no float takes part in it --, so the
 * kernel, the host build and Python agree bit for bit; the match itself stays the float64 IoU of yfi_track_iou.
 *
 * STATE.  yf_track_motion_state per stream: `issued`, `reserved` and YF_TRACK_SLOTS slots of yf_track_motion {base, pad, pos[4], vel[4]}:
 * `base` is the base tracker's slot, pos and vel the filter's position and velocity of the edges x1, y1, x2, y2 in 1/256 pixel and
 * 1/256 pixel per step.  A slot is 112 bytes, the state 7176, 8-byte aligned.  An all-zero state is the empty state.  The bytes are
 * untrusted as the base tracker's are: a slot is addressed by its place alone, and a free slot's other bytes are neither read nor written
 * until a track is born there.  Every pos and vel read from the state first goes through yfi_motion_sat, the clamp to [-2^40, 2^40]: then
 * |pos + vel| <= 2^41, |256 z - (pos + vel)| < 2^42 for an int32 edge z, a gain times that < 2^51, and no signed 64-bit operation
 * below can overflow whatever the bytes hold.  `pad` is carried and never read; it is written 0 at birth and at removal.
 *
 * PARAMETERS.  yf_track_motion_params {base, alpha, beta, damp, smooth}: base the base tracker's; alpha, beta, damp in [0, 256], gains in
 * units of 1/256; smooth 0 or 1.
 *   yfi_motion_mul(g, v) = v >= 0 ? (g v) >> 8 : -((g (-v)) >> 8): a gain applied, symmetric, truncating toward zero.
 *   yfi_motion_box(p)    = clamp(floor((p + 128) / 256), INT32_MIN, INT32_MAX): the pixel nearest to a position, halves up.
 *
 * ONE STEP: the steps 1-5 of yf_images_track.h, with these differences.
 *  0. Predict.  Every occupied slot: P' = pos + vel per edge; its box for the match is yfi_motion_box(P'), its area yfi_nms_area of those
 *     integers.  An inverted predicted box is never eligible, exactly as an inverted stored box is not in the base tracker.
 *  1-3. The match: the base tracker's -- the first m records, yfi_track_iou, the global greedy, its ties and its eligibility, literally --
 *     with the predicted box in the place of the slot's last record.
 *  4. Update.  A matched slot: base.det = the detection (all 28 bytes), the counters as in the base tracker; per edge, z the detection's
 *     edge, r = 256 z - P': pos = sat(P' + mul(alpha, r)), vel = sat(vel + mul(beta, r)).  An unmatched occupied slot: the counters as
 *     in the base tracker; pos = sat(P'), vel = mul(damp, vel); a removed slot is zeroed whole, all 112 bytes.  A birth: as in the base
 *     tracker, and pos = 256 z, vel = 0, pad = 0.
 *  5. Emit: the same tracks in the same order beside the same yf_track_info.  The record is the slot's base.det with `frame` set to f; its
 *     four edges are replaced by yfi_motion_box(pos) -- pos after the update -- if misses > 0 (a held-over track: this is the box that
 *     moved on) or if smooth is 1; with smooth 0 a track matched or born in this step emits its detection verbatim.  (A new track's pos is
 *     256 z: its smoothed box is its detection.)
 *
 * A CALL: as in yf_images_track.h, both layouts; state[s] is read before the first step of stream s and written after the last.
 *
 * TWO SETTINGS.  (alpha, beta) = (256, 0) is the base tracker: from the empty state vel stays 0 and pos stays 256 * the last box, so
 * every output byte equals yf_images_track_device's for any damp and either smooth (and every slot's `base` equals the base tracker's
 * slot).  (256, 256) predicts with the last frame-to-frame difference: pos = 256 z, vel = 256 * (z - the previous z) while matched.
 * The library's suggestion is YFI_MOTION_ALPHA, YFI_MOTION_BETA, YFI_MOTION_DAMP, smooth 0 = (192, 128, 256, 0): a choice, not a
 * measurement -- no accuracy or identity-switch figure on real video stands behind it.  What exists since: a score of tracks against labelled identities (yf_images_score.h,
 * yf_images_score_tracks_device: misses, false positives, identity switches, MOTA) and its figures on SYNTHETIC clips
 * (profiles/track_score_bench.txt); what still does not: any figure on labelled video.
 *
 * STILL OUT OF SCOPE.  No covariance (this is not a Kalman filter: the gains are fixed).  No appearance features.  No re-identification
 * after a track is removed.  No optimal assignment HERE: the match is the greedy one; the entry beside this one, yf_images_assign.h
 * (yf_images_track_motion_assign_device), puts a maximum-weight assignment in its place.  A predicted box is not clamped to the
 * picture: it may leave it; the crop, the redaction, the blur and the drawing clip to the picture themselves. */
#ifndef YF_IMAGES_MOTION_H
#define YF_IMAGES_MOTION_H
#include "yf_images_track.h"

#define YFI_MOTION_ONE 256                       /* the unit of the gains and of pos and vel */
#define YFI_MOTION_LIMIT (1ll << 40)             /* |pos|, |vel| <= this */
#define YFI_MOTION_ALPHA 192                     /* the suggested gains: a choice, not a measurement */
#define YFI_MOTION_BETA 128
#define YFI_MOTION_DAMP 256
#define YFI_MOTION_STATE_WORDS 1794              /* sizeof(yf_track_motion_state) / 4 */
#define YFI_MOTION_SLOT_WORDS 28                 /* sizeof(yf_track_motion) / 4 */

#ifdef __cplusplus
static_assert(sizeof(yf_track_motion) == 4 * YFI_MOTION_SLOT_WORDS && sizeof(yf_track_motion) == 112 &&
              sizeof(yf_track_motion_state) == 4 * YFI_MOTION_STATE_WORDS && sizeof(yf_track_motion_state) == 7176 &&
              sizeof(yf_track_motion_state) == 8 + YF_TRACK_SLOTS * sizeof(yf_track_motion) && sizeof(yf_track_motion_params) == 32,
              "the layout include/yf_images.h states");
#else
_Static_assert(sizeof(yf_track_motion) == 4 * YFI_MOTION_SLOT_WORDS && sizeof(yf_track_motion) == 112 &&
               sizeof(yf_track_motion_state) == 4 * YFI_MOTION_STATE_WORDS && sizeof(yf_track_motion_state) == 7176 &&
               sizeof(yf_track_motion_state) == 8 + YF_TRACK_SLOTS * sizeof(yf_track_motion) && sizeof(yf_track_motion_params) == 32,
               "the layout include/yf_images.h states");
#endif

/* THE clamp of a position or a velocity */
YFI_HD int64_t yfi_motion_sat(int64_t v) { return v < -YFI_MOTION_LIMIT ? -YFI_MOTION_LIMIT : (v > YFI_MOTION_LIMIT ? YFI_MOTION_LIMIT : v); }

/* a gain g in [0, 256] applied to v, |v| < 2^55: toward zero, mul(g, -v) == -mul(g, v) */
YFI_HD int64_t yfi_motion_mul(int32_t g, int64_t v) { return v >= 0 ? (int64_t)(((uint64_t)g * (uint64_t)v) >> 8) : -(int64_t)(((uint64_t)g * (uint64_t)(-v)) >> 8); }

/* the pixel of a position p, |p| < 2^62: floor((p + 128) / 256), clamped to int32 */
YFI_HD int32_t yfi_motion_box(int64_t p) {
  const int64_t q = p + 128;
  const int64_t f = q >= 0 ? q / 256 : -((255 - q) / 256);
  return f < INT32_MIN ? INT32_MIN : (f > INT32_MAX ? INT32_MAX : (int32_t)f);
}

/* what the host can see of a call's arguments: yfi_track_check's faults in its order, then the gains; NULL, or the text of the first */
static inline const char* yfi_motion_check(const void* dets, const void* counts, long streams, long steps, int layout, int cap,
                                           const yf_track_motion_params* params, const void* state, const void* out, const void* info,
                                           const void* out_counts, int out_cap, const void* status) {
  const char* t = yfi_track_check(dets, counts, streams, steps, layout, cap, params ? &params->base : NULL, state, out, info, out_counts,
                                  out_cap, status);
  if (t) return t;
  if (params->alpha < 0 || params->alpha > YFI_MOTION_ONE) return "alpha must be in [0, 256]";
  if (params->beta < 0 || params->beta > YFI_MOTION_ONE) return "beta must be in [0, 256]";
  if (params->damp < 0 || params->damp > YFI_MOTION_ONE) return "damp must be in [0, 256]";
  if (params->smooth != 0 && params->smooth != 1) return "smooth must be 0 or 1";
  return NULL;
}

#endif
