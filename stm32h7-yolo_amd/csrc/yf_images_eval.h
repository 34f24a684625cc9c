/* The arithmetic of scoring detection records against ground-truth boxes (yf_images_match_device, yf_images_average_precision_device),
 * shared by the device kernels (yf_images_eval.hip.h) and a host build (yf_images_host.c, libyf_images_host.so, which
 * tests/test_eval_host.py checks against a plain-Python restatement).  Restated from calculate_iou / calculate_ap / calculate_map,
 * yoloface/tensorflow/yolov3_train_tf.py:657-759, where a detection is [x1, y1, x2, y2] with the record's int32 edges and a ground truth
 * is four floats:
 *   x1 = max(d.x1, g.x1), y1 = max(d.y1, g.y1), x2 = min(d.x2, g.x2), y2 = min(d.y2, g.y2)
 *   inter = max(0, x2 - x1) * max(0, y2 - y1)                       -- NOT the suppression's formula: there is no + 1
 *   area1 = (d.x2 - d.x1) * (d.y2 - d.y1), area2 = (g.x2 - g.x1) * (g.y2 - g.y1), union = (area1 + area2) - inter
 *   iou = inter / union if union > 0 else 0.0
 * One IEEE double operation per Python operation, in that order.  Python's max(a, b) is "a unless b > a" and min(a, b) "a unless b < a":
 * they are written as exactly those ternaries, so NaN and infinity in a ground-truth row behave as they do in Python.  The int32 edges
 * convert exactly; where Python multiplies two ints exactly and rounds when the product meets a float, the double product rounds to the
 * same value.  Compile without FMA contraction (-ffp-contract=off; the pragma says so again for clang).
 *
 * Match, per detection (:727-746): best_iou = 0, best = -1; over the frame's ground truths in order a strictly larger IoU replaces, so an
 * IoU of 0 never matches and among equal best IoUs the first ground truth wins.  The detection is a candidate iff best_iou >= thr and
 * best >= 0.  Claim: detections are visited in the order below; a candidate whose (frame, best) is unclaimed claims it and is a true
 * positive, every other detection is a false positive -- also a candidate whose best ground truth was claimed before (no second choice).
 *
 * Order (:712-713, a list.sort(..., reverse=True), which is stable): descending conf (the float32 of the record), ties EARLIER record
 * first (lower frame, then lower slot) -- the opposite of the suppression's tie rule (yf_images_nms.h: later record first).  -0.0 ties with
 * +0.0.  "By confidence" is the reference's comment and its purpose; its key as written, x[4] of a tuple with the image id in front, reads
 * the box's y2.  The library orders by confidence -- its choice, equal to the reference wherever the confidences order as the y2 do.
 * A NaN confidence never comes out of a decode and Python's sort is not defined for it; the library's choice: NaN sorts after every
 * number.  A smaller key is earlier.
 *
 * Curve and AP (:748-759, :683-694) over the m detections in that order: ctp, cfp cumulative counts (as doubles: numpy's cumsum of float64),
 *   precision[i] = ctp / ((ctp + cfp) + 1e-16), recall[i] = ctp / max(1, num_gt), precision[i] = max(precision[i], precision[i + 1]) from
 *   the back, ap = sum over i = 1 .. m - 1, in that order, of (recall[i] - recall[i - 1]) * precision[i].  The term of i = 0 is missing in
 * the reference and stays missing.  A term is exactly +0.0 where detection i is a false positive (the recalls are equal), and x + 0.0 = x:
 * the sum over the true positives alone, in order, has the same bits. */
#ifndef YF_IMAGES_EVAL_H
#define YF_IMAGES_EVAL_H
#include <stdint.h>
#ifndef YFI_HD
#ifdef __HIPCC__
#define YFI_HD __host__ __device__ __forceinline__
#else
#define YFI_HD static inline
#endif
#endif

/* the records (or ground truths) of a frame that count: min(max(count, 0), cap) */
YFI_HD int yfi_eval_clamp(int count, int cap) { return count < 0 ? 0 : (count > cap ? cap : count); }

/* calculate_iou(detection, ground truth) */
YFI_HD double yfi_eval_iou(int32_t dx1, int32_t dy1, int32_t dx2, int32_t dy2, double gx1, double gy1, double gx2, double gy2) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double ax1 = (double)dx1, ay1 = (double)dy1, ax2 = (double)dx2, ay2 = (double)dy2;
  const double x1 = gx1 > ax1 ? gx1 : ax1, y1 = gy1 > ay1 ? gy1 : ay1;         /* max(a, b): a unless b > a */
  const double x2 = gx2 < ax2 ? gx2 : ax2, y2 = gy2 < ay2 ? gy2 : ay2;         /* min(a, b): a unless b < a */
  const double wv = x2 - x1, hv = y2 - y1;
  const double w = wv > 0.0 ? wv : 0.0, h = hv > 0.0 ? hv : 0.0;               /* max(0, v): 0 unless v > 0 */
  const double inter = w * h;
  const double area1 = (ax2 - ax1) * (ay2 - ay1), area2 = (gx2 - gx1) * (gy2 - gy1);
  const double uni = (area1 + area2) - inter;
  return uni > 0.0 ? inter / uni : 0.0;
}

/* The order of the detections as an unsigned key, smaller is earlier: descending conf, -0 as +0, every NaN last.  Equal keys keep their
 * input order (a stable sort; the input position ascends with frame, then slot). */
YFI_HD uint32_t yfi_eval_key(uint32_t conf_bits) {
  uint32_t u = conf_bits;
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0xFFFFFFFFu;       /* NaN: after every number (the library's choice) */
  if (u == 0x80000000u) u = 0u;                                 /* -0 == +0 */
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);               /* ascending with the value */
  return ~u;                                                    /* +inf -> 0x007FFFFF ... -inf -> 0xFF800000 */
}

/* ... and inside one frame, where the global order is the frame's own: the key above over an 11-bit slot.  The candidate with the smallest
 * claim key among those that share a best ground truth is the one that claims it.  Slot < 2048. */
YFI_HD uint64_t yfi_eval_claim_key(uint32_t conf_bits, uint32_t slot) { return ((uint64_t)yfi_eval_key(conf_bits) << 11) | (uint64_t)slot; }

/* precision and recall after ctp true and cfp false positives (counts as doubles, as numpy's cumsum of a float64 array gives them) */
YFI_HD double yfi_eval_precision(double ctp, double cfp) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  return ctp / ((ctp + cfp) + 1e-16);
}

YFI_HD double yfi_eval_recall(double ctp, int64_t num_gt) { return ctp / (double)(num_gt > 1 ? num_gt : 1); }

/* the term of a true positive at position i >= 1 that is the ctp-th one: (recall[i] - recall[i - 1]) * precision[i], precision[i] the
 * envelope's value */
YFI_HD double yfi_eval_term(double ctp, int64_t num_gt, double envelope) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  return (yfi_eval_recall(ctp, num_gt) - yfi_eval_recall(ctp - 1.0, num_gt)) * envelope;
}

#endif
