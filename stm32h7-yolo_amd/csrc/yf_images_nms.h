/* The pairwise decision of the greedy IoU suppression of decoded records (yf_images_nms_device), shared by the device kernel
 * (yf_images.hip) and a host build (yf_images_host.c, libyf_images_host.so, which tests/test_nms_host.py checks against numpy's float64
 * arithmetic).  Restated from YoloFaceDetector.non_max_suppression, yoloface/tensorflow/yoloface_test.py:165-190, where the boxes are a
 * float64 array [x1, y1, x2, y2, conf] and i is the survivor:
 *   area = (x2 - x1 + 1) * (y2 - y1 + 1)
 *   xx1 = max(x1[i], x1[j]), yy1 = max(y1[i], y1[j]), xx2 = min(x2[i], x2[j]), yy2 = min(y2[i], y2[j])
 *   w = max(0.0, xx2 - xx1 + 1), h = max(0.0, yy2 - yy1 + 1), inter = w * h, union = (area[i] + area[j]) - inter
 *   j survives i iff inter / union <= thr
 * One IEEE double operation per numpy operation, in that order.  The int32 edges convert exactly; the products can exceed 2^53 and round
 * as numpy's do; a union <= 0 follows IEEE (0 / 0 = NaN, and NaN <= thr is false: suppressed).  Compile without FMA contraction
 * (-ffp-contract=off; the pragma below says so again for clang): a fused (area[i] + area[j]) - w * h rounds once instead of twice. */
#ifndef YF_IMAGES_NMS_H
#define YF_IMAGES_NMS_H
#include <stdint.h>
#ifndef YFI_HD
#ifdef __HIPCC__
#define YFI_HD __host__ __device__ __forceinline__
#else
#define YFI_HD static inline
#endif
#endif

/* area of a box with int32 edges, the reference's (x2 - x1 + 1) * (y2 - y1 + 1) in double */
YFI_HD double yfi_nms_area(int32_t x1, int32_t y1, int32_t x2, int32_t y2) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  return ((double)x2 - (double)x1 + 1.0) * ((double)y2 - (double)y1 + 1.0);
}

/* 1 if box j (edges b, area area_b) survives the kept box i (edges a, area area_a) at threshold thr, 0 if it is suppressed */
YFI_HD int yfi_nms_survives(int32_t ax1, int32_t ay1, int32_t ax2, int32_t ay2, double area_a,
                            int32_t bx1, int32_t by1, int32_t bx2, int32_t by2, double area_b, double thr) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double xx1 = (double)(ax1 > bx1 ? ax1 : bx1), yy1 = (double)(ay1 > by1 ? ay1 : by1);
  const double xx2 = (double)(ax2 < bx2 ? ax2 : bx2), yy2 = (double)(ay2 < by2 ? ay2 : by2);
  const double wv = xx2 - xx1 + 1.0, hv = yy2 - yy1 + 1.0;
  const double w = wv > 0.0 ? wv : 0.0, h = hv > 0.0 ? hv : 0.0;
  const double inter = w * h;
  const double uni = (area_a + area_b) - inter;
  if (inter == 0.0) return uni != 0.0 && 0.0 <= thr;         /* 0 / uni without the division: +-0, or NaN when uni is 0 */
  return inter / uni <= thr;
}

/* The order of the records: descending conf, ties later record first (np.argsort(conf, kind="stable")[::-1]).  A larger key is earlier.
 * conf's bits are mapped to an unsigned order (-0 as +0, every NaN above +inf, where numpy's ascending sort puts NaN: last), the record
 * index below them makes every key unique.  Index < 256. */
YFI_HD uint64_t yfi_nms_key(uint32_t conf_bits, uint32_t index) {
  uint32_t u = conf_bits;
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) u = 0xFFFFFFFFu;         /* NaN */
  else {
    if (u == 0x80000000u) u = 0u;                              /* -0 == +0 */
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  }
  return ((uint64_t)u << 8) | (uint64_t)index;
}

/* The same order for yf_images_nms_wide_device (up to 1200 records per frame): the same mapping of conf's bits above an 11-bit record
 * index.  Index < 2048. */
YFI_HD uint64_t yfi_nms_key_wide(uint32_t conf_bits, uint32_t index) {
  return ((yfi_nms_key(conf_bits, 0u) >> 8) << 11) | (uint64_t)index;
}

#endif
