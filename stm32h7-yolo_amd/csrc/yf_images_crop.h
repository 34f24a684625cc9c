/* Face chips: the region of a detection record in its picture and the chip cut from it (yf_images_crop_records_device,
 * yf_images_crop_records_yuv_device), shared by the device kernels (yf_images_crop.hip.h), the host entries in yf_images.hip and a host
 * build (yf_images_host.c, libyf_images_host.so, which tests/test_crops_host.py checks against ptq.crop_resize_u8).  Plain C.
 *
 * The reference has no such step: its scripts end at cv2.rectangle(img, (x1, y1), (x2, y2), ...) (yoloface/tflite/tflite_prediction.py:64).
 * The region rule, the order of the chips and the status codes are the library's own definition; the resize is the restatement of
 * cv2.resize in yf_images_taps.h, the NV12 / NV21 conversion the one of yf_images_yuv.h.
 *
 * Order: of frame i the first m_i = min(max(count, 0), cap) records count (the suppression's clamp).  first[] is the exclusive prefix of
 * the m_i (first[n] the total); chip k = first[i] + s is slot s of frame i.
 *
 * Region of a record (x1, y1, x2, y2) in a picture of H x W pixels, int64 arithmetic on the int32 edges, which are inclusive (the script
 * draws them so, and the suppression's `+ 1` reads them so):
 *   1. bw = x2 - x1 + 1, bh = y2 - y1 + 1; either < 1: status 1 (YF_DECODE_FW clamps can give x1 > x2).
 *   2. margin, 0 <= margin_permille <= 1000: mx = bw * margin_permille / 1000, my = bh * margin_permille / 1000 (both operands are
 *      non-negative: floor); x1 -= mx, x2 += mx, y1 -= my, y2 += my.
 *   3. with YF_CROP_SQUARE: side = max(x2 - x1 + 1, y2 - y1 + 1); x1 -= (side - (x2 - x1 + 1)) / 2, then x2 = x1 + side - 1; y likewise.
 *   4. clamp: x1 = max(x1, 0), x2 = min(x2, W - 1), y1 = max(y1, 0), y2 = min(y2, H - 1); x1 > x2 or y1 > y2: status 1.
 * The region is NOT squared again after the clamp: a square that overhangs the picture comes back as the rectangle that lies inside it,
 * and the resize stretches that rectangle to the chip.  An INT32_MIN edge of YF_DECODE_PY and a saturated INT32_MAX edge of YF_DECODE_FW
 * simply follow this arithmetic (the largest magnitude, about 2^32 * 1000, is far inside int64).
 *
 * Chip: cv2.resize(P[y1 : y2 + 1, x1 : x2 + 1], (out_w, out_h)), INTER_LINEAR: the taps yfi_axis_tap(d, out, region side) moved by the
 * region's origin, then yfi_hpass / yfi_vpass.  P: the picture's three colour bytes (packed formats) or the converted surface (NV12 /
 * NV21: each of the four sampled pixels converted first, the chroma pair taken by the pixel's ABSOLUTE row and column, (y >> 1,
 * 2 * (x >> 1)), so an odd region origin is right).  The chip's byte order is out_format's, YF_PIX_RGB8 or YF_PIX_BGR8.
 *
 * Status of a chip: 0 a chip; 1 an empty region; 2 the picture's descriptor is invalid (yfi_image_ok / yfi_yuv_image_ok).  The descriptor
 * is checked first: every record of an invalid picture has status 2, whatever its edges.  A chip of status 1 or 2 is all zero bytes, its
 * picture is never read and its info row carries x0 = y0 = width = height = 0. */
#ifndef YF_IMAGES_CROP_H
#define YF_IMAGES_CROP_H
#include <stddef.h>
#include <stdint.h>
#include "../../include/yf_images.h"
#include "yf_images_taps.h"
#include "yf_images_yuv.h"

#define YFI_CROP_MIN_OUT   16
#define YFI_CROP_MAX_OUT   256
#define YFI_CROP_OUT_STEP  16

/* the records of a frame that count: min(max(count, 0), cap) */
YFI_HD int32_t yfi_crop_clamp(int32_t count, int32_t cap) { return count < 0 ? 0 : (count > cap ? cap : count); }

/* THE region rule.  W, H: the picture's sides (1 .. 16384).  Fills x0, y0, width, height of *r and returns the status, 0 or 1 (then the
 * four are 0). */
YFI_HD int yfi_crop_region(int32_t ex1, int32_t ey1, int32_t ex2, int32_t ey2, int32_t W, int32_t H, int margin_permille, int flags,
                           yf_chip* r) {
  int64_t x1 = ex1, y1 = ey1, x2 = ex2, y2 = ey2;
  r->x0 = 0; r->y0 = 0; r->width = 0; r->height = 0;
  const int64_t bw = x2 - x1 + 1, bh = y2 - y1 + 1;
  if (bw < 1 || bh < 1) return 1;
  const int64_t mx = bw * (int64_t)margin_permille / 1000, my = bh * (int64_t)margin_permille / 1000;
  x1 -= mx; x2 += mx; y1 -= my; y2 += my;
  if (flags & YF_CROP_SQUARE) {
    const int64_t w = x2 - x1 + 1, h = y2 - y1 + 1, side = w > h ? w : h;
    x1 -= (side - w) / 2; x2 = x1 + side - 1;
    y1 -= (side - h) / 2; y2 = y1 + side - 1;
  }
  if (x1 < 0) x1 = 0;
  if (y1 < 0) y1 = 0;
  if (x2 > (int64_t)W - 1) x2 = (int64_t)W - 1;
  if (y2 > (int64_t)H - 1) y2 = (int64_t)H - 1;
  if (x1 > x2 || y1 > y2) return 1;
  r->x0 = (int32_t)x1; r->y0 = (int32_t)y1; r->width = (int32_t)(x2 - x1 + 1); r->height = (int32_t)(y2 - y1 + 1);
  return 0;
}

/* the tap of output index d of an axis of the region: yfi_axis_tap over the region's side, moved to the picture's coordinates */
YFI_HD yfi_tap yfi_crop_tap(int d, int n_out, int32_t origin, int32_t side) {
  yfi_tap t = yfi_axis_tap(d, n_out, side);
  t.s0 += origin; t.s1 += origin;
  return t;
}

/* what the host can see of a call's arguments, in the order the entry points check them; NULL, or the text of the first fault */
static inline const char* yfi_crop_check(long n, int cap, int out_h, int out_w, int out_format, int margin_permille, int flags,
                                         long chips_cap) {
  if (n < 0 || n > 2147483646l) return "n must be in [0, 2^31 - 2]";
  if (cap < 1 || cap > YF_IMAGES_NMS_WIDE_MAX_CAP) return "cap must be in [1, 1200]";
  if ((uint64_t)n * (uint64_t)cap >= (1ull << 31)) return "n * cap must be below 2^31";
  if (out_h < YFI_CROP_MIN_OUT || out_h > YFI_CROP_MAX_OUT || out_h % YFI_CROP_OUT_STEP != 0 || out_w < YFI_CROP_MIN_OUT ||
      out_w > YFI_CROP_MAX_OUT || out_w % YFI_CROP_OUT_STEP != 0)
    return "out_h and out_w must be multiples of 16 in [16, 256]";
  if (out_format != YF_PIX_RGB8 && out_format != YF_PIX_BGR8) return "out_format must be YF_PIX_RGB8 or YF_PIX_BGR8";
  if (margin_permille < 0 || margin_permille > 1000) return "margin_permille must be in [0, 1000]";
  if ((flags & ~YF_CROP_SQUARE) != 0) return "flags must be 0 or YF_CROP_SQUARE";
  if (chips_cap < 0) return "chips_cap < 0";
  return NULL;
}

#endif
