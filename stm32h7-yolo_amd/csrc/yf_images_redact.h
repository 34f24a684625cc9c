/* Redaction: every detection record's region of its picture pixelated (block mosaic) or filled with one colour, in place, in the picture
 * where it lies (yf_images_redact_records_device, yf_images_redact_records_yuv_device), shared by the device kernels
 * (yf_images_redact.hip.h), the host entries in yf_images.hip and a host build (yf_images_host.c, libyf_images_host.so, which
 * tests/test_redact_host.py checks against ptq.redact_u8 and ptq.redact_yuv420sp).  Plain C.
 *
 * The reference has no such step: its scripts end by drawing into the picture (cv2.rectangle, yoloface/tflite/tflite_prediction.py:64).
 * The definition is the library's own.
 *
 * Records: of frame i the first m_i = yfi_crop_clamp(count, cap) records count.  Region of a record: yfi_crop_region of yf_images_crop.h
 * (margin in permille, optional YF_CROP_SQUARE, clamp to the picture); a record of status 1 (no region) is skipped.  Picture of frame i:
 * descriptor i, checked with yfi_image_ok / yfi_yuv_image_ok; an invalid one gives status[i] = 1 and is neither read nor written, a valid
 * one status[i] = 0.
 *
 * YF_REDACT_MOSAIC, block = k in {4, 8, 16, 32, 64}.  The block grid is anchored at picture pixel (0, 0): block (bx, by) holds columns
 * [bx * k, min(bx * k + k, W) - 1] and rows [by * k, min(by * k + k, H) - 1] (clipped at the right and bottom edge; cnt pixels).  A
 * region touches the blocks bx in [x0 / k, (x0 + width - 1) / k], by likewise (yfi_redact_blocks).  The redacted set of a picture is the
 * UNION of the blocks its records touch.  Every block of the set, every colour byte channel: v = (sum + cnt / 2) / cnt
 * (yfi_redact_mean), the sum over the block's pixels as they were before the call (at most 64 * 64 * 255); every pixel of the block gets
 * v.  The fourth byte of BGRA / RGBA is neither read nor written; nothing outside the set is written.  NV12 / NV21: the luma blocks on
 * the Y plane, and per block of the set the chroma block of the same (bx, by): pairs cx in [bx * k / 2, min(bx * k / 2 + k / 2, W / 2)
 * - 1], rows cy likewise over H / 2 (yfi_redact_chroma_span); the first bytes of the pairs are averaged together and the second bytes
 * together, so the mosaic does not care which of U and V comes first.  The result does not depend on the order of a frame's records,
 * and a second call changes nothing (the mean of a constant block is that constant).
 *
 * YF_REDACT_FILL, block = 0, colour = 0x00RRGGBB (a non-zero top byte is refused).  Every pixel of every region -- the exact region, not
 * grown to a grid -- gets R, G, B in the bytes where the picture's format keeps them (yfi_redact_fill_bytes); alpha is untouched.
 * NV12 / NV21: colour = 0x00YYUUVV; the region's Y bytes, and the chroma pairs cx in [x0 >> 1, (x0 + width - 1) >> 1], cy in [y0 >> 1,
 * (y0 + height - 1) >> 1]: (U, V) for NV12, (V, U) for NV21.
 *
 * ALIASING.  Mosaic: the pictures of different frames must not share bytes.  The call cannot check this; a caller who breaks it gets
 * unspecified picture contents, but never an access outside a picture's extent as its descriptor states it.  Fill: pictures may be
 * shared, because all writers write the same bytes. */
#ifndef YF_IMAGES_REDACT_H
#define YF_IMAGES_REDACT_H
#include <stddef.h>
#include <stdint.h>
#include "../../include/yf_images.h"
#include "yf_images_crop.h"

#define YFI_REDACT_MAX_BLOCK 64

/* the blocks a region touches, inclusive on both ends; with k >= 4 and sides up to 16384 an index is at most 4095 */
typedef struct yfi_blocks { int32_t bx0, by0, bx1, by1; } yfi_blocks;

YFI_HD yfi_blocks yfi_redact_blocks(const yf_chip* r, int k) {
  yfi_blocks b;
  b.bx0 = r->x0 / k; b.bx1 = (r->x0 + r->width - 1) / k;
  b.by0 = r->y0 / k; b.by1 = (r->y0 + r->height - 1) / k;
  return b;
}

/* block index b of an axis of `side` pixels: its first pixel and the number it really holds */
YFI_HD void yfi_redact_span(int32_t b, int k, int32_t side, int32_t* at, int32_t* len) {
  *at = b * k;
  *len = side - *at < k ? side - *at : k;
}

/* ... and of the chroma plane of a surface (side: W or H of the surface, even): its first pair (or row) and how many */
YFI_HD void yfi_redact_chroma_span(int32_t b, int k, int32_t side, int32_t* at, int32_t* len) {
  *at = b * (k / 2);
  *len = side / 2 - *at < k / 2 ? side / 2 - *at : k / 2;
}

/* THE mean */
YFI_HD uint32_t yfi_redact_mean(uint32_t sum, uint32_t cnt) { return (sum + cnt / 2) / cnt; }

/* the three bytes the fill writes, in the order the format keeps them in memory (NV12 / NV21: out[0] the Y byte, out[1], out[2] the
 * chroma pair in memory order) */
YFI_HD void yfi_redact_fill_bytes(uint32_t colour, int format, uint8_t out[3]) {
  const uint8_t a = (uint8_t)(colour >> 16), b = (uint8_t)(colour >> 8), c = (uint8_t)colour;
  const int rev = format == YF_PIX_BGR8 || format == YF_PIX_BGRA8;
  out[0] = rev ? c : a; out[1] = b; out[2] = rev ? a : c;
  if (format == YF_PIX_NV21) { out[1] = c; out[2] = b; }
}

/* what the host can see of a call's arguments, in the order the entry points check them; NULL, or the text of the first fault */
static inline const char* yfi_redact_check(long n, int cap, int mode, int block, uint32_t colour, int margin_permille, int flags) {
  if (n < 0 || n > 2147483646l) return "n must be in [0, 2^31 - 2]";
  if (cap < 1 || cap > YF_IMAGES_NMS_WIDE_MAX_CAP) return "cap must be in [1, 1200]";
  if ((uint64_t)n * (uint64_t)cap >= (1ull << 31)) return "n * cap must be below 2^31";
  if (mode != YF_REDACT_MOSAIC && mode != YF_REDACT_FILL) return "mode must be YF_REDACT_MOSAIC or YF_REDACT_FILL";
  if (mode == YF_REDACT_MOSAIC && block != 4 && block != 8 && block != 16 && block != 32 && block != 64)
    return "block must be 4, 8, 16, 32 or 64 in YF_REDACT_MOSAIC";
  if (mode == YF_REDACT_FILL && block != 0) return "block must be 0 in YF_REDACT_FILL";
  if (mode == YF_REDACT_FILL && (colour >> 24) != 0) return "colour must be 0x00RRGGBB (0x00YYUUVV): its top byte is not 0";
  if (margin_permille < 0 || margin_permille > 1000) return "margin_permille must be in [0, 1000]";
  if ((flags & ~YF_CROP_SQUARE) != 0) return "flags must be 0 or YF_CROP_SQUARE";
  return NULL;
}

#endif
