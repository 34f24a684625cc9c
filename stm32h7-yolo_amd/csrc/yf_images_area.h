/* Area-averaged frames: every source pixel of a picture counted in its frame, each with the exact share of it that an output pixel
 * covers.  The definition is this library's own, in integers only (include/yf_images.h states the interface); it is shared by the device
 * kernels (yf_images_area.hip.h), a host build (yf_images_host.c, which tests/test_area_host.py checks against ptq.resize_area_u8 and a
 * brute-force count of grid cells without a GPU) and a sanitizer program (tests/csrc/area_sanitize_main.c).
 *
 * One axis of n_in source and n_out output positions, on the grid of n_in * n_out sub-positions: output d covers [d n_in, (d + 1) n_in),
 * source s covers [s n_out, (s + 1) n_out), and a(d, s) is the length of the overlap of the two, an integer in [0, min(n_in, n_out)]
 * (yfi_area_weight).  For every d the a(d, s) sum to n_in; the sources with a weight are yfi_area_first(d) .. yfi_area_last(d), and all
 * but the first and the last of them have the weight n_out.  The rule holds for any ratio: a reduction, an enlargement, and
 * n_in = n_out, where it is the identity.
 *
 * One output pixel (y, x) of a picture of H x W resized to h_out x w_out, per channel, with D = H W:
 *   S = sum over sy, sx of ay(y, sy) ax(x, sx) p[sy][sx]          ay on (H, h_out), ax on (W, w_out)
 *   v = (2 S + D) / (2 D)                                         integer division: the exact area average, rounded HALF UP
 * S reaches 255 * 16384^2, about 6.8e10: the vertical sum and the division are 64-bit.  A row's horizontal sum, at most 255 * 16384, fits
 * 32 bits (yfi_area_row).  No floats and no weight tables rounded to a fixed point: integer sums are the same in any order of addition,
 * so a kernel may accumulate in whatever order is fastest and still equal the host build bit for bit.
 *
 * Frame element: (int8)(v - 128), or the fp16 bits yfi_f16_of_u8(v); channel order RGB whatever the format, the alpha byte never read.
 * NV12 / NV21: every source pixel is converted first (yf_images_yuv.h; pixel (y, x) takes the chroma pair of UV row y >> 1), then
 * averaged: the frame of cvtColor followed by the area resize.
 * Fit: YF_FIT_STRETCH resizes the picture to the whole frame; YF_FIT_LETTERBOX resizes it to the rectangle of yfi_fit_of
 * (yf_images_fit.h: its height and width are the two n_out) at (x0, y0), the rest of the frame is `pad`.  A square picture has the same
 * bytes either way.  Boxes map back through the fit, not through the filter: the plain ragged decodes, or yf_images_decode_fit_*.
 *
 * Relation to OpenCV: for integer ratios v is the half-up-rounded block mean, which is what cv2.resize(..., INTER_AREA)'s integer path
 * gives; at exactly 2x that is (a + b + c + d + 2) >> 2, the bytes of the linear prepare (yf_images_taps.h).  For other ratios OpenCV
 * accumulates float weights; this is the exact value those approximate.  Like the rest, it has not been pinned against a real cv2. */
#ifndef YF_IMAGES_AREA_H
#define YF_IMAGES_AREA_H
#include <stddef.h>
#include <stdint.h>
#include "../../include/yf_images.h"
#include "yf_images_taps.h"
#include "yf_images_fit.h"

/* all in int32: d < n_out <= 160 and s < n_in <= 16384, so every product is below 2^22 */
YFI_HD int32_t yfi_area_first(int32_t d, int32_t n_in, int32_t n_out) { return d * n_in / n_out; }
YFI_HD int32_t yfi_area_last(int32_t d, int32_t n_in, int32_t n_out) { return ((d + 1) * n_in - 1) / n_out; }

YFI_HD int32_t yfi_area_weight(int32_t d, int32_t s, int32_t n_in, int32_t n_out) {
  const int32_t lo_d = d * n_in, lo_s = s * n_out;
  const int32_t lo = lo_d > lo_s ? lo_d : lo_s;
  const int32_t hi = lo_d + n_in < lo_s + n_out ? lo_d + n_in : lo_s + n_out;
  return hi > lo ? hi - lo : 0;
}

/* what a thread (or a loop) keeps of one output index of an axis: its sources [first, last] and the weights of those two (the ones
 * between weigh n_out; first == last: w_first is the whole weight) */
typedef struct yfi_area_span { int32_t first, last, w_first, w_last, w_mid; } yfi_area_span;

YFI_HD yfi_area_span yfi_area_span_of(int32_t d, int32_t n_in, int32_t n_out) {
  yfi_area_span a;
  a.first = yfi_area_first(d, n_in, n_out);
  a.last = yfi_area_last(d, n_in, n_out);
  a.w_first = yfi_area_weight(d, a.first, n_in, n_out);
  a.w_last = yfi_area_weight(d, a.last, n_in, n_out);
  a.w_mid = n_out;
  return a;
}

YFI_HD int32_t yfi_area_span_weight(yfi_area_span a, int32_t s) { return s == a.first ? a.w_first : (s == a.last ? a.w_last : a.w_mid); }

/* the rounded average of a sum S of weights D = H W (both fit 64 bits with room: 2 S + D < 2^38) */
YFI_HD int32_t yfi_area_round(uint64_t S, uint64_t D) { return (int32_t)((2 * S + D) / (2 * D)); }

/* where the picture lies in its frame: the whole frame, or the letterbox rectangle */
YFI_HD yf_fit yfi_area_rect(int32_t h, int32_t w, int out_hw, int fit) {
  if (fit == YF_FIT_LETTERBOX) return yfi_fit_of(h, w, out_hw);
  yf_fit f;
  f.x0 = 0; f.y0 = 0; f.width = out_hw; f.height = out_hw;
  return f;
}

/* How many bands of whole output rows a frame is split into, one job per (frame, band): from n and out_hw alone, since the pictures'
 * sizes live in device memory.  About 2048 jobs (8 per CU) where the batch is small, one band per frame from 2048 frames on; a band
 * is an even number of rows, so that it is whole 16-byte vectors of every frame type (two rows of 56 int8 pixels are 336 bytes).  The
 * frames do not depend on it. */
#define YFI_AREA_JOBS 2048
YFI_HD int yfi_area_bands(long n, int out_hw) {
  const long half = out_hw / 2;
  if (n < 1) return 1;
  const long b = (YFI_AREA_JOBS + n - 1) / n;
  return (int)(b < 1 ? 1 : (b > half ? half : b));
}

/* the first row of band b of `bands` (b = bands: one past the last row of the frame) */
YFI_HD int yfi_area_band_row(int b, int bands, int out_hw) { return 2 * (int)((long)b * (out_hw / 2) / bands); }

/* ---- argument checks ----  the text of the first fault, or NULL; the order is part of the behaviour.  `yuv`: the entry's family (0:
 * packed pixels, 1: NV12 / NV21 surfaces), `f16`: fp16 frames (out_hw is then 56). */
static inline const char* yfi_area_check_prepare(int yuv, int f16, const void* d_pixels, int format, const void* d_images, long n, int out_hw,
                                                 int fit, int pad, const void* d_frames, const void* d_status) {
  const int packed = format == YF_PIX_BGR8 || format == YF_PIX_RGB8 || format == YF_PIX_BGRA8 || format == YF_PIX_RGBA8;
  const int planes = format == YF_PIX_NV12 || format == YF_PIX_NV21;
  if (!yuv && planes) return "format YF_PIX_NV12 / YF_PIX_NV21: such surfaces go through yf_images_prepare_area_yuv_ragged_device or "
                             "yf_images_prepare_area_yuv_f16_ragged_device";
  if (!yuv && !packed) return "format must be YF_PIX_BGR8, YF_PIX_RGB8, YF_PIX_BGRA8 or YF_PIX_RGBA8";
  if (yuv && packed) return "format YF_PIX_BGR8 / RGB8 / BGRA8 / RGBA8: packed pixels go through yf_images_prepare_area_ragged_device or "
                            "yf_images_prepare_area_f16_ragged_device";
  if (yuv && !planes) return "format must be YF_PIX_NV12 or YF_PIX_NV21";
  if (f16 ? out_hw != 56 : (out_hw != 56 && out_hw != 160)) return f16 ? "fp16 frames are 56x56" : "out_hw must be 56 or 160";
  if (fit != YF_FIT_STRETCH && fit != YF_FIT_LETTERBOX) return "fit must be YF_FIT_STRETCH or YF_FIT_LETTERBOX";
  if (pad < 0 || pad > 255) return "pad must be in [0, 255]";
  if (n < 0) return "n < 0";
  if (!d_frames || ((uintptr_t)d_frames & 15) != 0) return "d_frames is NULL or not 16-byte aligned";
  if (n > 0 && (!d_pixels || !d_images || ((uintptr_t)d_images & 7) != 0 || !d_status || ((uintptr_t)d_status & 3) != 0))
    return "d_pixels, d_images (8-byte aligned) or d_status (4-byte aligned) is NULL or misaligned";
  return NULL;
}

#endif
