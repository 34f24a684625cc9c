/* Letterboxed frames: the picture resized with its aspect kept, centred in the square frame and padded with one grey, and the decoded
 * boxes mapped back through the same rectangle.  The definition is this library's own (include/yf_images.h states the interface); it is
 * shared by the device kernels (yf_images_fit.hip.h), a host build (yf_images_host.c, which tests/test_fit_host.py checks against
 * ptq.letterbox_fit / ptq.letterbox_u8 without a GPU) and a sanitizer program (tests/csrc/fit_sanitize_main.c).
 *
 * The fit of a picture of H x W in a frame of side S (56 or 160), all in int64:
 *   W >= H:  width = S, height = max(1, (2 H S + W) / (2 W))      the exact ratio H S / W rounded HALF UP;  W < H symmetric
 *   x0 = (S - width) / 2,  y0 = (S - height) / 2                  floor: the odd pixel of padding goes right and bottom, as ultralytics'
 *                                                                 LetterBox centres it (its round(dw - 0.1), round(dw + 0.1))
 * A square picture has {0, 0, S, S}.  The rounding is THE LIBRARY'S CHOICE: the trainers call Python's round(), which rounds an exact half
 * to even; the two differ only where H S / W is exactly k + 1/2 (1920 x 1080 at 56: 31.5 -> 32 here, 32 there too, but 24.5 -> 25 here
 * and 24 there).
 *
 * Frame: inside the rectangle frame[y0 + y][x0 + x][c] = (int8)(R[y][x][rgb(c)] - 128), R = cv2.resize(picture, (width, height)): the
 * taps of yf_images_taps.h at a run-time n_out (yfi_axis_tap(x, width, W), yfi_axis_tap(y, height, H)), as the crop uses them.  Outside:
 * (int8)(pad - 128), pad in 0..255.  fp16 frames: yfi_f16_of_u8 of the same bytes.  A tap of a padded column or row says "outside"
 * (yfi_fit_tap: w0 = -1) and is never dereferenced.
 *
 * Boxes: the YF_DECODE_PY decode up to the four edges in frame pixels (yfi_d160_box of yf_images_decode160.h up to its scales), then
 *   x = (x - (float)x0) * x_scale,  x_scale = (float)((double)W / (double)width)
 *   y = (y - (float)y0) * y_scale,  y_scale = (float)((double)H / (double)height)
 * in float32, one IEEE operation per step, no contraction, and the float32 -> int32 of every decode (yfi_d160_f2i).  The scales are per
 * axis -- the ones the resize used --, not one shared ratio.  Nothing is clipped.  For a square picture x - 0.0f is x (bit for bit, NaN
 * and the zeros included) and the scale is W / S: the record is yfi_d160_box's.  Written once: yfi_fit_box. */
#ifndef YF_IMAGES_FIT_H
#define YF_IMAGES_FIT_H
#include <stddef.h>
#include <stdint.h>
#include "../../include/yf_images.h"
#include "yf_images_taps.h"
#include "yf_images_decode160.h"
#include "yf_images_float.h"
#ifdef __clang__
#pragma clang fp contract(off)
#endif

YFI_HD yf_fit yfi_fit_of(int64_t h, int64_t w, int64_t S) {
  yf_fit f;
  int64_t fw = S, fh = S;
  if (w > h) { fh = (2 * h * S + w) / (2 * w); if (fh < 1) fh = 1; }
  else if (h > w) { fw = (2 * w * S + h) / (2 * h); if (fw < 1) fw = 1; }
  f.width = (int32_t)fw; f.height = (int32_t)fh;
  f.x0 = (int32_t)((S - fw) / 2); f.y0 = (int32_t)((S - fh) / 2);
  return f;
}

/* The tap of frame index d along an axis on which the picture takes [start, start + extent) of the frame and has n_in pixels; outside
 * that span w0 = -1 (a weight is otherwise 0..2048) and the indices are 0: such a tap is not to be dereferenced. */
YFI_HD yfi_tap yfi_fit_tap(int d, int start, int extent, int n_in) {
  if (d < start || d >= start + extent) {
    yfi_tap t;
    t.s0 = 0; t.s1 = 0; t.w0 = -1; t.w1 = 0;
    return t;
  }
  return yfi_axis_tap(d - start, extent, n_in);
}

/* what a decode needs of a picture's fit: the offsets as float32 and the two scales */
typedef struct yfi_fit_map { float x0, y0, x_scale, y_scale; } yfi_fit_map;

YFI_HD yfi_fit_map yfi_fit_map_of(int32_t h, int32_t w, int S) {
  const yf_fit f = yfi_fit_of(h, w, S);
  yfi_fit_map m;
  m.x0 = (float)f.x0; m.y0 = (float)f.y0;
  m.x_scale = (float)((double)w / (double)f.width);
  m.y_scale = (float)((double)h / (double)f.height);
  return m;
}

/* THE tail: from the four transcendental values to d's x1, y1, x2, y2.  sx, sy: the sigmoids of the x and y logits; ew, eh: the
 * exponentials of the w and h logits. */
YFI_HD void yfi_fit_box(float sx, float sy, float ew, float eh, int a, int row, int col, yfi_fit_map m, yf_det* d) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const float anc_w = a == 0 ? 9.f : (a == 1 ? 12.f : 22.f), anc_h = a == 0 ? 14.f : (a == 1 ? 17.f : 21.f);
  const float cx = (sx + (float)col) * 8.f, cy = (sy + (float)row) * 8.f;
  const float bw = ew * anc_w, bh = eh * anc_h;
  float x1 = cx - bw / 2, y1 = cy - bh / 2, x2 = cx + bw / 2, y2 = cy + bh / 2;
  x1 = (x1 - m.x0) * m.x_scale; x2 = (x2 - m.x0) * m.x_scale;
  y1 = (y1 - m.y0) * m.y_scale; y2 = (y2 - m.y0) * m.y_scale;
  d->x1 = yfi_d160_f2i(x1); d->y1 = yfi_d160_f2i(y1); d->x2 = yfi_d160_f2i(x2); d->y2 = yfi_d160_f2i(y2);
}

/* byte offset (index, for float logits) in a G x G head of candidate i's six values; i = (anchor * G + row) * G + col */
YFI_HD int yfi_fit_offset(int i, int G) {
  const int a = i / (G * G);
  return (i - a * G * G) * 18 + a * 6;
}

/* One record from candidate i of a G x G int8 head (p = its six bytes); sig_bits, exp_bits: the two 256-entry tables. */
YFI_HD yf_det yfi_fit_candidate(const int8_t* p, int i, int G, int32_t frame, const uint32_t* sig_bits, const uint32_t* exp_bits,
                                yfi_fit_map m) {
  const int a = i / (G * G), cell = i - a * G * G;
  const int row = cell / G, col = cell - row * G;
  yf_det d;
  d.frame = frame; d.anchor = (uint8_t)a; d.row = (uint8_t)row; d.col = (uint8_t)col;
  d.q_conf = p[4]; d.conf = yfi_d160_bits(sig_bits[p[4] + 128]);
  yfi_fit_box(yfi_d160_bits(sig_bits[p[0] + 128]), yfi_d160_bits(sig_bits[p[1] + 128]), yfi_d160_bits(exp_bits[p[2] + 128]),
              yfi_d160_bits(exp_bits[p[3] + 128]), a, row, col, m, &d);
  return d;
}

/* ... and from candidate i of the fp16 network's float32 logits (p = its six values); conf = yfi_sigmoid_f32(p[4]), which the caller
 * has computed to decide that the candidate fires (conf > 0.7f). */
YFI_HD yf_det yfi_fit_candidate_f32(const float* p, int i, int32_t frame, float conf, yfi_fit_map m) {
  const int a = i / 49, cell = i - a * 49;
  const int row = cell / 7, col = cell - row * 7;
  yf_det d;
  d.frame = frame; d.anchor = (uint8_t)a; d.row = (uint8_t)row; d.col = (uint8_t)col;
  d.q_conf = 0; d.conf = conf;
  yfi_fit_box(yfi_sigmoid_f32(p[0]), yfi_sigmoid_f32(p[1]), yfi_exp_f32(p[2]), yfi_exp_f32(p[3]), a, row, col, m, &d);
  return d;
}

/* a descriptor a decode takes: both sides in range (and no status 1) */
YFI_HD int yfi_fit_sides_ok(int32_t h, int32_t w) { return h >= 1 && h <= YF_IMAGES_MAX_SIDE && w >= 1 && w <= YF_IMAGES_MAX_SIDE; }

/* ---- argument checks ----  the text of the first fault, or NULL; the order is part of the behaviour.  What the host can see of a
 * prepare: `yuv` the entry's family (0: packed pixels, 1: NV12 / NV21 surfaces), `f16` fp16 frames (out_hw is then 56). */
static inline const char* yfi_fit_check_prepare(int yuv, int f16, const void* d_pixels, int format, const void* d_images, long n, int out_hw,
                                                int pad, const void* d_frames, const void* d_status) {
  const int packed = format == YF_PIX_BGR8 || format == YF_PIX_RGB8 || format == YF_PIX_BGRA8 || format == YF_PIX_RGBA8;
  const int planes = format == YF_PIX_NV12 || format == YF_PIX_NV21;
  if (!yuv && planes) return "format YF_PIX_NV12 / YF_PIX_NV21: such surfaces go through yf_images_prepare_fit_yuv_ragged_device or "
                             "yf_images_prepare_fit_yuv_f16_ragged_device";
  if (!yuv && !packed) return "format must be YF_PIX_BGR8, YF_PIX_RGB8, YF_PIX_BGRA8 or YF_PIX_RGBA8";
  if (yuv && packed) return "format YF_PIX_BGR8 / RGB8 / BGRA8 / RGBA8: packed pixels go through yf_images_prepare_fit_ragged_device or "
                            "yf_images_prepare_fit_f16_ragged_device";
  if (yuv && !planes) return "format must be YF_PIX_NV12 or YF_PIX_NV21";
  if (f16 ? out_hw != 56 : (out_hw != 56 && out_hw != 160)) return f16 ? "fp16 frames are 56x56" : "out_hw must be 56 or 160";
  if (pad < 0 || pad > 255) return "pad must be in [0, 255]";
  if (n < 0) return "n < 0";
  if (!d_frames || ((uintptr_t)d_frames & 15) != 0) return "d_frames is NULL or not 16-byte aligned";
  if (n > 0 && (!d_pixels || !d_images || ((uintptr_t)d_images & 7) != 0 || !d_status || ((uintptr_t)d_status & 3) != 0))
    return "d_pixels, d_images (8-byte aligned) or d_status (4-byte aligned) is NULL or misaligned";
  return NULL;
}

/* ... and of a decode: `f32` the fp16 network's float32 logits (out_hw is then 56) */
static inline const char* yfi_fit_check_decode(int f32, const void* d_heads, const void* d_images, const void* d_status, long n, int out_hw,
                                               const void* d_dets, const void* d_counts, int cap) {
  if (out_hw != 56 && (f32 || out_hw != 160)) return f32 ? "float32 logits are those of 56x56 frames" : "out_hw must be 56 or 160";
  if (n < 0) return "n < 0";
  if (!d_heads) return f32 ? "d_logits is NULL" : "d_heads is NULL";
  if (f32 && ((uintptr_t)d_heads & 3) != 0) return "d_logits is not 4-byte aligned";
  if (out_hw == 160 && ((uintptr_t)d_heads & 15) != 0) return "d_heads is not 16-byte aligned";
  if (!d_dets) return "d_dets is NULL";
  if (!d_counts) return "d_counts is NULL";
  if (((uintptr_t)d_dets & 3) != 0) return "d_dets is not 4-byte aligned";
  if (((uintptr_t)d_counts & 3) != 0) return "d_counts is not 4-byte aligned";
  if (out_hw == 56 && (cap < 1 || cap > 147)) return "cap must be in [1, 147]";
  if (out_hw == 160 && (cap < 1 || cap > YF_IMAGES_CAND160)) return "cap must be in [1, 1200]";
  if (n > 0 && (!d_images || ((uintptr_t)d_images & 7) != 0)) return "d_images is NULL or not 8-byte aligned";
  if (((uintptr_t)d_status & 3) != 0) return "d_status is not 4-byte aligned";
  return NULL;
}

#endif
