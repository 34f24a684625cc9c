/* The per-candidate box decode of a 20x20 head (160x160 frames), shared by the device kernel (yf_images.hip, decode160_kernel) and a host
 * build (yf_images_host.c, libyf_images_host.so, which tests/test_boxes160_host.py checks against the oracle's yfo_decode_py without a GPU).
 * Restated from yoloface/tflite/tflite_prediction.py:43-63 with the hard-coded 7 of line 50 read as the script's own nx, ny (20 here):
 * stride 8 and the anchors unchanged, the scales W/160. and H/160. on a float32 array.  The arithmetic is YF_DECODE_PY's of
 * csrc/yf_decode.hip.h: every transcendental is a look-up in the committed float32 tables (index q + 128), everything else a single
 * float32 operation in the script's order, no contraction; float -> int32 as numpy on an x86-64 PC (truncation, out of range -> INT32_MIN).
 * Candidates are numbered in the script's loop order: i = (anchor * 20 + row) * 20 + col, i < 1200. */
#ifndef YF_IMAGES_DECODE160_H
#define YF_IMAGES_DECODE160_H
#include <stdint.h>
#include <string.h>
#include "../../include/yf_images.h"
#ifndef YFI_HD
#ifdef __HIPCC__
#define YFI_HD __host__ __device__ __forceinline__
#else
#define YFI_HD static inline
#endif
#endif

#define YFI_D160_CELLS (YF_IMAGES_GRID160 * YF_IMAGES_GRID160)
#define YFI_D160_HEAD_BYTES (YFI_D160_CELLS * 18)

YFI_HD float yfi_d160_bits(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}

YFI_HD int32_t yfi_d160_f2i(float v) {
  return (v > -2147483904.0f && v < 2147483648.0f) ? (int32_t)v : (int32_t)0x80000000;
}

/* byte offset in the head of candidate i's six values (x, y, w, h, conf, class) */
YFI_HD int yfi_d160_offset(int i) {
  const int a = i / YFI_D160_CELLS;
  return (i - a * YFI_D160_CELLS) * 18 + a * 6;
}

/* The smallest quantised confidence that passes `conf > 0.7f`, from the sigmoid table (which must not decrease: yfi_d160_monotonic);
 * 128 when none does.  The decode compares bytes against it and assembles boxes only for the candidates that fire. */
YFI_HD int yfi_d160_q_threshold(const uint32_t* sig_bits) {
  for (int i = 0; i < 256; ++i)
    if (yfi_d160_bits(sig_bits[i]) > 0.7f) return i - 128;
  return 128;
}

YFI_HD int yfi_d160_monotonic(const uint32_t* sig_bits) {
  for (int i = 1; i < 256; ++i)
    if (yfi_d160_bits(sig_bits[i]) < yfi_d160_bits(sig_bits[i - 1])) return 0;
  return 1;
}

/* The tail every YF_DECODE_PY-style decode shares, from the four transcendental values on: centre, size, edges, scales, float32 -> int32
 * into d's x1, y1, x2, y2.  sx, sy: the sigmoids of the x and y logits; ew, eh: the exponentials of the w and h logits. */
YFI_HD void yfi_d160_box(float sx, float sy, float ew, float eh, int a, int row, int col, float w_scale, float h_scale, yf_det* d) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const float anc_w = a == 0 ? 9.f : (a == 1 ? 12.f : 22.f), anc_h = a == 0 ? 14.f : (a == 1 ? 17.f : 21.f);
  const float cx = (sx + (float)col) * 8.f, cy = (sy + (float)row) * 8.f;
  const float bw = ew * anc_w, bh = eh * anc_h;
  float x1 = cx - bw / 2, y1 = cy - bh / 2, x2 = cx + bw / 2, y2 = cy + bh / 2;
  x1 *= w_scale; x2 *= w_scale; y1 *= h_scale; y2 *= h_scale;
  d->x1 = yfi_d160_f2i(x1); d->y1 = yfi_d160_f2i(y1); d->x2 = yfi_d160_f2i(x2); d->y2 = yfi_d160_f2i(y2);
}

/* One record from candidate i (p = its six head bytes) of frame `frame`; sig_bits, exp_bits: the two 256-entry tables. */
YFI_HD yf_det yfi_d160_candidate(const int8_t* p, int i, int32_t frame, const uint32_t* sig_bits, const uint32_t* exp_bits,
                                 float w_scale, float h_scale) {
  const int a = i / YFI_D160_CELLS, cell = i - a * YFI_D160_CELLS;
  const int row = cell / YF_IMAGES_GRID160, col = cell - row * YF_IMAGES_GRID160;
  yf_det d;
  d.frame = frame; d.anchor = (uint8_t)a; d.row = (uint8_t)row; d.col = (uint8_t)col;
  d.q_conf = p[4]; d.conf = yfi_d160_bits(sig_bits[p[4] + 128]);
  yfi_d160_box(yfi_d160_bits(sig_bits[p[0] + 128]), yfi_d160_bits(sig_bits[p[1] + 128]), yfi_d160_bits(exp_bits[p[2] + 128]),
               yfi_d160_bits(exp_bits[p[3] + 128]), a, row, col, w_scale, h_scale, &d);
  return d;
}

#endif
