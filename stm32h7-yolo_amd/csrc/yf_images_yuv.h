/* 4:2:0 semi-planar surfaces (NV12: a Y plane, then a plane of U, V byte pairs at half resolution; NV21: V, U) to the network's frames:
 * the arithmetic of cv2.cvtColor(yuv, cv2.COLOR_YUV2BGR_NV12 / _NV21) followed by the resize of yf_images_taps.h, shared by the device
 * kernel (yf_images.hip), a host build (yf_images_host.c) and the sanitizer program (tests/csrc/yuv_sanitize_main.c).  Restated from
 * OpenCV 4's imgproc/src/color_yuv.simd.hpp (YUV420sp -> RGB, BT.601 limited range) as ptq.yuv420sp_to_rgb_u8 states it; like the
 * resize, that restatement has not been pinned against a real cv2.  Everything is integer: no contraction concerns.
 *
 * One pixel, int32 throughout (the largest magnitude, 239 * CY + 2^19 + 127 * CUB, is about 5.6e8):
 *   yy = max(0, Y - 16) * CY;  uu = U - 128;  vv = V - 128
 *   R = clamp8((yy + (1 << 19) + CVR * vv) >> 20)
 *   G = clamp8((yy + (1 << 19) + CVG * vv + CUG * uu) >> 20)
 *   B = clamp8((yy + (1 << 19) + CUB * uu) >> 20)                          (arithmetic shift of negatives)
 * Pixel (y, x) takes the chroma pair at UV row y >> 1, byte columns 2 * (x >> 1) and 2 * (x >> 1) + 1; chroma is not interpolated.
 * The clamp makes the conversion non-linear, so a resized pixel converts its four source samples first and interpolates the bytes. */
#ifndef YF_IMAGES_YUV_H
#define YF_IMAGES_YUV_H
#include <stdint.h>
#include "../../include/yf_images.h"
#include "yf_images_taps.h"

#define YFI_YUV_CY    1220542
#define YFI_YUV_CUB   2116026
#define YFI_YUV_CUG   (-409993)
#define YFI_YUV_CVG   (-852492)
#define YFI_YUV_CVR   1673527
#define YFI_YUV_SHIFT 20

/* what a chroma pair adds to the luma term of each channel, rounding constant included: computed once per pair */
typedef struct yfi_chroma { int32_t r, g, b; } yfi_chroma;

YFI_HD yfi_chroma yfi_yuv_chroma(int32_t u, int32_t v) {
  const int32_t uu = u - 128, vv = v - 128, half = 1 << (YFI_YUV_SHIFT - 1);
  yfi_chroma c;
  c.r = half + YFI_YUV_CVR * vv;
  c.g = half + YFI_YUV_CVG * vv + YFI_YUV_CUG * uu;
  c.b = half + YFI_YUV_CUB * uu;
  return c;
}

YFI_HD int32_t yfi_yuv_luma(int32_t y) { return (y > 16 ? y - 16 : 0) * YFI_YUV_CY; }

/* one channel of one pixel: the luma term plus the pair's term of that channel, shifted (arithmetically) and saturated */
YFI_HD int32_t yfi_yuv_channel(int32_t yy, int32_t c) {
  const int32_t v = (yy + c) >> YFI_YUV_SHIFT;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

/* A surface of h x w luma bytes (rows stride_y apart, first at offset_y) and h / 2 rows of w chroma bytes (stride_uv, offset_uv) in a
 * buffer of `bytes` bytes: h, w even and in 2..16384, both strides >= w, each plane inside the buffer -- without overflow for any
 * input.  No alignment is asked of offsets or strides, and the planes may lie in either order. */
YFI_HD int yfi_yuv_image_ok(uint64_t offset_y, uint64_t offset_uv, int64_t h, int64_t w, int64_t stride_y, int64_t stride_uv, uint64_t bytes) {
  if (h < 2 || w < 2 || h > 16384 || w > 16384 || (h & 1) != 0 || (w & 1) != 0) return 0;
  return yfi_image_ok(offset_y, h, w, stride_y, 1, bytes) && yfi_image_ok(offset_uv, h / 2, w, stride_uv, 1, bytes);
}

/* ---- addresses ----  The byte offsets an output pixel samples, from its two axis taps.  Columns: the luma bytes s0, s1 of a row and
 * the first byte of their chroma pairs (the second one follows it).  Rows: the same from the start of the Y plane and of the UV plane. */
typedef struct yfi_yuv_xtap { int32_t y0, y1, c0, c1, w0, w1; } yfi_yuv_xtap;
typedef struct yfi_yuv_ytap { int64_t y0, y1, c0, c1; int32_t w0, w1; } yfi_yuv_ytap;

YFI_HD yfi_yuv_xtap yfi_yuv_xtap_of(yfi_tap t) {
  yfi_yuv_xtap x;
  x.y0 = t.s0; x.y1 = t.s1;
  x.c0 = (t.s0 >> 1) * 2; x.c1 = (t.s1 >> 1) * 2;
  x.w0 = t.w0; x.w1 = t.w1;
  return x;
}

YFI_HD yfi_yuv_ytap yfi_yuv_ytap_of(yfi_tap t, int64_t stride_y, int64_t stride_uv) {
  yfi_yuv_ytap y;
  y.y0 = (int64_t)t.s0 * stride_y; y.y1 = (int64_t)t.s1 * stride_y;
  y.c0 = (int64_t)(t.s0 >> 1) * stride_uv; y.c1 = (int64_t)(t.s1 >> 1) * stride_uv;
  y.w0 = t.w0; y.w1 = t.w1;
  return y;
}

/* the chroma terms of the pair whose first byte is at p; v_first: NV21 */
YFI_HD yfi_chroma yfi_yuv_pair(const uint8_t* p, int v_first) {
  const int32_t a = p[0], b = p[1];
  return v_first ? yfi_yuv_chroma(b, a) : yfi_yuv_chroma(a, b);
}

/* One output pixel: rgb[c] = the resize (yfi_hpass, yfi_vpass) of channel c of the four converted source pixels, 0..255.  yp, uvp: the
 * first byte of the Y plane and of the UV plane.  Four luma bytes are read, and one chroma pair per distinct pair among the four
 * samples (two columns or two rows often share theirs); each pair's three terms are computed once. */
YFI_HD void yfi_yuv_sample(const uint8_t* yp, const uint8_t* uvp, yfi_yuv_xtap tx, yfi_yuv_ytap ty, int v_first, int32_t rgb[3]) {
  const uint8_t* ya = yp + ty.y0;
  const uint8_t* yb = yp + ty.y1;
  const uint8_t* ua = uvp + ty.c0;
  const uint8_t* ub = uvp + ty.c1;
  const int32_t a0 = yfi_yuv_luma(ya[tx.y0]), a1 = yfi_yuv_luma(ya[tx.y1]);
  const int32_t b0 = yfi_yuv_luma(yb[tx.y0]), b1 = yfi_yuv_luma(yb[tx.y1]);
  const int same_col = tx.c1 == tx.c0, same_row = ty.c1 == ty.c0;
  const yfi_chroma ca0 = yfi_yuv_pair(ua + tx.c0, v_first);
  const yfi_chroma ca1 = same_col ? ca0 : yfi_yuv_pair(ua + tx.c1, v_first);
  const yfi_chroma cb0 = same_row ? ca0 : yfi_yuv_pair(ub + tx.c0, v_first);
  const yfi_chroma cb1 = same_row ? ca1 : (same_col ? cb0 : yfi_yuv_pair(ub + tx.c1, v_first));
  const int32_t r0 = yfi_hpass(yfi_yuv_channel(a0, ca0.r), yfi_yuv_channel(a1, ca1.r), tx.w0, tx.w1);
  const int32_t r1 = yfi_hpass(yfi_yuv_channel(b0, cb0.r), yfi_yuv_channel(b1, cb1.r), tx.w0, tx.w1);
  const int32_t g0 = yfi_hpass(yfi_yuv_channel(a0, ca0.g), yfi_yuv_channel(a1, ca1.g), tx.w0, tx.w1);
  const int32_t g1 = yfi_hpass(yfi_yuv_channel(b0, cb0.g), yfi_yuv_channel(b1, cb1.g), tx.w0, tx.w1);
  const int32_t l0 = yfi_hpass(yfi_yuv_channel(a0, ca0.b), yfi_yuv_channel(a1, ca1.b), tx.w0, tx.w1);
  const int32_t l1 = yfi_hpass(yfi_yuv_channel(b0, cb0.b), yfi_yuv_channel(b1, cb1.b), tx.w0, tx.w1);
  rgb[0] = yfi_vpass(r0, r1, ty.w0, ty.w1);
  rgb[1] = yfi_vpass(g0, g1, ty.w0, ty.w1);
  rgb[2] = yfi_vpass(l0, l1, ty.w0, ty.w1);
}

#endif
