/* The arithmetic of cv2.resize(..., INTER_LINEAR) on uint8 images, shared by the device kernel (yf_images.hip) and a host build
 * (yf_images_host.c, libyf_images_host.so, which tests/test_images_host.py checks against ptq.resize_linear_u8 for every size 1..8192).
 * Restated from OpenCV 4's imgproc/resize.cpp as ptq.resize_linear_u8 states it; that restatement has not been pinned against a real cv2.
 *
 * Per axis and output index d:  f = (float)((d + 0.5) * (n_in / n_out) - 0.5) in double, s = floor(f), f -= s, clamped at both edges
 * (f = 0), weights rint((1 - f) * 2048) and rint(f * 2048) (float32 products, ties to even).  Per output: horizontal int32
 * S[s] * a0 + S[s + 1] * a1, vertical (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2.  OpenCV forms the scale as
 * 1 / (n_out / n_in); the float f is the same for every size 1..8192 at 56 and 160.  OpenCV's switch of an exact 2x reduction to
 * INTER_AREA gives (a + b + c + d + 2) >> 2, which these weights give too.
 * Compile without FMA contraction (-ffp-contract=off): a fused (d + 0.5) * scale - 0.5 can land f on the other side of a boundary. */
#ifndef YF_IMAGES_TAPS_H
#define YF_IMAGES_TAPS_H
#include <stdint.h>
#ifdef __HIPCC__
#define YFI_HD __host__ __device__ __forceinline__
#else
#include <math.h>
#define YFI_HD static inline
#endif

typedef struct yfi_tap {
  int32_t s0, s1;      /* source indices (s1 = min(s0 + 1, n_in - 1)) */
  int32_t w0, w1;      /* 11-bit fixed-point weights */
} yfi_tap;

YFI_HD yfi_tap yfi_axis_tap(int d, int n_out, int n_in) {
  const double scale = (double)n_in / (double)n_out;
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (s < 0) { s = 0; f = 0.f; }
  if (s >= n_in - 1) { s = n_in - 1; f = 0.f; }
  yfi_tap t;
  t.s0 = s;
  t.s1 = s + 1 < n_in ? s + 1 : n_in - 1;
  t.w0 = (int32_t)rintf((1.f - f) * 2048.f);
  t.w1 = (int32_t)rintf(f * 2048.f);
  return t;
}

/* horizontal pass of one channel: two source bytes of a row */
YFI_HD int32_t yfi_hpass(int32_t p0, int32_t p1, int32_t a0, int32_t a1) { return p0 * a0 + p1 * a1; }

/* vertical pass of two horizontal results, saturated to uint8 */
YFI_HD int32_t yfi_vpass(int32_t r0, int32_t r1, int32_t b0, int32_t b1) {
  const int32_t v = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

/* An image of h x w pixels of C bytes, rows rs bytes apart, first byte at `offset` of a buffer of `bytes` bytes: 1 <= h, w <= 16384,
 * rs >= w * C, and offset + (h - 1) * rs + w * C <= bytes, without overflow for any input. */
YFI_HD int yfi_image_ok(uint64_t offset, int64_t h, int64_t w, int64_t rs, int C, uint64_t bytes) {
  if (h < 1 || w < 1 || h > 16384 || w > 16384) return 0;
  const uint64_t row = (uint64_t)w * (uint64_t)C;
  if (rs < (int64_t)row) return 0;
  if (offset > bytes) return 0;
  const uint64_t rem = bytes - offset;
  if (row > rem) return 0;
  if (h > 1 && (uint64_t)(h - 1) > (rem - row) / (uint64_t)rs) return 0;
  return 1;
}

#endif
