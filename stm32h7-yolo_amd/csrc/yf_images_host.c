/* Host build of the resize arithmetic in yf_images_taps.h, the suppression arithmetic in yf_images_nms.h, the 20x20 decode arithmetic in
 * yf_images_decode160.h and the fp16 frames and float32 decode of yf_images_float.h (the functions the device kernels call), for the CPU
 * tests only: libyf_images_host.so, no HIP. */
#include <stddef.h>
#include <stdint.h>
#include "yf_images_taps.h"
#include "yf_images_nms.h"
#include "yf_images_decode160.h"
#include "yf_images_float.h"
#include "gen/yf_decode_tables_gen.h"

#define EXPORT __attribute__((visibility("default")))

/* out[4] = {s0, s1, w0, w1} of output index d */
EXPORT void yfi_tap_host(int d, int n_out, int n_in, int32_t* out) {
  const yfi_tap t = yfi_axis_tap(d, n_out, n_in);
  out[0] = t.s0; out[1] = t.s1; out[2] = t.w0; out[3] = t.w1;
}

/* cv2.resize(src, (out_w, out_h)) of an h x w image of C channels (rows rs bytes apart) -> dst uint8[out_h][out_w][C] */
EXPORT int yfi_resize_host(const uint8_t* src, int h, int w, int C, long rs, int out_w, int out_h, uint8_t* dst) {
  if (!yfi_image_ok(0, h, w, rs, C, (uint64_t)(h - 1) * (uint64_t)rs + (uint64_t)w * (uint64_t)C) || out_w < 1 || out_h < 1) return -1;
  for (int y = 0; y < out_h; ++y) {
    const yfi_tap ty = yfi_axis_tap(y, out_h, h);
    const uint8_t* r0 = src + (size_t)ty.s0 * (size_t)rs;
    const uint8_t* r1 = src + (size_t)ty.s1 * (size_t)rs;
    for (int x = 0; x < out_w; ++x) {
      const yfi_tap tx = yfi_axis_tap(x, out_w, w);
      for (int c = 0; c < C; ++c) {
        const int32_t h0 = yfi_hpass(r0[tx.s0 * C + c], r0[tx.s1 * C + c], tx.w0, tx.w1);
        const int32_t h1 = yfi_hpass(r1[tx.s0 * C + c], r1[tx.s1 * C + c], tx.w0, tx.w1);
        dst[((size_t)y * out_w + x) * C + c] = (uint8_t)yfi_vpass(h0, h1, ty.w0, ty.w1);
      }
    }
  }
  return 0;
}

/* The suppression's pairwise decision (yf_images_nms.h) over n pairs: a[k], b[k] int32[4] edges (x1, y1, x2, y2), box a the kept one;
 * out[k] = 1 if b survives a at thr.  area[2k], area[2k + 1] = the two areas when `area` is not NULL. */
EXPORT void yfi_nms_pairs_host(const int32_t* a, const int32_t* b, long n, double thr, uint8_t* out, double* area) {
  for (long k = 0; k < n; ++k) {
    const int32_t* p = a + 4 * k;
    const int32_t* q = b + 4 * k;
    const double ap = yfi_nms_area(p[0], p[1], p[2], p[3]), aq = yfi_nms_area(q[0], q[1], q[2], q[3]);
    out[k] = (uint8_t)yfi_nms_survives(p[0], p[1], p[2], p[3], ap, q[0], q[1], q[2], q[3], aq, thr);
    if (area) { area[2 * k] = ap; area[2 * k + 1] = aq; }
  }
}

/* the order key of a record (yfi_nms_key) */
EXPORT uint64_t yfi_nms_key_host(uint32_t conf_bits, uint32_t index) { return yfi_nms_key(conf_bits, index); }

/* ... and with room for an 11-bit index (yfi_nms_key_wide) */
EXPORT uint64_t yfi_nms_key_wide_host(uint32_t conf_bits, uint32_t index) { return yfi_nms_key_wide(conf_bits, index); }

/* The decode of one 20x20 head as decode160_kernel computes it: the byte test q >= q_thr in candidate order (anchor, row, col), the
 * per-candidate record of yf_images_decode160.h for the candidates that fire, the first `cap` written.  Returns the true count. */
EXPORT int yfi_decode160_host(const int8_t* head, int32_t frame, float w_scale, float h_scale, yf_det* dets, int cap) {
  const int q_thr = yfi_d160_q_threshold(yf_sigmoid_bits);
  int n = 0;
  for (int i = 0; i < YF_IMAGES_CAND160; ++i) {
    const int8_t* p = head + yfi_d160_offset(i);
    if (p[4] < q_thr) continue;
    if (n < cap) dets[n] = yfi_d160_candidate(p, i, frame, yf_sigmoid_bits, yf_exp_bits, w_scale, h_scale);
    ++n;
  }
  return n;
}

EXPORT int yfi_decode160_q_threshold_host(void) { return yfi_d160_monotonic(yf_sigmoid_bits) ? yfi_d160_q_threshold(yf_sigmoid_bits) : -129; }

EXPORT int yfi_image_ok_host(uint64_t offset, int64_t h, int64_t w, int64_t rs, int C, uint64_t bytes) {
  return yfi_image_ok(offset, h, w, rs, C, bytes);
}

/* ---- yf_images_float.h ----  the 256 halves of v / 255. */
EXPORT void yfi_f16_of_u8_host(uint16_t* out) {
  for (int v = 0; v < 256; ++v) out[v] = yfi_f16_of_u8(v);
}

EXPORT void yfi_exp_f32_host(const float* x, long n, float* out) {
  for (long k = 0; k < n; ++k) out[k] = yfi_exp_f32(x[k]);
}

EXPORT void yfi_sigmoid_f32_host(const float* x, long n, float* out) {
  for (long k = 0; k < n; ++k) out[k] = yfi_sigmoid_f32(x[k]);
}

/* The decode of one frame's float32 logits [7][7][18] as decode_f32_kernel computes it: candidates in the order (anchor, row, col), the
 * confidence of each, the record of yf_images_float.h for those that fire, the first `cap` written.  Returns the true count. */
EXPORT int yfi_decode_f32_host(const float* logits, int32_t frame, float w_scale, float h_scale, yf_det* dets, int cap) {
  int n = 0;
  for (int i = 0; i < YFI_F32_CAND; ++i) {
    const float* p = logits + yfi_f32_offset(i);
    const float conf = yfi_sigmoid_f32(p[4]);
    if (!(conf > 0.7f)) continue;
    if (n < cap) dets[n] = yfi_f32_candidate(p, i, frame, conf, w_scale, h_scale);
    ++n;
  }
  return n;
}
