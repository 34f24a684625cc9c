/* Host build of the resize arithmetic in yf_images_taps.h, the NV12 / NV21 conversion and addressing in yf_images_yuv.h, the suppression arithmetic in yf_images_nms.h, the 20x20 decode arithmetic in
 * yf_images_decode160.h, the fp16 frames and float32 decode of yf_images_float.h and the scoring arithmetic of yf_images_eval.h (the
 * functions the device kernels call), the tile grid, planner and merge of yf_images_tiles.h the face chips of yf_images_crop.h, the redaction of yf_images_redact.h, the blur of yf_images_blur.h, the drawing of yf_images_draw.h, the tracker of yf_images_track.h, the tracker with a motion model of yf_images_motion.h and its optimal assignment of yf_images_assign.h, the score of tracks against labelled identities of yf_images_score.h, the letterboxed frames and decodes of yf_images_fit.h and the area-averaged frames of yf_images_area.h, for the CPU tests only:
 * libyf_images_host.so, no HIP. */
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "yf_images_taps.h"
#include "yf_images_yuv.h"
#include "yf_images_nms.h"
#include "yf_images_decode160.h"
#include "yf_images_float.h"
#include "yf_images_eval.h"
#include "yf_images_tiles.h"
#include "yf_images_crop.h"
#include "yf_images_redact.h"
#include "yf_images_blur.h"
#include "yf_images_draw.h"
#include "yf_images_track.h"
#include "yf_images_motion.h"
#include "yf_images_assign.h"
#include "yf_images_score.h"
#include "yf_images_describe.h"
#include "yf_images_reid.h"
#include "yf_images_fit.h"
#include "yf_images_area.h"
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

/* ---- yf_images_yuv.h ----  (R, G, B) of n (Y, U, V) triples: yuv uint8[n][3] -> rgb uint8[n][3] */
EXPORT void yfi_yuv_rgb_host(const uint8_t* yuv, long n, uint8_t* rgb) {
  for (long k = 0; k < n; ++k) {
    const int32_t yy = yfi_yuv_luma(yuv[3 * k]);
    const yfi_chroma c = yfi_yuv_chroma(yuv[3 * k + 1], yuv[3 * k + 2]);
    rgb[3 * k] = (uint8_t)yfi_yuv_channel(yy, c.r);
    rgb[3 * k + 1] = (uint8_t)yfi_yuv_channel(yy, c.g);
    rgb[3 * k + 2] = (uint8_t)yfi_yuv_channel(yy, c.b);
  }
}

EXPORT int yfi_yuv_image_ok_host(uint64_t offset_y, uint64_t offset_uv, int64_t h, int64_t w, int64_t stride_y, int64_t stride_uv, uint64_t bytes) {
  return yfi_yuv_image_ok(offset_y, offset_uv, h, w, stride_y, stride_uv, bytes);
}

/* One surface as prepare_yuv_kernel / prepare_yuv_f16_kernel take it: `base` + the descriptor's offsets, checked against `bytes` ->
 * frame int8[out_hw][out_hw][3] (f16 == 0) or the fp16 bits uint16[56][56][3] (f16 != 0), through the header's tap and address
 * functions.  Returns the status the kernel writes: 0, or 1 for an invalid descriptor, whose frame is all -128 (fp16: all 0) and which
 * is never read.  -1: out_hw is not 56 or 160 (fp16: not 56). */
EXPORT int yfi_prepare_yuv_host(const uint8_t* base, uint64_t bytes, const yf_image_yuv* im, int v_first, int out_hw, int f16, void* frame) {
  if (out_hw != 56 && (f16 || out_hw != 160)) return -1;
  const size_t count = (size_t)out_hw * (size_t)out_hw * 3;
  if (!yfi_yuv_image_ok(im->offset_y, im->offset_uv, im->height, im->width, im->stride_y, im->stride_uv, bytes)) {
    if (f16) memset(frame, 0, count * 2); else memset(frame, 0x80, count);
    return 1;
  }
  const uint8_t* yp = base + im->offset_y;
  const uint8_t* uvp = base + im->offset_uv;
  for (int y = 0; y < out_hw; ++y) {
    const yfi_yuv_ytap ty = yfi_yuv_ytap_of(yfi_axis_tap(y, out_hw, im->height), im->stride_y, im->stride_uv);
    for (int x = 0; x < out_hw; ++x) {
      const yfi_yuv_xtap tx = yfi_yuv_xtap_of(yfi_axis_tap(x, out_hw, im->width));
      int32_t rgb[3];
      yfi_yuv_sample(yp, uvp, tx, ty, v_first, rgb);
      for (int c = 0; c < 3; ++c) {
        const size_t at = ((size_t)y * out_hw + x) * 3 + c;
        if (f16) ((uint16_t*)frame)[at] = yfi_f16_of_u8(rgb[c]);
        else ((int8_t*)frame)[at] = (int8_t)(rgb[c] - 128);
      }
    }
  }
  return 0;
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

/* ---- yf_images_eval.h ----  calculate_iou over n pairs: d[k] int32[4] edges of a detection, g[k] double[4] of a ground truth */
EXPORT void yfi_eval_iou_host(const int32_t* d, const double* g, long n, double* out) {
  for (long k = 0; k < n; ++k) out[k] = yfi_eval_iou(d[4 * k], d[4 * k + 1], d[4 * k + 2], d[4 * k + 3], g[4 * k], g[4 * k + 1], g[4 * k + 2], g[4 * k + 3]);
}

/* the order key of a confidence (yfi_eval_key) */
EXPORT uint32_t yfi_eval_key_host(uint32_t conf_bits) { return yfi_eval_key(conf_bits); }

/* order[0 .. m): the positions 0 .. m - 1 sorted by key[], equal keys in input order (least significant byte first, counting); 0 on
 * success */
static int eval_order(const uint32_t* key, long m, int32_t* order) {
  int32_t* tmp = malloc((size_t)(m > 0 ? m : 1) * sizeof *tmp);
  if (!tmp) return -1;
  for (long i = 0; i < m; ++i) order[i] = (int32_t)i;
  for (int shift = 0; shift < 32; shift += 8) {
    long at[257] = {0};
    for (long i = 0; i < m; ++i) ++at[((key[order[i]] >> shift) & 255u) + 1];
    for (int d = 0; d < 256; ++d) at[d + 1] += at[d];
    for (long i = 0; i < m; ++i) tmp[at[(key[order[i]] >> shift) & 255u]++] = order[i];
    memcpy(order, tmp, (size_t)m * sizeof *tmp);
  }
  free(tmp);
  return 0;
}

/* yf_images_match_device as the reference's loop states it: per frame, the records in order (descending conf, earlier slot first), each
 * one's best ground truth, and a set of the claimed ones.  tp[n][cap], best[n][cap] (may be NULL); slots beyond a frame's records are
 * not written.  Returns n, or -1 without memory. */
EXPORT long yfi_eval_match_host(const yf_det* dets, const int32_t* counts, long n, int cap, const yf_gt_box* gt, const int32_t* gt_counts,
                                int gt_cap, double thr, uint8_t* tp, int32_t* best) {
  uint32_t* key = malloc((size_t)cap * sizeof *key);
  int32_t* order = malloc((size_t)cap * sizeof *order);
  uint8_t* claimed = malloc((size_t)gt_cap);
  long rc = n;
  if (!key || !order || !claimed) rc = -1;
  for (long f = 0; rc == n && f < n; ++f) {
    const int m = yfi_eval_clamp(counts[f], cap), k = yfi_eval_clamp(gt_counts[f], gt_cap);
    const yf_det* d = dets + f * cap;
    const yf_gt_box* g = gt + f * gt_cap;
    for (int r = 0; r < m; ++r) { uint32_t u; memcpy(&u, &d[r].conf, 4); key[r] = yfi_eval_key(u); }
    if (eval_order(key, m, order) != 0) { rc = -1; break; }
    memset(claimed, 0, (size_t)gt_cap);
    for (int o = 0; o < m; ++o) {
      const int r = order[o];
      double best_iou = 0.0;
      int b = -1;
      for (int j = 0; j < k; ++j) {
        const double iou = yfi_eval_iou(d[r].x1, d[r].y1, d[r].x2, d[r].y2, g[j].x1, g[j].y1, g[j].x2, g[j].y2);
        if (iou > best_iou) { best_iou = iou; b = j; }
      }
      uint8_t hit = 0;
      if (best_iou >= thr && b >= 0 && !claimed[b]) { claimed[b] = 1; hit = 1; }
      tp[f * cap + r] = hit;
      if (best) best[f * cap + r] = b;
    }
  }
  free(key); free(order); free(claimed);
  return rc;
}

/* yf_images_average_precision_device as the reference states it: the records of the batch in order, the cumulative counts, precision and
 * recall, the envelope from the back, the sum from i = 1.  curve (may be NULL): double[m][2] = (recall, envelope).  Returns n, or -1
 * without memory. */
EXPORT long yfi_eval_ap_host(const yf_det* dets, const int32_t* counts, const uint8_t* tp, long n, int cap, const int32_t* gt_counts, int gt_cap,
                             yf_eval_result* result, double* curve) {
  long m = 0;
  int64_t num_gt = 0;
  for (long f = 0; f < n; ++f) { m += yfi_eval_clamp(counts[f], cap); num_gt += yfi_eval_clamp(gt_counts[f], gt_cap); }
  const size_t room = (size_t)(m > 0 ? m : 1);
  uint32_t* key = malloc(room * sizeof *key);
  uint8_t* flag = malloc(room);
  int32_t* order = malloc(room * sizeof *order);
  double* precision = malloc(room * sizeof *precision);
  double* recall = malloc(room * sizeof *recall);
  long rc = n;
  if (!key || !flag || !order || !precision || !recall) rc = -1;
  if (rc == n) {
    long at = 0;
    for (long f = 0; f < n; ++f)
      for (int r = 0; r < yfi_eval_clamp(counts[f], cap); ++r, ++at) {
        uint32_t u;
        memcpy(&u, &dets[f * cap + r].conf, 4);
        key[at] = yfi_eval_key(u);
        flag[at] = tp[f * cap + r] != 0;
      }
    if (eval_order(key, m, order) != 0) rc = -1;
  }
  if (rc == n) {
    double ctp = 0.0, cfp = 0.0;
    for (long i = 0; i < m; ++i) {
      if (flag[order[i]]) ctp += 1.0; else cfp += 1.0;
      precision[i] = yfi_eval_precision(ctp, cfp);
      recall[i] = yfi_eval_recall(ctp, num_gt);
    }
    for (long i = m - 2; i >= 0; --i) precision[i] = precision[i + 1] > precision[i] ? precision[i + 1] : precision[i];
    double ap = 0.0;
    for (long i = 1; i < m; ++i) ap += (recall[i] - recall[i - 1]) * precision[i];
    if (curve) for (long i = 0; i < m; ++i) { curve[2 * i] = recall[i]; curve[2 * i + 1] = precision[i]; }
    result->ap = ap; result->detections = m; result->ground_truths = num_gt; result->true_positives = (int64_t)ctp;
  }
  free(key); free(flag); free(order); free(precision); free(recall);
  return rc;
}

/* ---- yf_images_tiles.h ----  yf_images_plan_tiles as libyf_images.so exports it (the error text is dropped) */
EXPORT long yfi_plan_tiles_host(const yf_image* images, long n, int format, int tile_h, int tile_w, int stride_y, int stride_x, int whole,
                                yf_tile* tiles, yf_image* tile_images, int32_t* first, long tiles_cap) {
  const char* err;
  return yfi_plan_tiles(images, n, format, tile_h, tile_w, stride_y, stride_x, whole, tiles, tile_images, first, tiles_cap, &err);
}

/* yf_images_gather_tiles_device as yf_images_tiles.h states it: per image its tiles in ascending order, each tile's clamped records in
 * theirs, translated, the first out_cap of them written and the total counted.  As on the device, a range end is clamped to [0, t]
 * first, so a malformed `first` reads and writes inside the buffers.  Returns n, or -1 for arguments the device entry refuses. */
EXPORT long yfi_gather_tiles_host(const yf_det* dets, const int32_t* counts, long t, int cap, const yf_tile* tiles, const int32_t* first,
                                  long n, yf_det* out, int32_t* out_counts, int out_cap) {
  if (n < 0 || t < 0 || cap < 1 || cap > YF_IMAGES_CAND160 || out_cap < 1 || out_cap > YF_IMAGES_NMS_WIDE_MAX_CAP ||
      (uint64_t)t * (uint64_t)cap >= (1ull << 31))
    return -1;
  if (t == 0) return n;
  for (long i = 0; i < n; ++i) {
    const long a = first[i] < 0 ? 0 : (first[i] > t ? t : first[i]), b = first[i + 1] < 0 ? 0 : (first[i + 1] > t ? t : first[i + 1]);
    int64_t total = 0;
    for (long j = a; j < b; ++j) {
      const int m = yfi_tiles_clamp(counts[j], cap);
      for (int r = 0; r < m && total + r < out_cap; ++r) {
        uint32_t w[7];
        memcpy(w, &dets[j * cap + r], sizeof w);
        for (int q = 0; q < 7; ++q) w[q] = yfi_tiles_dword(w[q], q, (int32_t)i, tiles[j].x0, tiles[j].y0);
        memcpy(&out[i * out_cap + total + r], w, sizeof w);
      }
      total += m;
    }
    out_counts[i] = (int32_t)total;
  }
  return n;
}

/* ---- yf_images_crop.h ----  yf_images_crop_records_device / _yuv_device as the header states them: the exclusive prefix of the clamped
 * counts into first[n + 1], then chip by chip the record's region and its resize through the header's tap function, for the chips below
 * chips_cap; chip slots and info rows at and beyond min(total, chips_cap) are not touched.  `images`: yf_image[n] (packed formats) or
 * yf_image_yuv[n] (NV12 / NV21), offsets from `base`, checked against `bytes`.  Returns n, or -1 for arguments the device entries refuse. */
static void crop_packed(const uint8_t* base, const yf_image* im, int C, int src_bgr, int out_bgr, const yf_chip* r, int out_h, int out_w,
                        uint8_t* chip) {
  const int swap = src_bgr != out_bgr;
  for (int y = 0; y < out_h; ++y) {
    const yfi_tap ty = yfi_crop_tap(y, out_h, r->y0, r->height);
    const uint8_t* r0 = base + im->offset + (uint64_t)ty.s0 * (uint64_t)im->row_stride;
    const uint8_t* r1 = base + im->offset + (uint64_t)ty.s1 * (uint64_t)im->row_stride;
    for (int x = 0; x < out_w; ++x) {
      const yfi_tap tx = yfi_crop_tap(x, out_w, r->x0, r->width);
      for (int c = 0; c < 3; ++c) {
        const int sc = swap ? 2 - c : c;
        const int32_t h0 = yfi_hpass(r0[tx.s0 * C + sc], r0[tx.s1 * C + sc], tx.w0, tx.w1);
        const int32_t h1 = yfi_hpass(r1[tx.s0 * C + sc], r1[tx.s1 * C + sc], tx.w0, tx.w1);
        chip[((size_t)y * out_w + x) * 3 + c] = (uint8_t)yfi_vpass(h0, h1, ty.w0, ty.w1);
      }
    }
  }
}

static void crop_yuv(const uint8_t* base, const yf_image_yuv* im, int v_first, int out_bgr, const yf_chip* r, int out_h, int out_w,
                     uint8_t* chip) {
  for (int y = 0; y < out_h; ++y) {
    const yfi_yuv_ytap ty = yfi_yuv_ytap_of(yfi_crop_tap(y, out_h, r->y0, r->height), im->stride_y, im->stride_uv);
    for (int x = 0; x < out_w; ++x) {
      const yfi_yuv_xtap tx = yfi_yuv_xtap_of(yfi_crop_tap(x, out_w, r->x0, r->width));
      int32_t rgb[3];
      yfi_yuv_sample(base + im->offset_y, base + im->offset_uv, tx, ty, v_first, rgb);
      for (int c = 0; c < 3; ++c) chip[((size_t)y * out_w + x) * 3 + c] = (uint8_t)rgb[out_bgr ? 2 - c : c];
    }
  }
}

static long crop_records(const uint8_t* base, uint64_t bytes, int format, const void* images, const yf_det* dets, const int32_t* counts, long n,
                         int cap, int out_h, int out_w, int out_format, int margin_permille, int flags, uint8_t* chips, long chips_cap,
                         int32_t* first, yf_chip* info) {
  if (yfi_crop_check(n, cap, out_h, out_w, out_format, margin_permille, flags, chips_cap) != NULL) return -1;
  if (!dets || !counts || !first || !info || !chips || !base || !images) return -1;
  if (n == 0) return 0;
  const int yuv = format == YF_PIX_NV12 || format == YF_PIX_NV21;
  const int C = yfi_tiles_channels(format), out_bgr = out_format == YF_PIX_BGR8;
  const size_t chip_bytes = (size_t)out_h * (size_t)out_w * 3;
  int64_t k = 0;
  for (long i = 0; i < n; ++i) {
    const int m = yfi_crop_clamp(counts[i], cap);
    first[i] = (int32_t)k;
    for (int s = 0; s < m; ++s, ++k) {
      if (k >= (int64_t)chips_cap) continue;
      const yf_det* d = &dets[i * cap + s];
      uint8_t* chip = chips + (size_t)k * chip_bytes;
      yf_chip r = {(int32_t)i, s, 0, 0, 0, 0, 2};
      if (yuv) {
        const yf_image_yuv* im = (const yf_image_yuv*)images + i;
        if (yfi_yuv_image_ok(im->offset_y, im->offset_uv, im->height, im->width, im->stride_y, im->stride_uv, bytes))
          r.status = yfi_crop_region(d->x1, d->y1, d->x2, d->y2, im->width, im->height, margin_permille, flags, &r);
        if (r.status == 0) crop_yuv(base, im, format == YF_PIX_NV21, out_bgr, &r, out_h, out_w, chip);
      } else {
        const yf_image* im = (const yf_image*)images + i;
        if (yfi_image_ok(im->offset, im->height, im->width, im->row_stride, C, bytes))
          r.status = yfi_crop_region(d->x1, d->y1, d->x2, d->y2, im->width, im->height, margin_permille, flags, &r);
        if (r.status == 0) crop_packed(base, im, C, format == YF_PIX_BGR8 || format == YF_PIX_BGRA8, out_bgr, &r, out_h, out_w, chip);
      }
      if (r.status != 0) memset(chip, 0, chip_bytes);
      info[k] = r;
    }
  }
  first[n] = (int32_t)k;
  return n;
}

EXPORT long yfi_crop_records_host(const uint8_t* base, uint64_t bytes, int format, const yf_image* images, const yf_det* dets,
                                  const int32_t* counts, long n, int cap, int out_h, int out_w, int out_format, int margin_permille, int flags,
                                  uint8_t* chips, long chips_cap, int32_t* first, yf_chip* info) {
  if (!yfi_tiles_channels(format)) return -1;
  return crop_records(base, bytes, format, images, dets, counts, n, cap, out_h, out_w, out_format, margin_permille, flags, chips, chips_cap,
                      first, info);
}

EXPORT long yfi_crop_records_yuv_host(const uint8_t* base, uint64_t bytes, int format, const yf_image_yuv* images, const yf_det* dets,
                                      const int32_t* counts, long n, int cap, int out_h, int out_w, int out_format, int margin_permille,
                                      int flags, uint8_t* chips, long chips_cap, int32_t* first, yf_chip* info) {
  if (format != YF_PIX_NV12 && format != YF_PIX_NV21) return -1;
  return crop_records(base, bytes, format, images, dets, counts, n, cap, out_h, out_w, out_format, margin_permille, flags, chips, chips_cap,
                      first, info);
}

/* the region rule alone: out[5] = {x0, y0, width, height, status} */
EXPORT void yfi_crop_region_host(int32_t x1, int32_t y1, int32_t x2, int32_t y2, int32_t W, int32_t H, int margin_permille, int flags, int32_t* out) {
  yf_chip r;
  const int st = yfi_crop_region(x1, y1, x2, y2, W, H, margin_permille, flags, &r);
  out[0] = r.x0; out[1] = r.y0; out[2] = r.width; out[3] = r.height; out[4] = st;
}

/* ---- yf_images_redact.h ----  yf_images_redact_records_device / _yuv_device as the header states them, in place on the caller's buffer:
 * the exclusive prefix of the clamped counts into first[n + 1], status[n], and picture by picture the mosaic or the fill.  The mosaic
 * states the union literally: a map of the picture's blocks, one byte each, marks the blocks the frame's records touch; then every marked
 * block is read, averaged and written once (blocks do not overlap, so no copy of the source is needed).  `images`: yf_image[n] or
 * yf_image_yuv[n], offsets from `base`, checked against `bytes`.  Returns n, or -1 for arguments the device entries refuse (or no memory
 * for the map). */
static void redact_mean(uint8_t* p, int64_t stride, int rows, int cols, int C, int NC) {
  for (int c = 0; c < NC; ++c) {
    uint32_t sum = 0;
    for (int y = 0; y < rows; ++y)
      for (int x = 0; x < cols; ++x) sum += p[(int64_t)y * stride + (int64_t)x * C + c];
    const uint8_t v = (uint8_t)yfi_redact_mean(sum, (uint32_t)rows * (uint32_t)cols);
    for (int y = 0; y < rows; ++y)
      for (int x = 0; x < cols; ++x) p[(int64_t)y * stride + (int64_t)x * C + c] = v;
  }
}

static void redact_fill(uint8_t* p, int64_t stride, int rows, int cols, int C, int NC, const uint8_t* f) {
  for (int y = 0; y < rows; ++y)
    for (int x = 0; x < cols; ++x)
      for (int c = 0; c < NC; ++c) p[(int64_t)y * stride + (int64_t)x * C + c] = f[c];
}

static long redact_records(uint8_t* base, uint64_t bytes, int format, const void* images, const yf_det* dets, const int32_t* counts, long n,
                           int cap, int mode, int block, uint32_t colour, int margin_permille, int flags, int32_t* first, int32_t* status) {
  if (yfi_redact_check(n, cap, mode, block, colour, margin_permille, flags) != NULL) return -1;
  if (!dets || !counts || !first || !status || !base || !images) return -1;
  if (n == 0) return 0;
  const int yuv = format == YF_PIX_NV12 || format == YF_PIX_NV21;
  const int C = yuv ? 1 : yfi_tiles_channels(format);
  uint8_t f[3];
  yfi_redact_fill_bytes(colour, format, f);
  int64_t total = 0;
  for (long i = 0; i < n; ++i) {
    first[i] = (int32_t)total;
    total += yfi_crop_clamp(counts[i], cap);
  }
  first[n] = (int32_t)total;
  for (long i = 0; i < n; ++i) {
    const int m = yfi_crop_clamp(counts[i], cap);
    const yf_image* im = yuv ? NULL : (const yf_image*)images + i;
    const yf_image_yuv* iy = yuv ? (const yf_image_yuv*)images + i : NULL;
    const int ok = yuv ? yfi_yuv_image_ok(iy->offset_y, iy->offset_uv, iy->height, iy->width, iy->stride_y, iy->stride_uv, bytes)
                       : yfi_image_ok(im->offset, im->height, im->width, im->row_stride, C, bytes);
    status[i] = ok ? 0 : 1;
    if (!ok) continue;
    const int32_t W = yuv ? iy->width : im->width, H = yuv ? iy->height : im->height;
    uint8_t* px = base + (yuv ? iy->offset_y : im->offset);
    uint8_t* uv = yuv ? base + iy->offset_uv : NULL;
    const int64_t rs = yuv ? iy->stride_y : im->row_stride;
    const int nbx = mode == YF_REDACT_MOSAIC ? (W + block - 1) / block : 0, nby = mode == YF_REDACT_MOSAIC ? (H + block - 1) / block : 0;
    uint8_t* set = NULL;
    if (mode == YF_REDACT_MOSAIC && m > 0) {
      set = (uint8_t*)calloc((size_t)nbx * (size_t)nby, 1);
      if (!set) return -1;
    }
    for (int s = 0; s < m; ++s) {
      const yf_det* d = &dets[i * cap + s];
      yf_chip r;
      if (yfi_crop_region(d->x1, d->y1, d->x2, d->y2, W, H, margin_permille, flags, &r) != 0) continue;
      if (mode == YF_REDACT_MOSAIC) {
        const yfi_blocks b = yfi_redact_blocks(&r, block);
        for (int by = b.by0; by <= b.by1; ++by) memset(set + (size_t)by * nbx + b.bx0, 1, (size_t)(b.bx1 - b.bx0 + 1));
      } else if (!yuv) {
        redact_fill(px + (int64_t)r.y0 * rs + (int64_t)r.x0 * C, rs, r.height, r.width, C, 3, f);
      } else {
        const int cx0 = r.x0 >> 1, cx1 = (r.x0 + r.width - 1) >> 1, cy0 = r.y0 >> 1, cy1 = (r.y0 + r.height - 1) >> 1;
        redact_fill(px + (int64_t)r.y0 * rs + r.x0, rs, r.height, r.width, 1, 1, f);
        redact_fill(uv + (int64_t)cy0 * iy->stride_uv + 2 * cx0, iy->stride_uv, cy1 - cy0 + 1, cx1 - cx0 + 1, 2, 2, f + 1);
      }
    }
    if (set) {
      for (int by = 0; by < nby; ++by)
        for (int bx = 0; bx < nbx; ++bx) {
          if (!set[(size_t)by * nbx + bx]) continue;
          int32_t x, w, y, h;
          yfi_redact_span(bx, block, W, &x, &w);
          yfi_redact_span(by, block, H, &y, &h);
          redact_mean(px + (int64_t)y * rs + (int64_t)x * C, rs, h, w, C, yuv ? 1 : 3);
          if (yuv) {
            yfi_redact_chroma_span(bx, block, W, &x, &w);
            yfi_redact_chroma_span(by, block, H, &y, &h);
            redact_mean(uv + (int64_t)y * iy->stride_uv + 2 * x, iy->stride_uv, h, w, 2, 2);
          }
        }
      free(set);
    }
  }
  return n;
}

EXPORT long yfi_redact_records_host(uint8_t* base, uint64_t bytes, int format, const yf_image* images, const yf_det* dets, const int32_t* counts,
                                    long n, int cap, int mode, int block, uint32_t colour, int margin_permille, int flags, int32_t* first,
                                    int32_t* status) {
  if (!yfi_tiles_channels(format)) return -1;
  return redact_records(base, bytes, format, images, dets, counts, n, cap, mode, block, colour, margin_permille, flags, first, status);
}

EXPORT long yfi_redact_records_yuv_host(uint8_t* base, uint64_t bytes, int format, const yf_image_yuv* images, const yf_det* dets,
                                        const int32_t* counts, long n, int cap, int mode, int block, uint32_t colour, int margin_permille,
                                        int flags, int32_t* first, int32_t* status) {
  if (format != YF_PIX_NV12 && format != YF_PIX_NV21) return -1;
  return redact_records(base, bytes, format, images, dets, counts, n, cap, mode, block, colour, margin_permille, flags, first, status);
}

/* the argument check alone: the text of the first fault into out (at most out_bytes, 0-terminated), or an empty text; returns 1 for a fault */
EXPORT int yfi_redact_check_host(long n, int cap, int mode, int block, uint32_t colour, int margin_permille, int flags, char* out, int out_bytes) {
  const char* t = yfi_redact_check(n, cap, mode, block, colour, margin_permille, flags);
  if (out && out_bytes > 0) snprintf(out, (size_t)out_bytes, "%s", t ? t : "");
  return t != NULL;
}

/* ---- yf_images_blur.h ----  yf_images_blur_records_device / _yuv_device as the header states them, in place on the caller's buffer,
 * literally: frame by frame, first the grid of every record with a slot from the picture as it came in (into its slot of `work`), then
 * the records painted from the LAST slot to the first, so that a pixel ends with the value of the lowest slot whose region holds it --
 * that IS the ownership rule; no list of owners.  A record without a slot is painted with the fill's bytes in the same order.  Returns
 * n, or -1 for arguments the device entries refuse (or no memory for a row of taps). */
static void blur_means(const uint8_t* p, int64_t stride, const yf_chip* r, int C, int NC, int gx, int gy, uint8_t* cells, int at) {
  for (int cy = 0; cy < gy; ++cy)
    for (int cx = 0; cx < gx; ++cx) {
      const int32_t xa = yfi_blur_cell_at(cx, r->width, gx), xb = yfi_blur_cell_at(cx + 1, r->width, gx);
      const int32_t ya = yfi_blur_cell_at(cy, r->height, gy), yb = yfi_blur_cell_at(cy + 1, r->height, gy);
      for (int c = 0; c < NC; ++c) {
        uint64_t sum = 0;
        for (int32_t y = ya; y < yb; ++y)
          for (int32_t x = xa; x < xb; ++x) sum += p[(int64_t)(r->y0 + y) * stride + (int64_t)(r->x0 + x) * C + c];
        cells[(cy * gx + cx) * 4 + at + c] = (uint8_t)yfi_blur_mean(sum, (uint64_t)(xb - xa) * (uint64_t)(yb - ya));
      }
    }
}

/* cells == NULL: the fill with f[0 .. NC - 1].  The horizontal taps are worked out once per region (xt: room for r->width taps) */
static void blur_paint(uint8_t* p, int64_t stride, const yf_chip* r, int C, int NC, int gx, int gy, const uint32_t* cells, int at,
                       const uint8_t* f, yfi_tap* xt) {
  for (int32_t x = 0; x < r->width; ++x) xt[x] = yfi_axis_tap(x, r->width, gx);
  for (int32_t y = 0; y < r->height; ++y) {
    const yfi_tap ty = yfi_axis_tap(y, r->height, gy);
    for (int32_t x = 0; x < r->width; ++x) {
      uint8_t* q = p + (int64_t)(r->y0 + y) * stride + (int64_t)(r->x0 + x) * C;
      for (int c = 0; c < NC; ++c) q[c] = cells ? yfi_blur_sample(cells, gx, at + c, xt[x], ty) : f[c];
    }
  }
}

static long blur_records(uint8_t* base, uint64_t bytes, int format, const void* images, const yf_det* dets, const int32_t* counts, long n,
                         int cap, int grid, uint32_t colour, int margin_permille, int flags, void* work, size_t work_bytes, long records_cap,
                         int32_t* first, int32_t* status) {
  if (yfi_blur_check(n, cap, grid, colour, margin_permille, flags, work, work_bytes, records_cap) != NULL) return -1;
  if (!dets || !counts || !first || !status || !base || !images) return -1;
  if (n == 0) return 0;
  const int yuv = format == YF_PIX_NV12 || format == YF_PIX_NV21;
  const int C = yuv ? 1 : yfi_tiles_channels(format);
  uint8_t f[3];
  yfi_redact_fill_bytes(colour, format, f);
  int64_t total = 0;
  for (long i = 0; i < n; ++i) {
    first[i] = (int32_t)total;
    total += yfi_crop_clamp(counts[i], cap);
  }
  first[n] = (int32_t)total;
  for (long i = 0; i < n; ++i) {
    const int m = yfi_crop_clamp(counts[i], cap);
    const yf_image* im = yuv ? NULL : (const yf_image*)images + i;
    const yf_image_yuv* iy = yuv ? (const yf_image_yuv*)images + i : NULL;
    const int ok = yuv ? yfi_yuv_image_ok(iy->offset_y, iy->offset_uv, iy->height, iy->width, iy->stride_y, iy->stride_uv, bytes)
                       : yfi_image_ok(im->offset, im->height, im->width, im->row_stride, C, bytes);
    status[i] = (ok ? 0 : YFI_BLUR_INVALID) | (first[i + 1] > first[i] && (long)first[i + 1] > records_cap ? YFI_BLUR_FILLED : 0);
    if (!ok) continue;
    const int32_t W = yuv ? iy->width : im->width, H = yuv ? iy->height : im->height;
    uint8_t* px = base + (yuv ? iy->offset_y : im->offset);
    uint8_t* uv = yuv ? base + iy->offset_uv : NULL;
    const int64_t rs = yuv ? iy->stride_y : im->row_stride;
    yfi_tap* xt = m > 0 ? (yfi_tap*)malloc((size_t)W * sizeof(yfi_tap)) : NULL;
    if (m > 0 && !xt) return -1;
    for (int pass = 0; pass < 2; ++pass)                      /* every grid from the picture as it came in, then the paint, last slot first */
      for (int s = pass ? m - 1 : 0; pass ? s >= 0 : s < m; s += pass ? -1 : 1) {
        const yf_det* d = &dets[i * cap + s];
        const long k = (long)first[i] + s;
        yf_chip r;
        if (yfi_crop_region(d->x1, d->y1, d->x2, d->y2, W, H, margin_permille, flags, &r) != 0) continue;
        const yf_chip c = yfi_blur_chroma(&r);
        const int gx = yfi_blur_cells(r.width, grid, YF_BLUR_MIN_CELL), gy = yfi_blur_cells(r.height, grid, YF_BLUR_MIN_CELL);
        const int hx = yfi_blur_cells(c.width, grid, YFI_BLUR_MIN_CELL_CHROMA), hy = yfi_blur_cells(c.height, grid, YFI_BLUR_MIN_CELL_CHROMA);
        uint8_t* slot = k < records_cap ? (uint8_t*)work + (size_t)k * (size_t)(grid * grid) * 4u : NULL;
        if (pass == 0 && slot) {
          memset(slot, 0, (size_t)(grid * grid) * 4u);
          blur_means(px, rs, &r, C, yuv ? 1 : 3, gx, gy, slot, 0);
          if (yuv) blur_means(uv, iy->stride_uv, &c, 2, 2, hx, hy, slot, 1);
        } else if (pass == 1) {
          blur_paint(px, rs, &r, C, yuv ? 1 : 3, gx, gy, (const uint32_t*)slot, 0, f, xt);
          if (yuv) blur_paint(uv, iy->stride_uv, &c, 2, 2, hx, hy, (const uint32_t*)slot, 1, f + 1, xt);
        }
      }
    free(xt);
  }
  return n;
}

EXPORT long yfi_blur_records_host(uint8_t* base, uint64_t bytes, int format, const yf_image* images, const yf_det* dets, const int32_t* counts,
                                  long n, int cap, int grid, uint32_t colour, int margin_permille, int flags, void* work, size_t work_bytes,
                                  long records_cap, int32_t* first, int32_t* status) {
  if (!yfi_tiles_channels(format)) return -1;
  return blur_records(base, bytes, format, images, dets, counts, n, cap, grid, colour, margin_permille, flags, work, work_bytes, records_cap,
                      first, status);
}

EXPORT long yfi_blur_records_yuv_host(uint8_t* base, uint64_t bytes, int format, const yf_image_yuv* images, const yf_det* dets,
                                      const int32_t* counts, long n, int cap, int grid, uint32_t colour, int margin_permille, int flags,
                                      void* work, size_t work_bytes, long records_cap, int32_t* first, int32_t* status) {
  if (format != YF_PIX_NV12 && format != YF_PIX_NV21) return -1;
  return blur_records(base, bytes, format, images, dets, counts, n, cap, grid, colour, margin_permille, flags, work, work_bytes, records_cap,
                      first, status);
}

EXPORT size_t yfi_blur_workspace_host(long records_cap, int grid) { return yfi_blur_workspace(records_cap, grid); }

/* the argument check alone, as yfi_redact_check_host */
EXPORT int yfi_blur_check_host(long n, int cap, int grid, uint32_t colour, int margin_permille, int flags, const void* work, size_t work_bytes,
                               long records_cap, char* out, int out_bytes) {
  const char* t = yfi_blur_check(n, cap, grid, colour, margin_permille, flags, work, work_bytes, records_cap);
  if (out && out_bytes > 0) snprintf(out, (size_t)out_bytes, "%s", t ? t : "");
  return t != NULL;
}

/* ---- yf_images_draw.h ----  yf_images_draw_records_device / _yuv_device as the header states them, in place on the caller's buffer,
 * literally: frame by frame, record after record in slot order (that IS the overlap rule), every pixel of the record's outer box inside
 * the picture asked of yfi_draw_covers -- no bands, no ownership.  A surface's drawn pixel writes its Y byte and its chroma pair, so a
 * pair ends with the chroma of the highest slot that draws one of its pixels.  `keys`, `palette`: host memory here.  Returns n, or -1
 * for arguments the device entries refuse. */
static long draw_records(uint8_t* base, uint64_t bytes, int format, const void* images, const yf_det* dets, const int32_t* counts, long n,
                         int cap, int half, uint32_t colour, const uint8_t* keys, int key_stride, const uint32_t* palette, int palette_n,
                         int32_t* first, int32_t* status) {
  if (yfi_draw_check(n, cap, half, colour, keys, key_stride, palette, palette_n) != NULL) return -1;
  if (!dets || !counts || !first || !status || !base || !images) return -1;
  if (n == 0) return 0;
  const int yuv = format == YF_PIX_NV12 || format == YF_PIX_NV21;
  const int C = yuv ? 1 : yfi_tiles_channels(format);
  int64_t total = 0;
  for (long i = 0; i < n; ++i) {
    first[i] = (int32_t)total;
    total += yfi_crop_clamp(counts[i], cap);
  }
  first[n] = (int32_t)total;
  for (long i = 0; i < n; ++i) {
    const int m = yfi_crop_clamp(counts[i], cap);
    const yf_image* im = yuv ? NULL : (const yf_image*)images + i;
    const yf_image_yuv* iy = yuv ? (const yf_image_yuv*)images + i : NULL;
    const int ok = yuv ? yfi_yuv_image_ok(iy->offset_y, iy->offset_uv, iy->height, iy->width, iy->stride_y, iy->stride_uv, bytes)
                       : yfi_image_ok(im->offset, im->height, im->width, im->row_stride, C, bytes);
    status[i] = ok ? 0 : 1;
    if (!ok) continue;
    const int32_t W = yuv ? iy->width : im->width, H = yuv ? iy->height : im->height;
    uint8_t* px = base + (yuv ? iy->offset_y : im->offset);
    uint8_t* uv = yuv ? base + iy->offset_uv : NULL;
    const int64_t rs = yuv ? iy->stride_y : im->row_stride;
    for (int s = 0; s < m; ++s) {
      const yf_det* d = &dets[i * cap + s];
      uint32_t col = colour;
      if (keys) {
        uint32_t key;
        memcpy(&key, keys + (i * (int64_t)cap + s) * (int64_t)key_stride, 4);
        col = yfi_draw_key_colour(key, palette, palette_n);
      }
      uint8_t f[3];
      yfi_redact_fill_bytes(col, format, f);
      const yfi_draw_edges e = yfi_draw_clip(d->x1, d->y1, d->x2, d->y2, half, W, H);
      const yfi_draw_span rows = yfi_draw_span_of(e.ya - half, e.yb + half, H), cols = yfi_draw_span_of(e.xa - half, e.xb + half, W);
      for (int32_t y = rows.at; y < rows.at + rows.n; ++y)
        for (int32_t x = cols.at; x < cols.at + cols.n; ++x) {
          if (!yfi_draw_covers(&e, half, x, y)) continue;
          if (!yuv) {
            for (int c = 0; c < 3; ++c) px[(int64_t)y * rs + (int64_t)x * C + c] = f[c];
          } else {
            px[(int64_t)y * rs + x] = f[0];
            uint8_t* pair = uv + (int64_t)(y >> 1) * iy->stride_uv + 2 * (x >> 1);
            pair[0] = f[1]; pair[1] = f[2];
          }
        }
    }
  }
  return n;
}

EXPORT long yfi_draw_records_host(uint8_t* base, uint64_t bytes, int format, const yf_image* images, const yf_det* dets, const int32_t* counts,
                                  long n, int cap, int half, uint32_t colour, const void* keys, int key_stride, const uint32_t* palette,
                                  int palette_n, int32_t* first, int32_t* status) {
  if (!yfi_tiles_channels(format)) return -1;
  return draw_records(base, bytes, format, images, dets, counts, n, cap, half, colour, (const uint8_t*)keys, key_stride, palette, palette_n, first,
                      status);
}

EXPORT long yfi_draw_records_yuv_host(uint8_t* base, uint64_t bytes, int format, const yf_image_yuv* images, const yf_det* dets,
                                      const int32_t* counts, long n, int cap, int half, uint32_t colour, const void* keys, int key_stride,
                                      const uint32_t* palette, int palette_n, int32_t* first, int32_t* status) {
  if (format != YF_PIX_NV12 && format != YF_PIX_NV21) return -1;
  return draw_records(base, bytes, format, images, dets, counts, n, cap, half, colour, (const uint8_t*)keys, key_stride, palette, palette_n, first,
                      status);
}

/* THE rule alone: the drawn sets of n records (boxes int32[n][4]: x1, y1, x2, y2) in a picture of W x H, out uint8[n][H][W] of 0 / 1 --
 * yfi_draw_clip and yfi_draw_covers, asked for every pixel of the picture */
EXPORT void yfi_draw_masks_host(const int32_t* boxes, long n, int half, int32_t W, int32_t H, uint8_t* out) {
  for (long k = 0; k < n; ++k) {
    const yfi_draw_edges e = yfi_draw_clip(boxes[4 * k], boxes[4 * k + 1], boxes[4 * k + 2], boxes[4 * k + 3], half, W, H);
    for (int32_t y = 0; y < H; ++y)
      for (int32_t x = 0; x < W; ++x) out[((size_t)k * (size_t)H + (size_t)y) * (size_t)W + (size_t)x] = (uint8_t)yfi_draw_covers(&e, half, x, y);
  }
}

/* ... and what the kernels walk instead: per record out[14] = {at, n} of the spans top, bottom, between, across, left, right
 * (yfi_draw_bands_of), then yfi_draw_visible and a 0 */
EXPORT void yfi_draw_bands_host(const int32_t* boxes, long n, int half, int32_t W, int32_t H, int32_t* out) {
  for (long k = 0; k < n; ++k) {
    const yfi_draw_edges e = yfi_draw_clip(boxes[4 * k], boxes[4 * k + 1], boxes[4 * k + 2], boxes[4 * k + 3], half, W, H);
    const yfi_draw_bands b = yfi_draw_bands_of(&e, half, W, H);
    const yfi_draw_span s[6] = {b.top, b.bottom, b.between, b.across, b.left, b.right};
    for (int q = 0; q < 6; ++q) { out[14 * k + 2 * q] = s[q].at; out[14 * k + 2 * q + 1] = s[q].n; }
    out[14 * k + 12] = yfi_draw_visible(&e, half, W, H);
    out[14 * k + 13] = 0;
  }
}

/* the argument check alone: the text of the first fault into out (at most out_bytes, 0-terminated), or an empty text; returns 1 for a fault */
EXPORT int yfi_draw_check_host(long n, int cap, int half, uint32_t colour, const void* keys, int key_stride, const void* palette, int palette_n,
                               char* out, int out_bytes) {
  const char* t = yfi_draw_check(n, cap, half, colour, keys, key_stride, palette, palette_n);
  if (out && out_bytes > 0) snprintf(out, (size_t)out_bytes, "%s", t ? t : "");
  return t != NULL;
}

/* ---- yf_images_track.h, yf_images_motion.h ----  the match of one step, shared by both trackers: box[s] the box an occupied slot s is matched by -> slot_det[s], det_slot[j < m]; -1: none */
static void track_match_host(int32_t (*box)[4], const int* occupied, const yf_det* dets, int m, double match_iou, int* slot_det,
                             int* det_slot) {
  static _Thread_local double iou[YF_TRACK_SLOTS][YF_TRACK_MAX_DETS];
  for (int j = 0; j < m; ++j) det_slot[j] = -1;
  for (int s = 0; s < YF_TRACK_SLOTS; ++s) {
    slot_det[s] = -1;
    if (!occupied[s]) continue;
    const double area_a = yfi_nms_area(box[s][0], box[s][1], box[s][2], box[s][3]);
    for (int j = 0; j < m; ++j) {
      const yf_det* d = &dets[j];
      yfi_track_iou(box[s][0], box[s][1], box[s][2], box[s][3], area_a, d->x1, d->y1, d->x2, d->y2,
                    yfi_nms_area(d->x1, d->y1, d->x2, d->y2), match_iou, &iou[s][j]);              /* 0.0: not eligible */
    }
  }
  for (;;) {
    double best = 0.0;
    int bj = -1, bs = -1;
    for (int j = 0; j < m; ++j) {
      if (det_slot[j] >= 0) continue;
      for (int s = 0; s < YF_TRACK_SLOTS; ++s)
        if (occupied[s] && slot_det[s] < 0 && iou[s][j] > best) { best = iou[s][j]; bj = j; bs = s; }
    }
    if (bj < 0) break;
    det_slot[bj] = bs;
    slot_det[bs] = bj;
  }
}

/* ---- yf_images_assign.h ----  the optimal match of one step, with `track_match_host`'s arguments: the table of weights, then the
 * header's sequential procedure; returns the matching's total weight; `table` (int32[m][64], or NULL) receives the weights */
static int64_t assign_match_host(int32_t (*box)[4], const int* occupied, const yf_det* dets, int m, double match_iou, int* slot_det,
                                 int* det_slot, int32_t* table) {
  static _Thread_local int32_t w[YF_TRACK_MAX_DETS * YF_TRACK_SLOTS];
  for (int s = 0; s < YF_TRACK_SLOTS; ++s) {
    const double area_a = yfi_nms_area(box[s][0], box[s][1], box[s][2], box[s][3]);
    for (int j = 0; j < m; ++j) {
      const yf_det* d = &dets[j];
      double iou;
      const int ok = yfi_track_iou(box[s][0], box[s][1], box[s][2], box[s][3], area_a, d->x1, d->y1, d->x2, d->y2,
                                   yfi_nms_area(d->x1, d->y1, d->x2, d->y2), match_iou, &iou);
      w[j * YF_TRACK_SLOTS + s] = yfi_assign_weight(ok && occupied[s], iou);
    }
  }
  if (table) memcpy(table, w, sizeof(int32_t) * (size_t)m * YF_TRACK_SLOTS);
  return yfi_assign_solve(w, m, slot_det, det_slot);
}

/* ---- yf_images_track.h, yf_images_motion.h, yf_images_assign.h ----  one step of a stream as the headers state it, literally, on
 * either state: mp NULL is the base tracker (yf_track_state, the greedy match on the slot's last record), mp given the tracker with a
 * motion model (yf_track_motion_state, whose slot begins with the base slot: the prediction in front of the match chosen by `assign`,
 * the filter in the update).  The match -- for the greedy one the table of the eligible pairs' IoUs, then round after round the largest
 * entry among the slots and detections still unmatched (a scan in ascending detection, then ascending slot, with a strict comparison: the
 * tie rule) --, the update, the births, and the output by a selection of the smallest (id, slot) not yet emitted.  A free slot's bytes
 * are neither read (but its id) nor written. */
static void track_step_host(void* state, const yf_track_params* p, const yf_track_motion_params* mp, int assign, const yf_det* dets,
                            int32_t count, int cap, int32_t frame, yf_det* out, yf_track_info* info, int32_t* out_count, int out_cap,
                            int32_t* status) {
  const int m = yfi_track_clamp(count, cap);
  int bits = yfi_track_clipped(count, cap) ? YFI_TRACK_ST_CLIPPED : 0;
  int slot_det[YF_TRACK_SLOTS], det_slot[YF_TRACK_MAX_DETS], occupied[YF_TRACK_SLOTS];
  int32_t box[YF_TRACK_SLOTS][4];
  int64_t pp[YF_TRACK_SLOTS][4];
  yf_track* slot[YF_TRACK_SLOTS];                                    /* the base slot, and where there is one its motion model */
  yf_track_motion* mo[YF_TRACK_SLOTS];
  uint32_t* issued = mp ? &((yf_track_motion_state*)state)->issued : &((yf_track_state*)state)->issued;
  for (int s = 0; s < YF_TRACK_SLOTS; ++s) {
    mo[s] = mp ? &((yf_track_motion_state*)state)->slot[s] : NULL;
    slot[s] = mp ? &mo[s]->base : &((yf_track_state*)state)->slot[s];
    const yf_track* k = slot[s];
    const int32_t last[4] = {k->det.x1, k->det.y1, k->det.x2, k->det.y2};
    occupied[s] = k->id != 0;
    for (int e = 0; e < 4; ++e) {
      pp[s][e] = mp && occupied[s] ? yfi_motion_sat(mo[s]->pos[e]) + yfi_motion_sat(mo[s]->vel[e]) : 0;
      box[s][e] = mp ? yfi_motion_box(pp[s][e]) : last[e];
    }
  }
  if (assign == YF_ASSIGN_OPTIMAL) assign_match_host(box, occupied, dets, m, p->match_iou, slot_det, det_slot, NULL);
  else track_match_host(box, occupied, dets, m, p->match_iou, slot_det, det_slot);
  for (int s = 0; s < YF_TRACK_SLOTS; ++s) {
    yf_track* k = slot[s];
    if (!occupied[s]) continue;
    k->age = yfi_track_inc(k->age);
    if (slot_det[s] >= 0) {
      const yf_det* d = &dets[slot_det[s]];
      const int32_t z[4] = {d->x1, d->y1, d->x2, d->y2};
      k->det = *d;
      k->hits = yfi_track_inc(k->hits);
      k->misses = 0;
      for (int e = 0; mp && e < 4; ++e) {
        const int64_t r = 256ll * (int64_t)z[e] - pp[s][e];
        mo[s]->pos[e] = yfi_motion_sat(pp[s][e] + yfi_motion_mul(mp->alpha, r));
        mo[s]->vel[e] = yfi_motion_sat(yfi_motion_sat(mo[s]->vel[e]) + yfi_motion_mul(mp->beta, r));
      }
    } else {
      k->misses = yfi_track_inc(k->misses);
      if (k->misses > p->max_misses) {
        if (mp) memset(mo[s], 0, sizeof *mo[s]);
        else memset(k, 0, sizeof *k);
      } else
        for (int e = 0; mp && e < 4; ++e) {
          mo[s]->pos[e] = yfi_motion_sat(pp[s][e]);
          mo[s]->vel[e] = yfi_motion_mul(mp->damp, yfi_motion_sat(mo[s]->vel[e]));
        }
    }
  }
  int s = 0;
  for (int j = 0; j < m; ++j) {
    if (det_slot[j] >= 0) continue;
    while (s < YF_TRACK_SLOTS && slot[s]->id != 0) ++s;
    if (s == YF_TRACK_SLOTS) { bits |= YFI_TRACK_ST_DROPPED; break; }
    yf_track* k = slot[s];
    const int32_t z[4] = {dets[j].x1, dets[j].y1, dets[j].x2, dets[j].y2};
    *issued = yfi_track_next_id(*issued, 0);
    k->id = *issued; k->hits = 1; k->misses = 0; k->age = 1; k->det = dets[j];
    if (mp) {
      mo[s]->pad = 0;
      for (int e = 0; e < 4; ++e) { mo[s]->pos[e] = 256ll * (int64_t)z[e]; mo[s]->vel[e] = 0; }
    }
  }
  int emitted[YF_TRACK_SLOTS] = {0}, total = 0;
  for (;;) {
    int pick = -1;
    for (int q = 0; q < YF_TRACK_SLOTS; ++q) {
      const yf_track* k = slot[q];
      if (emitted[q] || k->id == 0 || k->hits < p->min_hits) continue;
      if (pick < 0 || k->id < slot[pick]->id) pick = q;
    }
    if (pick < 0) break;
    emitted[pick] = 1;
    if (total < out_cap) {
      const yf_track* k = slot[pick];
      out[total] = k->det;
      out[total].frame = frame;
      if (mp && (k->misses > 0 || mp->smooth != 0)) {                /* pos was written in this step or at an earlier one: within the clamp */
        const int64_t* pos = mo[pick]->pos;
        out[total].x1 = yfi_motion_box(pos[0]); out[total].y1 = yfi_motion_box(pos[1]);
        out[total].x2 = yfi_motion_box(pos[2]); out[total].y2 = yfi_motion_box(pos[3]);
      }
      info[total].id = k->id; info[total].hits = k->hits; info[total].misses = k->misses; info[total].age = k->age;
    }
    ++total;
  }
  *out_count = total;
  if (status) *status = bits;
}

/* a call behind its check, on host memory: stream by stream, step by step; `params` is the entry's own copy.  Returns n */
static long track_run_host(const void* dets, const void* counts, long streams, long steps, int layout, int cap, const yf_track_params* p,
                           const yf_track_motion_params* mp, int assign, void* state, void* out, void* info, void* out_counts, int out_cap,
                           int32_t* status) {
  const size_t state_bytes = mp ? sizeof(yf_track_motion_state) : sizeof(yf_track_state);
  for (long s = 0; s < streams; ++s)
    for (long t = 0; t < steps; ++t) {
      const long f = layout == YF_TRACK_TIME_MAJOR ? t * streams + s : s * steps + t;
      track_step_host((char*)state + (size_t)s * state_bytes, p, mp, assign, (const yf_det*)dets + (size_t)f * (size_t)cap,
                      ((const int32_t*)counts)[f], cap, (int32_t)f, (yf_det*)out + (size_t)f * (size_t)out_cap,
                      (yf_track_info*)info + (size_t)f * (size_t)out_cap, (int32_t*)out_counts + f, out_cap, status ? status + f : NULL);
    }
  return streams * steps;
}

/* ---- yf_images_track.h ----  yf_images_track_device on host memory (`stream` is not used).  Returns n, or -1 for arguments the device
 * entry refuses. */
EXPORT long yf_images_track_host(const void* dets, const void* counts, long streams, long steps, int layout, int cap,
                                 const yf_track_params* params, void* state, void* out, void* info, void* out_counts, int out_cap,
                                 int32_t* status, void* stream) {
  (void)stream;
  if (yfi_track_check(dets, counts, streams, steps, layout, cap, params, state, out, info, out_counts, out_cap, status) != NULL) return -1;
  const yf_track_params p = *params;
  return track_run_host(dets, counts, streams, steps, layout, cap, &p, NULL, YF_ASSIGN_GREEDY, state, out, info, out_counts, out_cap, status);
}

/* the argument check alone: the text of the first fault into text (at most text_bytes, 0-terminated), or an empty text; returns 1 for a fault */
EXPORT int yfi_track_check_host(const void* dets, const void* counts, long streams, long steps, int layout, int cap,
                                const yf_track_params* params, const void* state, const void* out, const void* info, const void* out_counts,
                                int out_cap, const void* status, char* text, int text_bytes) {
  const char* t = yfi_track_check(dets, counts, streams, steps, layout, cap, params, state, out, info, out_counts, out_cap, status);
  if (text && text_bytes > 0) snprintf(text, (size_t)text_bytes, "%s", t ? t : "");
  return t != NULL;
}

EXPORT size_t yf_images_track_state_bytes_host(long streams) { return streams > 0 ? (size_t)streams * sizeof(yf_track_state) : 0; }

/* ---- yf_images_motion.h ----  yf_images_track_motion_device on host memory: the contract of the entry above */
EXPORT long yf_images_track_motion_host(const void* dets, const void* counts, long streams, long steps, int layout, int cap,
                                        const yf_track_motion_params* params, void* state, void* out, void* info, void* out_counts,
                                        int out_cap, int32_t* status, void* stream) {
  (void)stream;
  if (yfi_motion_check(dets, counts, streams, steps, layout, cap, params, state, out, info, out_counts, out_cap, status) != NULL) return -1;
  const yf_track_motion_params p = *params;
  return track_run_host(dets, counts, streams, steps, layout, cap, &p.base, &p, YF_ASSIGN_GREEDY, state, out, info, out_counts, out_cap, status);
}

EXPORT int yfi_motion_check_host(const void* dets, const void* counts, long streams, long steps, int layout, int cap,
                                 const yf_track_motion_params* params, const void* state, const void* out, const void* info,
                                 const void* out_counts, int out_cap, const void* status, char* text, int text_bytes) {
  const char* t = yfi_motion_check(dets, counts, streams, steps, layout, cap, params, state, out, info, out_counts, out_cap, status);
  if (text && text_bytes > 0) snprintf(text, (size_t)text_bytes, "%s", t ? t : "");
  return t != NULL;
}

EXPORT size_t yf_images_track_motion_state_bytes_host(long streams) { return streams > 0 ? (size_t)streams * sizeof(yf_track_motion_state) : 0; }

/* ---- yf_images_assign.h ----  yf_images_track_motion_assign_device as the header states it, on host memory: the entry above with
 * the match chosen by `assign` */
EXPORT long yf_images_track_motion_assign_host(const void* dets, const void* counts, long streams, long steps, int layout, int cap,
                                               const yf_track_motion_params* params, int assign, void* state, void* out, void* info,
                                               void* out_counts, int out_cap, int32_t* status, void* stream) {
  (void)stream;
  if (yfi_assign_check(dets, counts, streams, steps, layout, cap, params, assign, state, out, info, out_counts, out_cap, status) != NULL) return -1;
  const yf_track_motion_params p = *params;
  return track_run_host(dets, counts, streams, steps, layout, cap, &p.base, &p, assign, state, out, info, out_counts, out_cap, status);
}

EXPORT int yfi_assign_check_host(const void* dets, const void* counts, long streams, long steps, int layout, int cap,
                                 const yf_track_motion_params* params, int assign, const void* state, const void* out, const void* info,
                                 const void* out_counts, int out_cap, const void* status, char* text, int text_bytes) {
  const char* t = yfi_assign_check(dets, counts, streams, steps, layout, cap, params, assign, state, out, info, out_counts, out_cap, status);
  if (text && text_bytes > 0) snprintf(text, (size_t)text_bytes, "%s", t ? t : "");
  return t != NULL;
}

/* the match alone: boxes int32[64][4] of the slots, occupied int[64], dets yf_det[m], m <= 64 -> slot_det int[64], det_slot int[m] (-1:
 * none); returns the total weight.  With weights (int32[m][64], or NULL) the table is written too. */
EXPORT int64_t yfi_assign_match_host(const int32_t* boxes, const int* occupied, const void* dets, int m, double match_iou, int* slot_det,
                                     int* det_slot, int32_t* weights) {
  int32_t box[YF_TRACK_SLOTS][4];
  memcpy(box, boxes, sizeof box);
  return assign_match_host(box, occupied, (const yf_det*)dets, m, match_iou, slot_det, det_slot, weights);
}

/* the procedure alone on a table of weights int32[m][64] */
EXPORT int64_t yfi_assign_solve_host(const int32_t* weights, int m, int* slot_det, int* det_slot) { return yfi_assign_solve(weights, m, slot_det, det_slot); }

/* ---- yf_images_score.h ----  yf_images_score_tracks_device as the header states it, on host memory (`stream` is not used): the
 * header's sequential step, stream by stream.  Returns n, or -1 for arguments the device entry refuses. */
EXPORT long yf_images_score_tracks_host(const void* out, const void* info, const void* out_counts, int out_cap, const void* gt,
                                        const void* gt_counts, int gt_cap, long streams, long steps, int layout, double score_iou, void* state,
                                        int32_t* match, int32_t* status, void* stream) {
  (void)stream;
  if (yfi_score_check(out, info, out_counts, out_cap, gt, gt_counts, gt_cap, streams, steps, layout, score_iou, state, match, status) != NULL) return -1;
  return yfi_score_run(out, info, out_counts, out_cap, gt, gt_counts, gt_cap, streams, steps, layout, score_iou, state, match, status);
}

EXPORT int yfi_score_check_host(const void* out, const void* info, const void* out_counts, int out_cap, const void* gt, const void* gt_counts,
                                int gt_cap, long streams, long steps, int layout, double score_iou, const void* state, const void* match,
                                const void* status, char* text, int text_bytes) {
  const char* t = yfi_score_check(out, info, out_counts, out_cap, gt, gt_counts, gt_cap, streams, steps, layout, score_iou, state, match, status);
  if (text && text_bytes > 0) snprintf(text, (size_t)text_bytes, "%s", t ? t : "");
  return t != NULL;
}

EXPORT size_t yf_images_score_state_bytes_host(long streams) { return streams > 0 ? (size_t)streams * sizeof(yf_score_state) : 0; }

/* yf_images_score_summary as libyf_images.so exports it (the error text is dropped): the header's body */
EXPORT int yf_images_score_summary_host(const void* host_states, long streams, yf_score_summary* out) { return yfi_score_summary(host_states, streams, out); }

/* ---- yf_images_describe.h ----  yf_images_describe_records_device / _yuv_device as the header states them, on host memory: the
 * header's check and the header's run.  Returns n, or -1 for arguments the device entries refuse. */
EXPORT long yfi_describe_records_host(const uint8_t* base, uint64_t bytes, int format, const yf_image* images, const yf_det* dets,
                                      const int32_t* counts, long n, int cap, int margin_permille, int flags, yf_face_desc* desc, int32_t* first,
                                      int32_t* status) {
  if (!yfi_tiles_channels(format)) return -1;
  if (yfi_describe_check(base, images, dets, counts, n, cap, margin_permille, flags, desc, first, status) != NULL) return -1;
  return yfi_describe_run(base, bytes, format, images, dets, counts, n, cap, margin_permille, flags, desc, first, status);
}

EXPORT long yfi_describe_records_yuv_host(const uint8_t* base, uint64_t bytes, int format, const yf_image_yuv* images, const yf_det* dets,
                                          const int32_t* counts, long n, int cap, int margin_permille, int flags, yf_face_desc* desc,
                                          int32_t* first, int32_t* status) {
  if (format != YF_PIX_NV12 && format != YF_PIX_NV21) return -1;
  if (yfi_describe_check(base, images, dets, counts, n, cap, margin_permille, flags, desc, first, status) != NULL) return -1;
  return yfi_describe_run(base, bytes, format, images, dets, counts, n, cap, margin_permille, flags, desc, first, status);
}

/* the argument check alone, as yfi_redact_check_host */
EXPORT int yfi_describe_check_host(const void* pixels, const void* images, const void* dets, const void* counts, long n, int cap,
                                   int margin_permille, int flags, const void* desc, const void* first, const void* status, char* out,
                                   int out_bytes) {
  const char* t = yfi_describe_check(pixels, images, dets, counts, n, cap, margin_permille, flags, desc, first, status);
  if (out && out_bytes > 0) snprintf(out, (size_t)out_bytes, "%s", t ? t : "");
  return t != NULL;
}

/* ---- yf_images_reid.h ----  yf_images_reid_device as the header states it, on host memory (`stream` is not used): the header's check
 * and the header's step, stream by stream.  Returns n, or -1 for arguments the device entry refuses. */
EXPORT long yf_images_reid_host(const void* info, const void* out_counts, const void* desc, int out_cap, long streams, long steps, int layout,
                                const yf_reid_params* params, void* state, void* info_out, int32_t* what, int32_t* status, void* stream) {
  (void)stream;
  if (yfi_reid_check(info, out_counts, desc, out_cap, streams, steps, layout, params, state, info_out, what, status) != NULL) return -1;
  return yfi_reid_run(info, out_counts, desc, out_cap, streams, steps, layout, params, state, info_out, what, status);
}

EXPORT int yfi_reid_check_host(const void* info, const void* out_counts, const void* desc, int out_cap, long streams, long steps, int layout,
                               const yf_reid_params* params, const void* state, const void* info_out, const void* what, const void* status,
                               char* text, int text_bytes) {
  const char* t = yfi_reid_check(info, out_counts, desc, out_cap, streams, steps, layout, params, state, info_out, what, status);
  if (text && text_bytes > 0) snprintf(text, (size_t)text_bytes, "%s", t ? t : "");
  return t != NULL;
}

EXPORT size_t yf_images_reid_state_bytes_host(long streams) { return streams > 0 ? (size_t)streams * sizeof(yf_reid_state) : 0; }

EXPORT int32_t yfi_reid_distance_host(const uint8_t* a, const uint8_t* b) { return yfi_reid_distance(a, b); }

/* the filter's helpers as they are (no range check: the tests ask for what the definition gives) */
EXPORT int64_t yfi_motion_mul_host(int32_t g, int64_t v) { return yfi_motion_mul(g, v); }
EXPORT int32_t yfi_motion_box_host(int64_t p) { return yfi_motion_box(p); }
EXPORT int64_t yfi_motion_sat_host(int64_t v) { return yfi_motion_sat(v); }

/* ---- yf_images_fit.h ----  out[4] = {x0, y0, width, height} of a picture of h x w in a frame of side S (no range check: the tests
 * ask for what the definition gives) */
EXPORT void yfi_fit_host(int64_t h, int64_t w, int64_t S, int32_t* out) {
  const yf_fit f = yfi_fit_of(h, w, S);
  out[0] = f.x0; out[1] = f.y0; out[2] = f.width; out[3] = f.height;
}

static void fit_store(void* frame, size_t at, int f16, int32_t v) {
  if (f16) ((uint16_t*)frame)[at] = yfi_f16_of_u8(v);
  else ((int8_t*)frame)[at] = (int8_t)(v - 128);
}

/* One packed picture as yffit::frames_kernel takes it: `base` + the descriptor's offset, checked against `bytes` -> frame
 * int8[out_hw][out_hw][3] (f16 == 0) or the fp16 bits uint16[56][56][3], through yfi_fit_of and yfi_fit_tap; a padded pixel reads nothing.
 * Returns the status the kernel writes: 0, or 1 for an invalid descriptor, whose frame is all -128 (fp16: all 0) and which is never
 * read.  -1: the format is not a packed one, out_hw is not 56 or 160 (fp16: not 56), or pad is outside [0, 255]. */
EXPORT int yfi_prepare_fit_host(const uint8_t* base, uint64_t bytes, int format, const yf_image* im, int out_hw, int pad, int f16, void* frame) {
  const int C = yfi_tiles_channels(format), bgr = format == YF_PIX_BGR8 || format == YF_PIX_BGRA8;
  if (!C || (out_hw != 56 && (f16 || out_hw != 160)) || pad < 0 || pad > 255) return -1;
  const size_t count = (size_t)out_hw * (size_t)out_hw * 3;
  if (!yfi_image_ok(im->offset, im->height, im->width, im->row_stride, C, bytes)) {
    if (f16) memset(frame, 0, count * 2); else memset(frame, 0x80, count);
    return 1;
  }
  const yf_fit fit = yfi_fit_of(im->height, im->width, out_hw);
  const uint8_t* px = base + im->offset;
  for (int y = 0; y < out_hw; ++y) {
    const yfi_tap ty = yfi_fit_tap(y, fit.y0, fit.height, im->height);
    for (int x = 0; x < out_hw; ++x) {
      const yfi_tap tx = yfi_fit_tap(x, fit.x0, fit.width, im->width);
      for (int c = 0; c < 3; ++c) {
        const size_t at = ((size_t)y * out_hw + x) * 3 + c;
        if ((tx.w0 | ty.w0) < 0) { fit_store(frame, at, f16, pad); continue; }
        const uint8_t* r0 = px + (uint64_t)ty.s0 * (uint64_t)im->row_stride;
        const uint8_t* r1 = px + (uint64_t)ty.s1 * (uint64_t)im->row_stride;
        const int sc = bgr ? 2 - c : c;
        const int32_t h0 = yfi_hpass(r0[tx.s0 * C + sc], r0[tx.s1 * C + sc], tx.w0, tx.w1);
        const int32_t h1 = yfi_hpass(r1[tx.s0 * C + sc], r1[tx.s1 * C + sc], tx.w0, tx.w1);
        fit_store(frame, at, f16, yfi_vpass(h0, h1, ty.w0, ty.w1));
      }
    }
  }
  return 0;
}

/* ... and one NV12 / NV21 surface as yffit::frames_yuv_kernel takes it (yfi_prepare_yuv_host with the fit) */
EXPORT int yfi_prepare_fit_yuv_host(const uint8_t* base, uint64_t bytes, const yf_image_yuv* im, int v_first, int out_hw, int pad, int f16,
                                    void* frame) {
  if ((out_hw != 56 && (f16 || out_hw != 160)) || pad < 0 || pad > 255) return -1;
  const size_t count = (size_t)out_hw * (size_t)out_hw * 3;
  if (!yfi_yuv_image_ok(im->offset_y, im->offset_uv, im->height, im->width, im->stride_y, im->stride_uv, bytes)) {
    if (f16) memset(frame, 0, count * 2); else memset(frame, 0x80, count);
    return 1;
  }
  const yf_fit fit = yfi_fit_of(im->height, im->width, out_hw);
  const uint8_t* yp = base + im->offset_y;
  const uint8_t* uvp = base + im->offset_uv;
  for (int y = 0; y < out_hw; ++y) {
    const yfi_tap fy = yfi_fit_tap(y, fit.y0, fit.height, im->height);
    const yfi_yuv_ytap ty = yfi_yuv_ytap_of(fy, im->stride_y, im->stride_uv);
    for (int x = 0; x < out_hw; ++x) {
      const yfi_tap fx = yfi_fit_tap(x, fit.x0, fit.width, im->width);
      int32_t rgb[3] = {pad, pad, pad};
      if ((fx.w0 | fy.w0) >= 0) yfi_yuv_sample(yp, uvp, yfi_yuv_xtap_of(fx), ty, v_first, rgb);
      for (int c = 0; c < 3; ++c) fit_store(frame, ((size_t)y * out_hw + x) * 3 + c, f16, rgb[c]);
    }
  }
  return 0;
}

/* The decode of one int8 head (7x7 at out_hw 56, 20x20 at 160) of a picture of height x width as yffit::decode56_kernel /
 * decode160_kernel compute it, with the compiled-in tables: candidates in the order (anchor, row, col), conf > 0.7f (at 160 the byte test
 * against yfi_d160_q_threshold, which says the same for a monotonic table), the record of yfi_fit_candidate for those that fire, the first
 * `cap` written.  status != 0 or a side outside [1, 16384]: 0 records.  Returns the true count, or -1 for another out_hw. */
EXPORT int yfi_decode_fit_host(const int8_t* head, int32_t frame, int32_t height, int32_t width, int32_t status, int out_hw, yf_det* dets,
                               int cap) {
  if (out_hw != 56 && out_hw != 160) return -1;
  if (!yfi_fit_sides_ok(height, width) || status != 0) return 0;
  const int G = out_hw / 8, q_thr = yfi_d160_q_threshold(yf_sigmoid_bits);
  const yfi_fit_map m = yfi_fit_map_of(height, width, out_hw);
  int n = 0;
  for (int i = 0; i < 3 * G * G; ++i) {
    const int8_t* p = head + yfi_fit_offset(i, G);
    if (out_hw == 56 ? !(yfi_d160_bits(yf_sigmoid_bits[p[4] + 128]) > 0.7f) : p[4] < q_thr) continue;
    if (n < cap) dets[n] = yfi_fit_candidate(p, i, G, frame, yf_sigmoid_bits, yf_exp_bits, m);
    ++n;
  }
  return n;
}

/* ... and of one frame's float32 logits [7][7][18] as yffit::decode_f32_kernel computes it */
EXPORT int yfi_decode_f32_fit_host(const float* logits, int32_t frame, int32_t height, int32_t width, int32_t status, yf_det* dets, int cap) {
  if (!yfi_fit_sides_ok(height, width) || status != 0) return 0;
  const yfi_fit_map m = yfi_fit_map_of(height, width, 56);
  int n = 0;
  for (int i = 0; i < YFI_F32_CAND; ++i) {
    const float* p = logits + yfi_fit_offset(i, 7);
    const float conf = yfi_sigmoid_f32(p[4]);
    if (!(conf > 0.7f)) continue;
    if (n < cap) dets[n] = yfi_fit_candidate_f32(p, i, frame, conf, m);
    ++n;
  }
  return n;
}

/* the argument checks alone, as the entry points make them: what 0 a prepare (yuv: the entry's family, f16: fp16 frames), what 1 a
 * decode (f16: float32 logits; a: the heads, pad and format are not used).  The text of the first fault into out (at most out_bytes,
 * 0-terminated), or an empty text; returns 1 for a fault */
EXPORT int yfi_fit_check_host(int what, int yuv, int f16, const void* a, int format, const void* images, long n, int out_hw, int pad,
                              const void* frames_or_dets, const void* status, const void* counts, int cap, char* out, int out_bytes) {
  const char* t = what == 0 ? yfi_fit_check_prepare(yuv, f16, a, format, images, n, out_hw, pad, frames_or_dets, status)
                            : yfi_fit_check_decode(f16, a, images, status, n, out_hw, frames_or_dets, counts, cap);
  if (out && out_bytes > 0) snprintf(out, (size_t)out_bytes, "%s", t ? t : "");
  return t != NULL;
}

/* ---- yf_images_area.h ----  out[0] = a(d, s) on an axis of n_in sources and n_out outputs, out[1], out[2] = the first and the last
 * source of d (no range check: the tests ask for what the definition gives) */
EXPORT void yfi_area_weight_host(int32_t d, int32_t s, int32_t n_in, int32_t n_out, int32_t* out) {
  out[0] = yfi_area_weight(d, s, n_in, n_out);
  out[1] = yfi_area_first(d, n_in, n_out);
  out[2] = yfi_area_last(d, n_in, n_out);
}

/* a whole axis: for every d in [0, n_out) its first and last source and the sum of a(d, s) over them, through yfi_area_span_of and
 * yfi_area_span_weight as the kernels take them; returns the number of d whose neighbours outside the span (first - 1, last + 1) do
 * not weigh 0, or whose span disagrees with yfi_area_weight */
EXPORT int yfi_area_axis_host(int32_t n_in, int32_t n_out, int32_t* firsts, int32_t* lasts, int64_t* sums) {
  int bad = 0;
  for (int32_t d = 0; d < n_out; ++d) {
    const yfi_area_span a = yfi_area_span_of(d, n_in, n_out);
    int64_t sum = 0;
    for (int32_t s = a.first; s <= a.last; ++s) {
      sum += yfi_area_span_weight(a, s);
      bad += yfi_area_span_weight(a, s) != yfi_area_weight(d, s, n_in, n_out);
    }
    bad += a.first > 0 && yfi_area_weight(d, a.first - 1, n_in, n_out) != 0;
    bad += a.last + 1 < n_in && yfi_area_weight(d, a.last + 1, n_in, n_out) != 0;
    firsts[d] = a.first; lasts[d] = a.last; sums[d] = sum;
  }
  return bad;
}

EXPORT int yfi_area_bands_host(long n, int out_hw) { return yfi_area_bands(n, out_hw); }
EXPORT int yfi_area_band_row_host(int b, int bands, int out_hw) { return yfi_area_band_row(b, bands, out_hw); }

/* The frame of one picture whose pixel (sy, sx) has the RGB bytes `pixel` gives: output pixel by output pixel, source row by source
 * row, the definition as it is written -- nothing of the kernel's staging. */
typedef void (*area_pixel_fn)(const void* ctx, int sy, int sx, int32_t rgb[3]);

static void area_frame(const void* ctx, area_pixel_fn pixel, int h, int w, int out_hw, int fit, int pad, int f16, void* frame) {
  const yf_fit r = yfi_area_rect(h, w, out_hw, fit);
  const uint64_t D = (uint64_t)h * (uint64_t)w;
  for (int y = 0; y < out_hw; ++y) {
    for (int x = 0; x < out_hw; ++x) {
      const size_t at = ((size_t)y * out_hw + x) * 3;
      if (y < r.y0 || y >= r.y0 + r.height || x < r.x0 || x >= r.x0 + r.width) {
        for (int c = 0; c < 3; ++c) fit_store(frame, at + c, f16, pad);
        continue;
      }
      const int dy = y - r.y0, dx = x - r.x0;
      uint64_t S[3] = {0, 0, 0};
      for (int sy = yfi_area_first(dy, h, r.height); sy <= yfi_area_last(dy, h, r.height); ++sy) {
        uint32_t row[3] = {0, 0, 0};
        for (int sx = yfi_area_first(dx, w, r.width); sx <= yfi_area_last(dx, w, r.width); ++sx) {
          int32_t rgb[3];
          pixel(ctx, sy, sx, rgb);
          const uint32_t ax = (uint32_t)yfi_area_weight(dx, sx, w, r.width);
          for (int c = 0; c < 3; ++c) row[c] += ax * (uint32_t)rgb[c];
        }
        const uint64_t ay = (uint64_t)yfi_area_weight(dy, sy, h, r.height);
        for (int c = 0; c < 3; ++c) S[c] += ay * row[c];
      }
      for (int c = 0; c < 3; ++c) fit_store(frame, at + c, f16, yfi_area_round(S[c], D));
    }
  }
}

typedef struct area_packed { const uint8_t* px; int64_t rs; int C, bgr; } area_packed;
static void area_packed_pixel(const void* ctx, int sy, int sx, int32_t rgb[3]) {
  const area_packed* p = (const area_packed*)ctx;
  const uint8_t* s = p->px + (uint64_t)sy * (uint64_t)p->rs + (size_t)sx * p->C;
  for (int c = 0; c < 3; ++c) rgb[c] = s[p->bgr ? 2 - c : c];
}

typedef struct area_planes { const uint8_t* y; const uint8_t* uv; int64_t sy, suv; int v_first; } area_planes;
static void area_planes_pixel(const void* ctx, int sy, int sx, int32_t rgb[3]) {
  const area_planes* p = (const area_planes*)ctx;
  const int32_t yy = yfi_yuv_luma(p->y[(uint64_t)sy * (uint64_t)p->sy + sx]);
  const yfi_chroma k = yfi_yuv_pair(p->uv + (uint64_t)(sy >> 1) * (uint64_t)p->suv + (sx >> 1) * 2, p->v_first);
  rgb[0] = yfi_yuv_channel(yy, k.r); rgb[1] = yfi_yuv_channel(yy, k.g); rgb[2] = yfi_yuv_channel(yy, k.b);
}

static int area_args_ok(int out_hw, int fit, int pad, int f16) {
  return (out_hw == 56 || (!f16 && out_hw == 160)) && (fit == YF_FIT_STRETCH || fit == YF_FIT_LETTERBOX) && pad >= 0 && pad <= 255;
}

/* One packed picture as yfarea::area_kernel takes it: `base` + the descriptor's offset, checked against `bytes` -> frame
 * int8[out_hw][out_hw][3] (f16 == 0) or the fp16 bits uint16[56][56][3].  Returns the status the kernel writes: 0, or 1 for an invalid
 * descriptor, whose frame is all -128 (fp16: all 0) and which is never read.  -1: the format is not a packed one, out_hw is not 56 or 160
 * (fp16: not 56), fit is not one of the two, or pad is outside [0, 255]. */
EXPORT int yfi_prepare_area_host(const uint8_t* base, uint64_t bytes, int format, const yf_image* im, int out_hw, int fit, int pad, int f16,
                                 void* frame) {
  const int C = yfi_tiles_channels(format);
  if (!C || !area_args_ok(out_hw, fit, pad, f16)) return -1;
  const size_t count = (size_t)out_hw * (size_t)out_hw * 3;
  if (!yfi_image_ok(im->offset, im->height, im->width, im->row_stride, C, bytes)) {
    if (f16) memset(frame, 0, count * 2); else memset(frame, 0x80, count);
    return 1;
  }
  const area_packed p = {base + im->offset, im->row_stride, C, format == YF_PIX_BGR8 || format == YF_PIX_BGRA8};
  area_frame(&p, area_packed_pixel, im->height, im->width, out_hw, fit, pad, f16, frame);
  return 0;
}

/* ... and one NV12 / NV21 surface: every source pixel converted, then averaged */
EXPORT int yfi_prepare_area_yuv_host(const uint8_t* base, uint64_t bytes, const yf_image_yuv* im, int v_first, int out_hw, int fit, int pad,
                                     int f16, void* frame) {
  if (!area_args_ok(out_hw, fit, pad, f16)) return -1;
  const size_t count = (size_t)out_hw * (size_t)out_hw * 3;
  if (!yfi_yuv_image_ok(im->offset_y, im->offset_uv, im->height, im->width, im->stride_y, im->stride_uv, bytes)) {
    if (f16) memset(frame, 0, count * 2); else memset(frame, 0x80, count);
    return 1;
  }
  const area_planes p = {base + im->offset_y, base + im->offset_uv, im->stride_y, im->stride_uv, v_first};
  area_frame(&p, area_planes_pixel, im->height, im->width, out_hw, fit, pad, f16, frame);
  return 0;
}

/* the argument checks alone, as the entry points make them: the text of the first fault into out (at most out_bytes, 0-terminated), or
 * an empty text; returns 1 for a fault */
EXPORT int yfi_area_check_host(int yuv, int f16, const void* pixels, int format, const void* images, long n, int out_hw, int fit, int pad,
                               const void* frames, const void* status, char* out, int out_bytes) {
  const char* t = yfi_area_check_prepare(yuv, f16, pixels, format, images, n, out_hw, fit, pad, frames, status);
  if (out && out_bytes > 0) snprintf(out, (size_t)out_bytes, "%s", t ? t : "");
  return t != NULL;
}
