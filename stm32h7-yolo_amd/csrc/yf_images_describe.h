/* Appearance descriptors: a yf_face_desc per detection record -- the record's region of its picture as an 8 x 8 grid of mean luma
 * (yf_images_describe_records_device, yf_images_describe_records_yuv_device), shared by the device kernels (yf_images_describe.hip.h),
 * the host entries in yf_images.hip, a host build (yf_images_host.c, which tests/test_reid_host.py checks against ptq.describe_u8 and
 * ptq.describe_yuv420sp) and the sanitizer program tests/csrc/reid_sanitize_main.c.  Plain C.
 *
 * The reference has no such step; the definition is the library's own.  THE DESCRIPTOR IS A TINY TEMPLATE, NOT A LEARNED EMBEDDING: it
 * tells two faces apart as far as their coarse pattern of light and dark differs, no further.  The re-identification that consumes it
 * (yf_images_reid.h) takes any 64 bytes, so a caller with a recogniser behind the chips can hand over its own embedding quantised to
 * uint8 in the place of this one.
 *
 * Records, regions, pictures: exactly the blur's (yf_images_blur.h).  Of frame i the first m_i = yfi_crop_clamp(count, cap) records
 * count; a record's region is yfi_crop_region (margin, YF_CROP_SQUARE, clamp); the picture of frame i is descriptor i, checked with
 * yfi_image_ok / yfi_yuv_image_ok.  The pictures are only read.
 *
 * Output: d_desc yf_face_desc[n][cap]; the record in slot s of frame f goes to d_desc[f][s].  Only the slots of the first m_f records of
 * a frame are written; the slots beyond them are not touched.
 *
 * A record's descriptor is INVALID -- all 68 bytes zero -- when the record has no region, when the region is narrower or lower than
 * YF_DESC_GRID = 8 pixels, or when the picture's descriptor is invalid.
 *
 * A valid descriptor has flags = YF_DESC_VALID.  The region is cut into 8 x 8 cells with the blur's cell bounds, yfi_blur_cell_at(c,
 * side, 8): no cell is empty, since the side is at least 8.  v[cy * 8 + cx] is the cell's mean luma in exact 64-bit integers:
 *   packed formats: S = the sum over the cell's pixels of 77 R + 150 G + 29 B, v = (S + 128 cnt) / (256 cnt) (yfi_describe_luma); R, G
 *                   and B sit where the format keeps them (yfi_describe_weight), and the fourth byte of BGRA / RGBA is never read;
 *   NV12 / NV21:    v = yfi_blur_mean(the sum of Y, cnt); only the Y plane is read.
 * The weights add up to 256, so a grey pixel (R = G = B) has its own value as luma and v <= 255.
 *
 * d_first int32[n + 1] and d_status int32[n] are written as the redaction writes them: the exclusive prefix of the m_i, and
 * YFI_DESCRIBE_INVALID (1) for a frame whose picture descriptor is invalid. */
#ifndef YF_IMAGES_DESCRIBE_H
#define YF_IMAGES_DESCRIBE_H
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include "../../include/yf_images.h"
#include "yf_images_yuv.h"
#include "yf_images_crop.h"
#include "yf_images_blur.h"

#define YFI_DESCRIBE_INVALID 1
#define YFI_DESC_WORDS 17               /* sizeof(yf_face_desc) / 4 */

#ifdef __cplusplus
static_assert(sizeof(yf_face_desc) == 68 && sizeof(yf_face_desc) == 4 * YFI_DESC_WORDS && YF_DESC_BYTES == YF_DESC_GRID * YF_DESC_GRID,
              "the layout include/yf_images.h states");
#else
_Static_assert(sizeof(yf_face_desc) == 68 && sizeof(yf_face_desc) == 4 * YFI_DESC_WORDS && YF_DESC_BYTES == YF_DESC_GRID * YF_DESC_GRID,
               "the layout include/yf_images.h states");
#endif

/* the luma weight of colour byte ch (0, 1, 2) of a packed pixel; bgr: the format keeps blue first (YF_PIX_BGR8, YF_PIX_BGRA8) */
YFI_HD uint32_t yfi_describe_weight(int ch, int bgr) { return ch == 1 ? 150u : ((ch == 0) == (bgr != 0) ? 29u : 77u); }

/* THE mean luma of a cell of packed pixels: S the weighted sum, cnt the pixels */
YFI_HD uint32_t yfi_describe_luma(uint64_t S, uint64_t cnt) { return (uint32_t)((S + 128u * cnt) / (256u * cnt)); }

/* 1 for a region that has a descriptor */
YFI_HD int yfi_describe_region_ok(const yf_chip* r) { return r->width >= YF_DESC_GRID && r->height >= YF_DESC_GRID; }

/* 1 for a format whose first colour byte is blue */
YFI_HD int yfi_describe_bgr(int format) { return format == YF_PIX_BGR8 || format == YF_PIX_BGRA8; }

/* THE descriptor of one region of one plane, sequentially.  p: the plane's first byte; C: bytes per pixel (1: the Y plane); bgr as above */
static inline void yfi_describe_region(const uint8_t* p, int64_t stride, const yf_chip* r, int C, int bgr, yf_face_desc* out) {
  out->flags = YF_DESC_VALID;
  for (int cy = 0; cy < YF_DESC_GRID; ++cy)
    for (int cx = 0; cx < YF_DESC_GRID; ++cx) {
      const int32_t xa = yfi_blur_cell_at(cx, r->width, YF_DESC_GRID), xb = yfi_blur_cell_at(cx + 1, r->width, YF_DESC_GRID);
      const int32_t ya = yfi_blur_cell_at(cy, r->height, YF_DESC_GRID), yb = yfi_blur_cell_at(cy + 1, r->height, YF_DESC_GRID);
      const uint64_t cnt = (uint64_t)(xb - xa) * (uint64_t)(yb - ya);
      uint64_t sum = 0;
      for (int32_t y = ya; y < yb; ++y)
        for (int32_t x = xa; x < xb; ++x) {
          const uint8_t* q = p + (int64_t)(r->y0 + y) * stride + (int64_t)(r->x0 + x) * C;
          if (C == 1) sum += q[0];
          else sum += (uint64_t)(yfi_describe_weight(0, bgr) * q[0] + yfi_describe_weight(1, bgr) * q[1] + yfi_describe_weight(2, bgr) * q[2]);
        }
      out->v[cy * YF_DESC_GRID + cx] = (uint8_t)(C == 1 ? yfi_blur_mean(sum, cnt) : yfi_describe_luma(sum, cnt));
    }
}

/* what the host can see of a call's arguments, in the order the entry points check them (the format's family comes first, in the entry
 * itself); NULL, or the text of the first fault */
static inline const char* yfi_describe_check(const void* pixels, const void* images, const void* dets, const void* counts, long n, int cap,
                                             int margin_permille, int flags, const void* desc, const void* first, const void* status) {
  if (n < 0 || n > 2147483646l) return "n must be in [0, 2^31 - 2]";
  if (cap < 1 || cap > YF_IMAGES_NMS_WIDE_MAX_CAP) return "cap must be in [1, 1200]";
  if ((uint64_t)n * (uint64_t)cap >= (1ull << 31)) return "n * cap must be below 2^31";
  if (margin_permille < 0 || margin_permille > 1000) return "margin_permille must be in [0, 1000]";
  if ((flags & ~YF_CROP_SQUARE) != 0) return "flags must be 0 or YF_CROP_SQUARE";
  if (!dets || !counts || !desc || !first || !status) return "d_dets, d_counts, d_desc, d_first or d_status is NULL";
  if ((((uintptr_t)dets | (uintptr_t)counts | (uintptr_t)desc | (uintptr_t)first | (uintptr_t)status) & 3) != 0)
    return "d_dets, d_counts, d_desc, d_first and d_status must be 4-byte aligned";
  if (!pixels) return "d_pixels is NULL";
  if (!images || ((uintptr_t)images & 7) != 0) return "d_images is NULL or not 8-byte aligned";
  return NULL;
}

/* a call behind its checks, on host memory: the scan, the status, then record by record.  format: any of the six.  Returns n */
static inline long yfi_describe_run(const uint8_t* base, uint64_t bytes, int format, const void* images, const yf_det* dets, const int32_t* counts,
                                    long n, int cap, int margin_permille, int flags, yf_face_desc* desc, int32_t* first, int32_t* status) {
  const int yuv = format == YF_PIX_NV12 || format == YF_PIX_NV21;
  const int C = yuv ? 1 : (format == YF_PIX_BGRA8 || format == YF_PIX_RGBA8 ? 4 : 3);
  int64_t total = 0;
  if (n == 0) return 0;                                                /* nothing is written, as nothing is launched */
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
    status[i] = ok ? 0 : YFI_DESCRIBE_INVALID;
    for (int s = 0; s < m; ++s) {
      yf_face_desc* out = desc + (size_t)i * (size_t)cap + (size_t)s;
      const yf_det* d = &dets[(size_t)i * (size_t)cap + (size_t)s];
      yf_chip r;
      memset(out, 0, sizeof *out);
      if (!ok) continue;
      if (yfi_crop_region(d->x1, d->y1, d->x2, d->y2, yuv ? iy->width : im->width, yuv ? iy->height : im->height, margin_permille, flags, &r) != 0)
        continue;
      if (!yfi_describe_region_ok(&r)) continue;
      yfi_describe_region(base + (yuv ? iy->offset_y : im->offset), yuv ? iy->stride_y : im->row_stride, &r, C, yfi_describe_bgr(format), out);
    }
  }
  return n;
}

#endif
