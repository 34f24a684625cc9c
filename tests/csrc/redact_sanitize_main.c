/* The host build of the redaction (csrc/yf_images_redact.h through csrc/yf_images_host.c) under ASan + UBSan: a program of its own,
 * compiled together with yf_images_host.c by tests/test_redact_sanitize.py.  Every packed picture, and every Y plane and UV plane of a
 * surface, is an allocation of exactly its extent ((rows - 1) * stride + width * C bytes), handed over as one base with offsets, so a load
 * or a store one byte before or past a picture is a report.  It runs the designed boxes of tests/crops_support.py -- a box well inside,
 * the whole picture, a 1 x 1 box, boxes overhanging each side and a corner, a box wholly outside, x1 > x2, y1 > y2, INT32_MIN / INT32_MAX
 * edges -- and boxes at the last pixel with odd origins; frames with count 0, a count above cap and a negative count; pictures of 37 x 53,
 * 64 x 48, 1 x 1 and 410 x 362 (surfaces: the even sizes next to them), every format, the mosaic at every block size and the fill,
 * margins 0, 250 and 1000, square on and off, packed and padded strides; and invalid descriptors over memory that has been freed, which
 * must be neither read nor written.  Each frame has a picture of its own. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/yf_images.h"

long yfi_redact_records_host(uint8_t* base, uint64_t bytes, int format, const yf_image* images, const yf_det* dets, const int32_t* counts,
                             long n, int cap, int mode, int block, uint32_t colour, int margin_permille, int flags, int32_t* first,
                             int32_t* status);
long yfi_redact_records_yuv_host(uint8_t* base, uint64_t bytes, int format, const yf_image_yuv* images, const yf_det* dets,
                                 const int32_t* counts, long n, int cap, int mode, int block, uint32_t colour, int margin_permille, int flags,
                                 int32_t* first, int32_t* status);

static uint32_t g_seed = 5353u;
static uint32_t rnd(void) { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

#define CHECK(c) do { if (!(c)) { printf("redact: FAILED %s (line %d)\n", #c, __LINE__); exit(1); } } while (0)

static uint8_t* exact(size_t bytes) {
  uint8_t* p = malloc(bytes);
  CHECK(p);
  for (size_t i = 0; i < bytes; ++i) p[i] = (uint8_t)rnd();
  return p;
}

enum { CAP = 18, FRAMES = 4, DESIGNED = 16 };

/* frame 0: the 16 designed records; frame 1: count 0; frame 2: a count above cap, all cap records present; frame 3: a negative count */
static void records(int w, int h, yf_det* dets, int32_t* counts) {
  const int32_t b[DESIGNED][4] = {
      {w / 4, h / 4, 3 * w / 4, 3 * h / 4}, {0, 0, w - 1, h - 1}, {w / 2, h / 2, w / 2, h / 2},
      {-w / 3 - 2, h / 4, w / 2, h / 2}, {w / 2, h / 4, w + 5, h / 2}, {w / 4, -7, w / 2, h / 2}, {w / 4, h / 2, w / 2, h + 9},
      {-5, -6, w / 3, h / 3}, {w + 3, h + 3, w + 10, h + 12}, {w / 2, 0, w / 2 - 1, h - 1}, {0, h / 2, w - 1, h / 2 - 2},
      {INT32_MIN, INT32_MIN, INT32_MAX, INT32_MAX}, {INT32_MIN, h / 4, w / 2, INT32_MAX},
      {w - 1, h - 1, w - 1, h - 1}, {w - 3, h - 5, w - 1, h - 1}, {1, 1, 3, 3}};
  memset(dets, 0xA5, sizeof(yf_det) * FRAMES * CAP);
  for (int f = 0; f < FRAMES; f += 2)
    for (int s = 0; s < (f == 0 ? DESIGNED : CAP); ++s) {
      yf_det* d = &dets[f * CAP + s];
      if (f == 0) { d->x1 = b[s][0]; d->y1 = b[s][1]; d->x2 = b[s][2]; d->y2 = b[s][3]; }
      else { d->x1 = (int32_t)(rnd() % (uint32_t)w) - 3; d->y1 = (int32_t)(rnd() % (uint32_t)h) - 3; d->x2 = d->x1 + (int32_t)(rnd() % 50u); d->y2 = d->y1 + (int32_t)(rnd() % 50u); }
    }
  counts[0] = DESIGNED; counts[1] = 0; counts[2] = CAP + 100; counts[3] = -2;
}

static const int BLOCKS[6] = {4, 8, 16, 32, 64, 0};                 /* 0: the fill */
static const int MARGINS[3] = {0, 250, 1000};

static void check_run(long rc, const int32_t* first, const int32_t* status, int want_status) {
  CHECK(rc == FRAMES);
  CHECK(first[0] == 0 && first[1] == DESIGNED && first[2] == DESIGNED && first[3] == DESIGNED + CAP && first[4] == DESIGNED + CAP);
  for (int f = 0; f < FRAMES; ++f) CHECK(status[f] == want_status);
}

static void packed_case(int w, int h, int format, int pad) {
  const int C = format >= 2 ? 4 : 3;
  const int64_t rs = (int64_t)w * C + pad;
  const size_t ext = (size_t)(h - 1) * (size_t)rs + (size_t)w * C;
  uint8_t* px[FRAMES];
  uint8_t* base = NULL;
  yf_image im[FRAMES];
  for (int f = 0; f < FRAMES; ++f) {
    px[f] = exact(ext);
    if (!base || px[f] < base) base = px[f];
  }
  uint64_t bytes = 0;
  for (int f = 0; f < FRAMES; ++f) {
    im[f].offset = (uint64_t)((uintptr_t)px[f] - (uintptr_t)base); im[f].height = h; im[f].width = w; im[f].row_stride = rs;
    if (im[f].offset + ext > bytes) bytes = im[f].offset + ext;
  }
  yf_det dets[FRAMES * CAP];
  int32_t counts[FRAMES], first[FRAMES + 1], status[FRAMES];
  records(w, h, dets, counts);
  uint8_t* keep1 = malloc(ext);
  uint8_t* keep3 = malloc(ext);
  CHECK(keep1 && keep3);
  memcpy(keep1, px[1], ext); memcpy(keep3, px[3], ext);
  for (int k = 0; k < 6; ++k)
    for (int m = 0; m < 3; ++m)
      for (int flags = 0; flags < 2; ++flags) {
        const int mode = BLOCKS[k] ? YF_REDACT_MOSAIC : YF_REDACT_FILL;
        check_run(yfi_redact_records_host(base, bytes, format, im, dets, counts, FRAMES, CAP, mode, BLOCKS[k], 0x00C82D5Au, MARGINS[m], flags,
                                          first, status), first, status, 0);
        if (mode == YF_REDACT_FILL) {                               /* record 1 is the whole picture: every pixel carries the colour */
          const uint8_t* p = px[0] + (size_t)(h - 1) * (size_t)rs + (size_t)(w - 1) * C;
          CHECK(p[1] == 0x2D && p[0] == (format == YF_PIX_BGR8 || format == YF_PIX_BGRA8 ? 0x5A : 0xC8));
        }
      }
  CHECK(memcmp(keep1, px[1], ext) == 0 && memcmp(keep3, px[3], ext) == 0);   /* the frames whose counts are 0 and -2 */
  free(keep1); free(keep3);
  /* invalid descriptors over freed memory: one byte less of buffer, a stride below the row, a side of 0 -- status 1, no access */
  for (int f = 0; f < FRAMES; ++f) free(px[f]);
  CHECK(ext >= 1);
  for (int f = 0; f < FRAMES; ++f) im[f].offset = bytes - ext;
  check_run(yfi_redact_records_host(base, bytes - 1, format, im, dets, counts, FRAMES, CAP, YF_REDACT_MOSAIC, 8, 0, 250, 1, first, status), first,
            status, 1);
  for (int f = 0; f < FRAMES; ++f) im[f].row_stride = (int64_t)w * C - 1;
  check_run(yfi_redact_records_host(base, UINT64_MAX, format, im, dets, counts, FRAMES, CAP, YF_REDACT_FILL, 0, 0, 0, 0, first, status), first,
            status, 1);
  for (int f = 0; f < FRAMES; ++f) { im[f].row_stride = rs; im[f].height = 0; }
  check_run(yfi_redact_records_host(base, UINT64_MAX, format, im, dets, counts, FRAMES, CAP, YF_REDACT_MOSAIC, 64, 0, 0, 0, first, status), first,
            status, 1);
}

static void yuv_case(int w, int h, int format, int pad_y, int pad_uv) {
  const int64_t sy = w + pad_y, suv = w + pad_uv;
  const size_t ext_y = (size_t)(h - 1) * (size_t)sy + (size_t)w, ext_uv = (size_t)(h / 2 - 1) * (size_t)suv + (size_t)w;
  uint8_t* y[FRAMES];
  uint8_t* uv[FRAMES];
  uint8_t* base = NULL;
  for (int f = 0; f < FRAMES; ++f) {
    y[f] = exact(ext_y); uv[f] = exact(ext_uv);
    if (!base || y[f] < base) base = y[f];
    if (uv[f] < base) base = uv[f];
  }
  yf_image_yuv im[FRAMES];
  uint64_t bytes = 0;
  for (int f = 0; f < FRAMES; ++f) {
    im[f].offset_y = (uint64_t)((uintptr_t)y[f] - (uintptr_t)base); im[f].offset_uv = (uint64_t)((uintptr_t)uv[f] - (uintptr_t)base);
    im[f].height = h; im[f].width = w; im[f].stride_y = sy; im[f].stride_uv = suv;
    if (im[f].offset_y + ext_y > bytes) bytes = im[f].offset_y + ext_y;
    if (im[f].offset_uv + ext_uv > bytes) bytes = im[f].offset_uv + ext_uv;
  }
  yf_det dets[FRAMES * CAP];
  int32_t counts[FRAMES], first[FRAMES + 1], status[FRAMES];
  records(w, h, dets, counts);
  for (int k = 0; k < 6; ++k)
    for (int m = 0; m < 3; ++m)
      for (int flags = 0; flags < 2; ++flags) {
        const int mode = BLOCKS[k] ? YF_REDACT_MOSAIC : YF_REDACT_FILL;
        check_run(yfi_redact_records_yuv_host(base, bytes, format, im, dets, counts, FRAMES, CAP, mode, BLOCKS[k], 0x00C82D5Au, MARGINS[m], flags,
                                              first, status), first, status, 0);
        if (mode == YF_REDACT_FILL) {
          const uint8_t* p = uv[0] + (size_t)(h / 2 - 1) * (size_t)suv + (size_t)(w - 2);
          CHECK(y[0][ext_y - 1] == 0xC8 && p[0] == (format == YF_PIX_NV21 ? 0x5A : 0x2D) && p[1] == (format == YF_PIX_NV21 ? 0x2D : 0x5A));
        }
      }
  for (int f = 0; f < FRAMES; ++f) { free(y[f]); free(uv[f]); }
  for (int f = 0; f < FRAMES; ++f) im[f].width = w - 1;                                    /* an odd side */
  check_run(yfi_redact_records_yuv_host(base, UINT64_MAX, format, im, dets, counts, FRAMES, CAP, YF_REDACT_MOSAIC, 4, 0, 0, 0, first, status),
            first, status, 1);
  for (int f = 0; f < FRAMES; ++f) { im[f].width = w; im[f].offset_uv = bytes - ext_uv; }
  check_run(yfi_redact_records_yuv_host(base, bytes - 1, format, im, dets, counts, FRAMES, CAP, YF_REDACT_FILL, 0, 0, 0, 0, first, status), first,
            status, 1);
}

int main(void) {
  const int sizes[4][2] = {{37, 53}, {64, 48}, {1, 1}, {410, 362}};                       /* (W, H) */
  const int even[4][2] = {{38, 54}, {64, 48}, {2, 2}, {410, 362}};
  for (int k = 0; k < 4; ++k)
    for (int format = 0; format < 4; ++format) {
      packed_case(sizes[k][0], sizes[k][1], format, 0);
      packed_case(sizes[k][0], sizes[k][1], format, 5);
    }
  for (int k = 0; k < 4; ++k)
    for (int format = YF_PIX_NV12; format <= YF_PIX_NV21; ++format) {
      yuv_case(even[k][0], even[k][1], format, 0, 0);
      yuv_case(even[k][0], even[k][1], format, 3, 6);
    }
  /* arguments the entries refuse: nothing is touched (the pointers are NULL) */
  CHECK(yfi_redact_records_host(NULL, 0, 0, NULL, NULL, NULL, 1, 1, YF_REDACT_MOSAIC, 12, 0, 0, 0, NULL, NULL) == -1);
  CHECK(yfi_redact_records_host(NULL, 0, 0, NULL, NULL, NULL, 1, 1, YF_REDACT_FILL, 8, 0, 0, 0, NULL, NULL) == -1);
  CHECK(yfi_redact_records_host(NULL, 0, 0, NULL, NULL, NULL, 1, 1, YF_REDACT_FILL, 0, 0x01000000u, 0, 0, NULL, NULL) == -1);
  CHECK(yfi_redact_records_host(NULL, 0, 0, NULL, NULL, NULL, 1, 1, YF_REDACT_MOSAIC, 8, 0, 1001, 0, NULL, NULL) == -1);
  CHECK(yfi_redact_records_host(NULL, 0, YF_PIX_NV12, NULL, NULL, NULL, 1, 1, YF_REDACT_MOSAIC, 8, 0, 0, 0, NULL, NULL) == -1);
  CHECK(yfi_redact_records_yuv_host(NULL, 0, YF_PIX_BGR8, NULL, NULL, NULL, 1, 1, YF_REDACT_MOSAIC, 8, 0, 0, 0, NULL, NULL) == -1);
  printf("redact: ok\n");
  return 0;
}
