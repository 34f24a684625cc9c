/* The host build of the face chips (csrc/yf_images_crop.h through csrc/yf_images_host.c) under ASan + UBSan: a program of its own, compiled
 * together with yf_images_host.c by tests/test_crops_sanitize.py.  Every packed picture, and every Y plane and UV plane of a surface, is an
 * allocation of exactly its extent ((rows - 1) * stride + width * C bytes), handed over as one base with offsets, so an index one byte
 * before or past a picture is a report.  It runs the designed records of tests/crops_support.py -- a box well inside, the whole picture, a
 * 1 x 1 box, boxes overhanging each side and a corner, a box wholly outside, x1 > x2, y1 > y2, INT32_MIN / INT32_MAX edges; frames with
 * count 0, a count above cap and a negative count -- on pictures of 37 x 53, 64 x 48, 1 x 1 and 410 x 362 (surfaces: the even sizes next to
 * them), every format, both byte orders, three chip sizes, margins 0, 250 and 1000, square on and off, packed and padded strides; and
 * invalid descriptors over memory that has been freed, which must not be read. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/yf_images.h"

long yfi_crop_records_host(const uint8_t* base, uint64_t bytes, int format, const yf_image* images, const yf_det* dets, const int32_t* counts,
                           long n, int cap, int out_h, int out_w, int out_format, int margin_permille, int flags, uint8_t* chips,
                           long chips_cap, int32_t* first, yf_chip* info);
long yfi_crop_records_yuv_host(const uint8_t* base, uint64_t bytes, int format, const yf_image_yuv* images, const yf_det* dets,
                               const int32_t* counts, long n, int cap, int out_h, int out_w, int out_format, int margin_permille, int flags,
                               uint8_t* chips, long chips_cap, int32_t* first, yf_chip* info);

static uint32_t g_seed = 4242u;
static uint32_t rnd(void) { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

#define CHECK(c) do { if (!(c)) { printf("crop: FAILED %s (line %d)\n", #c, __LINE__); exit(1); } } while (0)

static uint8_t* exact(size_t bytes) {
  uint8_t* p = malloc(bytes);
  CHECK(p);
  for (size_t i = 0; i < bytes; ++i) p[i] = (uint8_t)rnd();
  return p;
}

enum { CAP = 15, FRAMES = 4, DESIGNED = 13 };

/* frame 0: the 13 designed records; frame 1: count 0; frame 2: a count above cap, all cap records present; frame 3: a negative count */
static void records(int w, int h, yf_det* dets, int32_t* counts) {
  const int32_t b[DESIGNED][4] = {
      {w / 4, h / 4, 3 * w / 4, 3 * h / 4}, {0, 0, w - 1, h - 1}, {w / 2, h / 2, w / 2, h / 2},
      {-w / 3 - 2, h / 4, w / 2, h / 2}, {w / 2, h / 4, w + 5, h / 2}, {w / 4, -7, w / 2, h / 2}, {w / 4, h / 2, w / 2, h + 9},
      {-5, -6, w / 3, h / 3}, {w + 3, h + 3, w + 10, h + 12}, {w / 2, 0, w / 2 - 1, h - 1}, {0, h / 2, w - 1, h / 2 - 2},
      {INT32_MIN, INT32_MIN, INT32_MAX, INT32_MAX}, {INT32_MIN, h / 4, w / 2, INT32_MAX}};
  memset(dets, 0xA5, sizeof(yf_det) * FRAMES * CAP);
  for (int f = 0; f < FRAMES; f += 2)
    for (int s = 0; s < (f == 0 ? DESIGNED : CAP); ++s) {
      yf_det* d = &dets[f * CAP + s];
      if (s < DESIGNED) { d->x1 = b[s][0]; d->y1 = b[s][1]; d->x2 = b[s][2]; d->y2 = b[s][3]; }
      else { d->x1 = (int32_t)(rnd() % (uint32_t)w) - 3; d->y1 = (int32_t)(rnd() % (uint32_t)h) - 3; d->x2 = d->x1 + (int32_t)(rnd() % 50u); d->y2 = d->y1 + (int32_t)(rnd() % 50u); }
    }
  counts[0] = DESIGNED; counts[1] = 0; counts[2] = CAP + 100; counts[3] = -2;
}

static const int OUTS[3][2] = {{16, 16}, {112, 112}, {32, 48}};
static const int MARGINS[3] = {0, 250, 1000};

/* what every run must show: the prefix, and per chip a region inside the picture or an all-zero chip */
static void check_run(long rc, const int32_t* first, const yf_chip* info, const uint8_t* chips, size_t chip_bytes, int w, int h, int want_status2) {
  CHECK(rc == FRAMES);
  CHECK(first[0] == 0 && first[1] == DESIGNED && first[2] == DESIGNED && first[3] == DESIGNED + CAP && first[4] == DESIGNED + CAP);
  for (int k = 0; k < DESIGNED + CAP; ++k) {
    const yf_chip* c = &info[k];
    CHECK(c->frame == (k < DESIGNED ? 0 : 2) && c->slot == (k < DESIGNED ? k : k - DESIGNED));
    if (want_status2) CHECK(c->status == 2);
    if (c->status == 0) {
      CHECK(c->x0 >= 0 && c->y0 >= 0 && c->width >= 1 && c->height >= 1 && c->x0 + c->width <= w && c->y0 + c->height <= h);
    } else {
      CHECK(c->x0 == 0 && c->y0 == 0 && c->width == 0 && c->height == 0);
      for (size_t q = 0; q < chip_bytes; ++q) CHECK(chips[(size_t)k * chip_bytes + q] == 0);
    }
  }
  if (!want_status2) {
    CHECK(info[0].status == 0 && info[1].status == 0 && info[1].width == w && info[1].height == h && info[2].width >= 1 && info[2].width <= 3);
    CHECK(info[9].status == 1 && info[10].status == 1);            /* (a margin can bring the box outside, record 8, back in) */
  }
}

static void packed_case(int w, int h, int format, int pad) {
  const int C = format >= 2 ? 4 : 3;
  const int64_t rs = (int64_t)w * C + pad;
  const size_t ext = (size_t)(h - 1) * (size_t)rs + (size_t)w * C;
  uint8_t* px = exact(ext);
  yf_image im[FRAMES];
  for (int f = 0; f < FRAMES; ++f) { im[f].offset = 0; im[f].height = h; im[f].width = w; im[f].row_stride = rs; }
  yf_det dets[FRAMES * CAP];
  int32_t counts[FRAMES], first[FRAMES + 1];
  yf_chip info[DESIGNED + CAP];
  records(w, h, dets, counts);
  for (int o = 0; o < 3; ++o)
    for (int m = 0; m < 3; ++m)
      for (int flags = 0; flags < 2; ++flags) {
        const size_t chip_bytes = (size_t)OUTS[o][0] * OUTS[o][1] * 3;
        uint8_t* chips = exact(chip_bytes * (DESIGNED + CAP));
        const long rc = yfi_crop_records_host(px, ext, format, im, dets, counts, FRAMES, CAP, OUTS[o][0], OUTS[o][1], (o + m + flags) & 1,
                                              MARGINS[m], flags, chips, DESIGNED + CAP, first, info);
        check_run(rc, first, info, chips, chip_bytes, w, h, 0);
        free(chips);
      }
  /* a cut inside frame 2: chips and info rows beyond it are not written (they do not exist here) */
  {
    const size_t chip_bytes = 16 * 16 * 3;
    uint8_t* chips = exact(chip_bytes * (DESIGNED + 2));
    yf_chip* few = malloc(sizeof(yf_chip) * (DESIGNED + 2));
    CHECK(few);
    CHECK(yfi_crop_records_host(px, ext, format, im, dets, counts, FRAMES, CAP, 16, 16, 1, 0, 0, chips, DESIGNED + 2, first, few) == FRAMES);
    CHECK(first[FRAMES] == DESIGNED + CAP && few[DESIGNED + 1].frame == 2 && few[DESIGNED + 1].slot == 1);
    free(few); free(chips);
  }
  /* invalid descriptors over freed memory: one byte less of buffer, a stride below the row, a side of 0 -- status 2, zeros, no read */
  free(px);
  const size_t chip_bytes = 16 * 16 * 3;
  uint8_t* chips = exact(chip_bytes * (DESIGNED + CAP));
  CHECK(ext >= 1);
  check_run(yfi_crop_records_host(px, ext - 1, format, im, dets, counts, FRAMES, CAP, 16, 16, 1, 250, 1, chips, DESIGNED + CAP, first, info),
            first, info, chips, chip_bytes, w, h, 1);
  for (int f = 0; f < FRAMES; ++f) im[f].row_stride = (int64_t)w * C - 1;
  check_run(yfi_crop_records_host(px, UINT64_MAX, format, im, dets, counts, FRAMES, CAP, 16, 16, 1, 0, 0, chips, DESIGNED + CAP, first, info),
            first, info, chips, chip_bytes, w, h, 1);
  for (int f = 0; f < FRAMES; ++f) { im[f].row_stride = rs; im[f].height = 0; }
  check_run(yfi_crop_records_host(px, UINT64_MAX, format, im, dets, counts, FRAMES, CAP, 16, 16, 0, 0, 0, chips, DESIGNED + CAP, first, info),
            first, info, chips, chip_bytes, w, h, 1);
  free(chips);
}

static void yuv_case(int w, int h, int format, int pad_y, int pad_uv) {
  const int64_t sy = w + pad_y, suv = w + pad_uv;
  const size_t ext_y = (size_t)(h - 1) * (size_t)sy + (size_t)w, ext_uv = (size_t)(h / 2 - 1) * (size_t)suv + (size_t)w;
  uint8_t* y = exact(ext_y);
  uint8_t* uv = exact(ext_uv);
  const uint8_t* base = y < uv ? y : uv;
  yf_image_yuv im[FRAMES];
  for (int f = 0; f < FRAMES; ++f) {
    im[f].offset_y = (uint64_t)((uintptr_t)y - (uintptr_t)base); im[f].offset_uv = (uint64_t)((uintptr_t)uv - (uintptr_t)base);
    im[f].height = h; im[f].width = w; im[f].stride_y = sy; im[f].stride_uv = suv;
  }
  const uint64_t end_y = im[0].offset_y + ext_y, end_uv = im[0].offset_uv + ext_uv, bytes = end_y > end_uv ? end_y : end_uv;
  yf_det dets[FRAMES * CAP];
  int32_t counts[FRAMES], first[FRAMES + 1];
  yf_chip info[DESIGNED + CAP];
  records(w, h, dets, counts);
  for (int o = 0; o < 3; ++o)
    for (int m = 0; m < 3; ++m)
      for (int flags = 0; flags < 2; ++flags) {
        const size_t chip_bytes = (size_t)OUTS[o][0] * OUTS[o][1] * 3;
        uint8_t* chips = exact(chip_bytes * (DESIGNED + CAP));
        const long rc = yfi_crop_records_yuv_host(base, bytes, format, im, dets, counts, FRAMES, CAP, OUTS[o][0], OUTS[o][1], (o + m + flags) & 1,
                                                  MARGINS[m], flags, chips, DESIGNED + CAP, first, info);
        check_run(rc, first, info, chips, chip_bytes, w, h, 0);
        free(chips);
      }
  free(y); free(uv);
  const size_t chip_bytes = 16 * 16 * 3;
  uint8_t* chips = exact(chip_bytes * (DESIGNED + CAP));
  check_run(yfi_crop_records_yuv_host(base, bytes - 1, format, im, dets, counts, FRAMES, CAP, 16, 16, 1, 0, 0, chips, DESIGNED + CAP, first, info),
            first, info, chips, chip_bytes, w, h, 1);
  for (int f = 0; f < FRAMES; ++f) im[f].width = w - 1;                                    /* an odd side */
  check_run(yfi_crop_records_yuv_host(base, UINT64_MAX, format, im, dets, counts, FRAMES, CAP, 16, 16, 1, 0, 0, chips, DESIGNED + CAP, first, info),
            first, info, chips, chip_bytes, w, h, 1);
  free(chips);
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
  CHECK(yfi_crop_records_host(NULL, 0, 0, NULL, NULL, NULL, 1, 1, 24, 16, 1, 0, 0, NULL, 0, NULL, NULL) == -1);
  CHECK(yfi_crop_records_host(NULL, 0, 0, NULL, NULL, NULL, 1, 1, 16, 16, 1, 1001, 0, NULL, 0, NULL, NULL) == -1);
  CHECK(yfi_crop_records_host(NULL, 0, YF_PIX_NV12, NULL, NULL, NULL, 1, 1, 16, 16, 1, 0, 0, NULL, 0, NULL, NULL) == -1);
  CHECK(yfi_crop_records_yuv_host(NULL, 0, YF_PIX_BGR8, NULL, NULL, NULL, 1, 1, 16, 16, 1, 0, 0, NULL, 0, NULL, NULL) == -1);
  printf("crop: ok\n");
  return 0;
}
