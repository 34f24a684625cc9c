/* The host build of the blur (csrc/yf_images_blur.h through csrc/yf_images_host.c) under ASan + UBSan: a program of its own, compiled
 * together with yf_images_host.c by tests/test_blur_sanitize.py.  Every packed picture, every Y plane and UV plane of a surface and the
 * workspace are allocations of exactly their extent ((rows - 1) * stride + width * C bytes; yfi_blur_workspace_host bytes), the pictures
 * handed over as one base with offsets, so a load or a store one byte before or past any of them is a report.  It runs designed boxes --
 * well inside, the whole picture, 1 x 1, overhanging each side and a corner, wholly outside, x1 > x2, y1 > y2, INT32_MIN / INT32_MAX
 * edges, the last pixel, odd origins -- and then records and counts of random bytes; pictures of 37 x 53, 64 x 48, 1 x 1 and 410 x 362
 * (surfaces: the even sizes next to them), every format, grids 1, 3, 8 and 16, margins 0, 250 and 1000, square on and off, packed and
 * padded strides (the largest picture: padded strides and every fifth case, which still takes in every grid, margin and flag), the
 * workspace at its exact size for records_cap = 0, one frame's worth and n * cap; and invalid descriptors over memory that has been
 * freed, which must be neither read nor written.  Each frame has a picture of its own. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/yf_images.h"

long yfi_blur_records_host(uint8_t* base, uint64_t bytes, int format, const yf_image* images, const yf_det* dets, const int32_t* counts,
                           long n, int cap, int grid, uint32_t colour, int margin_permille, int flags, void* work, size_t work_bytes,
                           long records_cap, int32_t* first, int32_t* status);
long yfi_blur_records_yuv_host(uint8_t* base, uint64_t bytes, int format, const yf_image_yuv* images, const yf_det* dets,
                               const int32_t* counts, long n, int cap, int grid, uint32_t colour, int margin_permille, int flags, void* work,
                               size_t work_bytes, long records_cap, int32_t* first, int32_t* status);
size_t yfi_blur_workspace_host(long records_cap, int grid);

static uint32_t g_seed = 6363u;
static uint32_t rnd(void) { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

#define CHECK(c) do { if (!(c)) { printf("blur: FAILED %s (line %d)\n", #c, __LINE__); exit(1); } } while (0)

static uint8_t* exact(size_t bytes) {
  uint8_t* p = malloc(bytes);
  CHECK(p);
  for (size_t i = 0; i < bytes; ++i) p[i] = (uint8_t)rnd();
  return p;
}

enum { CAP = 18, FRAMES = 4, DESIGNED = 16 };

static int clampi(int32_t c) { return c < 0 ? 0 : (c > CAP ? CAP : c); }

/* random = 0 -- frame 0: the 16 designed records; frame 1: count 0; frame 2: a count above cap, all cap records present; frame 3: a
 * negative count.  random = 1: every byte of the records and of the counts is random */
static void records(int w, int h, int random, yf_det* dets, int32_t* counts) {
  const int32_t b[DESIGNED][4] = {
      {w / 4, h / 4, 3 * w / 4, 3 * h / 4}, {0, 0, w - 1, h - 1}, {w / 2, h / 2, w / 2, h / 2},
      {-w / 3 - 2, h / 4, w / 2, h / 2}, {w / 2, h / 4, w + 5, h / 2}, {w / 4, -7, w / 2, h / 2}, {w / 4, h / 2, w / 2, h + 9},
      {-5, -6, w / 3, h / 3}, {w + 3, h + 3, w + 10, h + 12}, {w / 2, 0, w / 2 - 1, h - 1}, {0, h / 2, w - 1, h / 2 - 2},
      {INT32_MIN, INT32_MIN, INT32_MAX, INT32_MAX}, {INT32_MIN, h / 4, w / 2, INT32_MAX},
      {w - 1, h - 1, w - 1, h - 1}, {w - 3, h - 5, w - 1, h - 1}, {1, 1, 3, 3}};
  if (random) {
    uint8_t* p = (uint8_t*)dets;
    for (size_t i = 0; i < sizeof(yf_det) * FRAMES * CAP; ++i) p[i] = (uint8_t)rnd();
    p = (uint8_t*)counts;
    for (size_t i = 0; i < sizeof(int32_t) * FRAMES; ++i) p[i] = (uint8_t)rnd();
    counts[1] = (int32_t)(rnd() % 40u) - 10;                        /* ... and one count near the clamp's range */
    for (int s = 0; s < CAP; s += 2) {                              /* half of frame 1's records near the picture, so that something is blurred */
      yf_det* d = &dets[CAP + s];
      d->x1 = (int32_t)(rnd() % (uint32_t)w) - 3; d->y1 = (int32_t)(rnd() % (uint32_t)h) - 3;
      d->x2 = d->x1 + (int32_t)(rnd() % 70u); d->y2 = d->y1 + (int32_t)(rnd() % 70u);
    }
    return;
  }
  memset(dets, 0xA5, sizeof(yf_det) * FRAMES * CAP);
  for (int f = 0; f < FRAMES; f += 2)
    for (int s = 0; s < (f == 0 ? DESIGNED : CAP); ++s) {
      yf_det* d = &dets[f * CAP + s];
      if (f == 0) { d->x1 = b[s][0]; d->y1 = b[s][1]; d->x2 = b[s][2]; d->y2 = b[s][3]; }
      else { d->x1 = (int32_t)(rnd() % (uint32_t)w) - 3; d->y1 = (int32_t)(rnd() % (uint32_t)h) - 3; d->x2 = d->x1 + (int32_t)(rnd() % 50u); d->y2 = d->y1 + (int32_t)(rnd() % 50u); }
    }
  counts[0] = DESIGNED; counts[1] = 0; counts[2] = CAP + 100; counts[3] = -2;
}

static const int GRIDS[4] = {1, 3, 8, 16};
static const int MARGINS[3] = {0, 250, 1000};

/* first[] is the prefix of the clamped counts; status carries `invalid` in bit 0 and bit 1 by the header's rule */
static void check_run(long rc, const int32_t* counts, const int32_t* first, const int32_t* status, int invalid, long records_cap) {
  CHECK(rc == FRAMES);
  int32_t at = 0;
  for (int f = 0; f < FRAMES; ++f) {
    CHECK(first[f] == at);
    at += clampi(counts[f]);
    CHECK(status[f] == (invalid | (at > first[f] && at > records_cap ? 2 : 0)));
  }
  CHECK(first[FRAMES] == at);
}

static const long CAPS[3] = {0, CAP, (long)FRAMES * CAP};

/* every `step`-th of the 24 (grid, margin, square) cases */
static void packed_case(int w, int h, int format, int pad, int step) {
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
  for (int random = 0; random < 2; ++random) {
    records(w, h, random, dets, counts);
    uint8_t* keep3 = malloc(ext);
    CHECK(keep3);
    memcpy(keep3, px[3], ext);
    for (int k = 0; k < 4; ++k)
      for (int m = 0; m < 3; ++m)
        for (int flags = 0; flags < 2; ++flags) {
          if ((k * 6 + m * 2 + flags + random) % step != 0) continue;
          const long records_cap = CAPS[(k + m + flags) % 3];
          const size_t room = yfi_blur_workspace_host(records_cap, GRIDS[k]);
          CHECK(room == (((size_t)records_cap * (size_t)(GRIDS[k] * GRIDS[k]) * 4u + 15u) & ~(size_t)15u));
          void* work = NULL;
          if (room) CHECK(posix_memalign(&work, 16, room) == 0);
          check_run(yfi_blur_records_host(base, bytes, format, im, dets, counts, FRAMES, CAP, GRIDS[k], 0x00C82D5Au, MARGINS[m], flags, work, room,
                                          records_cap, first, status), counts, first, status, 0, records_cap);
          if (!random && records_cap == 0) {                        /* record 1 is the whole picture and nothing has a slot: the colour */
            const uint8_t* p = px[0] + (size_t)(h - 1) * (size_t)rs + (size_t)(w - 1) * C;
            if (w > 1) CHECK(p[1] == 0x2D && p[0] == (format == YF_PIX_BGR8 || format == YF_PIX_BGRA8 ? 0x5A : 0xC8));
          }
          free(work);
        }
    if (!random) CHECK(memcmp(keep3, px[3], ext) == 0);             /* the frame whose count is -2 */
    free(keep3);
  }
  /* invalid descriptors over freed memory: one byte less of buffer, a stride below the row, a side of 0 -- bit 0, no access */
  records(w, h, 0, dets, counts);
  for (int f = 0; f < FRAMES; ++f) free(px[f]);
  const size_t room = yfi_blur_workspace_host((long)FRAMES * CAP, 8);
  void* work = NULL;
  CHECK(posix_memalign(&work, 16, room) == 0);
  for (int f = 0; f < FRAMES; ++f) im[f].offset = bytes - ext;
  check_run(yfi_blur_records_host(base, bytes - 1, format, im, dets, counts, FRAMES, CAP, 8, 0, 250, 1, work, room, (long)FRAMES * CAP, first,
                                  status), counts, first, status, 1, (long)FRAMES * CAP);
  for (int f = 0; f < FRAMES; ++f) im[f].row_stride = (int64_t)w * C - 1;
  check_run(yfi_blur_records_host(base, UINT64_MAX, format, im, dets, counts, FRAMES, CAP, 16, 0, 0, 0, NULL, 0, 0, first, status), counts, first,
            status, 1, 0);
  for (int f = 0; f < FRAMES; ++f) { im[f].row_stride = rs; im[f].height = 0; }
  check_run(yfi_blur_records_host(base, UINT64_MAX, format, im, dets, counts, FRAMES, CAP, 1, 0, 0, 0, work, room, CAP, first, status), counts,
            first, status, 1, CAP);
  free(work);
}

static void yuv_case(int w, int h, int format, int pad_y, int pad_uv, int step) {
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
  for (int random = 0; random < 2; ++random) {
    records(w, h, random, dets, counts);
    for (int k = 0; k < 4; ++k)
      for (int m = 0; m < 3; ++m)
        for (int flags = 0; flags < 2; ++flags) {
          if ((k * 6 + m * 2 + flags + random) % step != 0) continue;
          const long records_cap = CAPS[(k + m + flags) % 3];
          const size_t room = yfi_blur_workspace_host(records_cap, GRIDS[k]);
          void* work = NULL;
          if (room) CHECK(posix_memalign(&work, 16, room) == 0);
          check_run(yfi_blur_records_yuv_host(base, bytes, format, im, dets, counts, FRAMES, CAP, GRIDS[k], 0x00C82D5Au, MARGINS[m], flags, work,
                                              room, records_cap, first, status), counts, first, status, 0, records_cap);
          if (!random && records_cap == 0) {
            const uint8_t* p = uv[0] + (size_t)(h / 2 - 1) * (size_t)suv + (size_t)(w - 2);
            CHECK(y[0][ext_y - 1] == 0xC8 && p[0] == (format == YF_PIX_NV21 ? 0x5A : 0x2D) && p[1] == (format == YF_PIX_NV21 ? 0x2D : 0x5A));
          }
          free(work);
        }
  }
  records(w, h, 0, dets, counts);
  for (int f = 0; f < FRAMES; ++f) { free(y[f]); free(uv[f]); }
  const size_t room = yfi_blur_workspace_host((long)FRAMES * CAP, 3);
  void* work = NULL;
  CHECK(posix_memalign(&work, 16, room) == 0);
  for (int f = 0; f < FRAMES; ++f) im[f].width = w - 1;                                    /* an odd side */
  check_run(yfi_blur_records_yuv_host(base, UINT64_MAX, format, im, dets, counts, FRAMES, CAP, 3, 0, 0, 0, work, room, (long)FRAMES * CAP, first,
                                      status), counts, first, status, 1, (long)FRAMES * CAP);
  for (int f = 0; f < FRAMES; ++f) { im[f].width = w; im[f].offset_uv = bytes - ext_uv; }
  check_run(yfi_blur_records_yuv_host(base, bytes - 1, format, im, dets, counts, FRAMES, CAP, 3, 0, 0, 0, work, room, 2, first, status), counts,
            first, status, 1, 2);
  free(work);
}

int main(void) {
  const int sizes[4][2] = {{37, 53}, {64, 48}, {1, 1}, {410, 362}};                       /* (W, H) */
  const int even[4][2] = {{38, 54}, {64, 48}, {2, 2}, {410, 362}};
  for (int k = 0; k < 4; ++k)
    for (int format = 0; format < 4; ++format) {
      if (k < 3) packed_case(sizes[k][0], sizes[k][1], format, 0, 1);     /* the large picture: padded rows only, every fifth case */
      packed_case(sizes[k][0], sizes[k][1], format, 5, k < 3 ? 1 : 5);
    }
  for (int k = 0; k < 4; ++k)
    for (int format = YF_PIX_NV12; format <= YF_PIX_NV21; ++format) {
      if (k < 3) yuv_case(even[k][0], even[k][1], format, 0, 0, 1);
      yuv_case(even[k][0], even[k][1], format, 3, 6, k < 3 ? 1 : 5);
    }
  /* arguments the entries refuse: nothing is touched (the pointers are NULL) */
  CHECK(yfi_blur_records_host(NULL, 0, 0, NULL, NULL, NULL, 1, 1, 0, 0, 0, 0, NULL, 0, 0, NULL, NULL) == -1);
  CHECK(yfi_blur_records_host(NULL, 0, 0, NULL, NULL, NULL, 1, 1, 17, 0, 0, 0, NULL, 0, 0, NULL, NULL) == -1);
  CHECK(yfi_blur_records_host(NULL, 0, 0, NULL, NULL, NULL, 1, 1, 8, 0x01000000u, 0, 0, NULL, 0, 0, NULL, NULL) == -1);
  CHECK(yfi_blur_records_host(NULL, 0, 0, NULL, NULL, NULL, 1, 1, 8, 0, 1001, 0, NULL, 0, 0, NULL, NULL) == -1);
  CHECK(yfi_blur_records_host(NULL, 0, 0, NULL, NULL, NULL, 1, 1, 8, 0, 0, 0, NULL, 0, 2, NULL, NULL) == -1);
  CHECK(yfi_blur_records_host(NULL, 0, 0, NULL, NULL, NULL, 1, 1, 8, 0, 0, 0, NULL, 0, 1, NULL, NULL) == -1);
  CHECK(yfi_blur_records_host(NULL, 0, YF_PIX_NV12, NULL, NULL, NULL, 1, 1, 8, 0, 0, 0, NULL, 0, 0, NULL, NULL) == -1);
  CHECK(yfi_blur_records_yuv_host(NULL, 0, YF_PIX_BGR8, NULL, NULL, NULL, 1, 1, 8, 0, 0, 0, NULL, 0, 0, NULL, NULL) == -1);
  printf("blur: ok\n");
  return 0;
}
