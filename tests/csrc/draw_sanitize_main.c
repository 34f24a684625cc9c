/* The host build of the drawing (csrc/yf_images_draw.h through csrc/yf_images_host.c) under ASan + UBSan: a program of its own, compiled
 * together with yf_images_host.c by tests/test_draw_sanitize.py.  Every packed picture, and every Y plane and UV plane of a surface, is an
 * allocation of exactly its extent ((rows - 1) * stride + width * C bytes), handed over as one base with offsets, so a store one byte
 * before or past a picture is a report.  Frame 0 holds designed records -- inside, on every border, beyond every side, wholly outside at
 * distance half and half + 1, x1 > x2, y1 > y2, a point, lines, a box thinner than 2 * half + 1, INT32_MIN / INT32_MAX edges, odd and even
 * origins, boxes that cross, coincide and contain each other --, frame 1 records of random bytes under a count of random bytes, frame 2 a
 * count above cap, frame 3 a negative count; keys and palettes are random bytes; pictures of 1 x 1, 2 x 7, 23 x 37 and 64 x 48 (surfaces:
 * 2 x 2, 22 x 34, 48 x 64), every format, half 0 to 3, with and without keys, packed and padded strides; and invalid descriptors over
 * memory that has been freed, which must be neither read nor written.  Each frame has a picture of its own. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/yf_images.h"

long yfi_draw_records_host(uint8_t* base, uint64_t bytes, int format, const yf_image* images, const yf_det* dets, const int32_t* counts, long n,
                           int cap, int half, uint32_t colour, const void* keys, int key_stride, const uint32_t* palette, int palette_n,
                           int32_t* first, int32_t* status);
long yfi_draw_records_yuv_host(uint8_t* base, uint64_t bytes, int format, const yf_image_yuv* images, const yf_det* dets, const int32_t* counts,
                               long n, int cap, int half, uint32_t colour, const void* keys, int key_stride, const uint32_t* palette,
                               int palette_n, int32_t* first, int32_t* status);

static uint32_t g_seed = 6161u;
static uint32_t rnd(void) { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

#define CHECK(c) do { if (!(c)) { printf("draw: FAILED %s (line %d)\n", #c, __LINE__); exit(1); } } while (0)

static uint8_t* exact(size_t bytes) {
  uint8_t* p = malloc(bytes);
  CHECK(p);
  for (size_t i = 0; i < bytes; ++i) p[i] = (uint8_t)rnd();
  return p;
}

static void random_bytes(void* p, size_t bytes) {
  for (size_t i = 0; i < bytes; ++i) ((uint8_t*)p)[i] = (uint8_t)rnd();
}

enum { CAP = 32, FRAMES = 4, DESIGNED = 30 };

static int32_t clampi(int32_t v, int32_t cap) { return v < 0 ? 0 : (v > cap ? cap : v); }

/* frame 0: the designed records; frame 1: records and a count of random bytes; frame 2: a count above cap over random records about the
 * picture; frame 3: a negative count */
static void records(int w, int h, int k, yf_det* dets, int32_t* counts) {
  const int32_t b[DESIGNED][4] = {
      {w / 4, h / 4, 3 * w / 4, 3 * h / 4}, {0, 0, w - 1, h - 1},
      {-5, h / 3, w + 4, 2 * h / 3}, {w / 3, -6, 2 * w / 3, h + 7}, {-4, -4, w / 2, h / 2},
      {-k - 4, 2, -k, h - 3}, {-k - 5, 1, -k - 1, h - 2}, {w - 1 + k, 1, w + 5 + k, h - 2}, {w + k, 2, w + 6 + k, h - 3},
      {1, -k - 3, w - 2, -k}, {2, -k - 4, w - 3, -k - 1}, {2, h - 1 + k, w - 3, h + 4 + k}, {1, h + k, w - 2, h + 5 + k},
      {2 * w / 3, h / 4, w / 3, h / 2}, {w / 4, 2 * h / 3, w / 2, h / 3},
      {w / 2, h / 2, w / 2, h / 2}, {1, h / 2 + 2, w - 2, h / 2 + 2}, {w / 2 + 1, 1, w / 2 + 1, h - 2},
      {w / 3, h / 3, w / 3 + k, h / 3 + 2 * k},
      {INT32_MIN, INT32_MIN, INT32_MAX, INT32_MAX}, {INT32_MIN, h / 4, w / 2, INT32_MAX}, {INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN},
      {1, 1, 6, 6}, {2, 2, 7, 7}, {3, 4, 8, 9},
      {2, h / 2 - 3, w - 3, h / 2 + 3}, {w / 2 - 3, 2, w / 2 + 3, h - 3},
      {w / 5, h / 5, w / 5 + 9, h / 5 + 9}, {w / 5, h / 5, w / 5 + 9, h / 5 + 9}, {6, 6, 19, 19}};
  random_bytes(dets, sizeof(yf_det) * FRAMES * CAP);
  for (int s = 0; s < DESIGNED; ++s) {
    yf_det* d = &dets[s];
    d->x1 = b[s][0]; d->y1 = b[s][1]; d->x2 = b[s][2]; d->y2 = b[s][3];
  }
  for (int s = 0; s < CAP; ++s) {
    yf_det* d = &dets[2 * CAP + s];
    d->x1 = (int32_t)(rnd() % (uint32_t)(w + 8)) - 4; d->y1 = (int32_t)(rnd() % (uint32_t)(h + 8)) - 4;
    d->x2 = d->x1 + (int32_t)(rnd() % 40u) - 3; d->y2 = d->y1 + (int32_t)(rnd() % 40u) - 3;
  }
  counts[0] = DESIGNED; random_bytes(&counts[1], 4); counts[2] = CAP + 100; counts[3] = -2;
}

static void check_run(long rc, const int32_t* counts, const int32_t* first, const int32_t* status, int want_status) {
  CHECK(rc == FRAMES);
  int32_t at = 0;
  for (int f = 0; f < FRAMES; ++f) {
    CHECK(first[f] == at && status[f] == want_status);
    at += clampi(counts[f], CAP);
  }
  CHECK(first[FRAMES] == at);
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
  uint8_t* keep3 = malloc(ext);
  CHECK(keep3);
  memcpy(keep3, px[3], ext);
  for (int half = 0; half < 4; ++half) {
    records(w, h, half, dets, counts);
    /* one colour: record 1 of frame 0 is the picture's border, so its last pixel carries the colour (nothing behind it draws there with
     * another: all writers write the same bytes) */
    check_run(yfi_draw_records_host(base, bytes, format, im, dets, counts, FRAMES, CAP, half, 0x00C82D5Au, NULL, 0, NULL, 0, first, status), counts,
              first, status, 0);
    const uint8_t* p = px[0] + (size_t)(h - 1) * (size_t)rs + (size_t)(w - 1) * C;
    CHECK(p[1] == 0x2D && p[0] == (format == YF_PIX_BGR8 || format == YF_PIX_BGRA8 ? 0x5A : 0xC8));
    /* keys of random bytes at every stride, palettes of random bytes of 1, 3 and 256 entries: exact allocations */
    for (int stride = 4; stride <= 64; stride += (stride < 16 ? 4 : 24)) {
      const int pn = stride == 4 ? 1 : (stride == 16 ? 256 : 3);
      const size_t key_bytes = (size_t)(FRAMES * CAP - 1) * (size_t)stride + 4;
      uint8_t* keys = exact(key_bytes);
      uint32_t* pal = (uint32_t*)exact((size_t)pn * 4);
      check_run(yfi_draw_records_host(base, bytes, format, im, dets, counts, FRAMES, CAP, half, 0, keys, stride, pal, pn, first, status), counts,
                first, status, 0);
      free(keys); free(pal);
    }
  }
  CHECK(memcmp(keep3, px[3], ext) == 0);                                   /* the frame whose count is -2 */
  free(keep3);
  /* invalid descriptors over freed memory: one byte less of buffer, a stride below the row, a side of 0 -- status 1, no access */
  for (int f = 0; f < FRAMES; ++f) free(px[f]);
  CHECK(ext >= 1);
  for (int f = 0; f < FRAMES; ++f) im[f].offset = bytes - ext;
  check_run(yfi_draw_records_host(base, bytes - 1, format, im, dets, counts, FRAMES, CAP, 3, 0, NULL, 0, NULL, 0, first, status), counts, first,
            status, 1);
  for (int f = 0; f < FRAMES; ++f) im[f].row_stride = (int64_t)w * C - 1;
  check_run(yfi_draw_records_host(base, UINT64_MAX, format, im, dets, counts, FRAMES, CAP, 1, 0, NULL, 0, NULL, 0, first, status), counts, first,
            status, 1);
  for (int f = 0; f < FRAMES; ++f) { im[f].row_stride = rs; im[f].height = 0; }
  check_run(yfi_draw_records_host(base, UINT64_MAX, format, im, dets, counts, FRAMES, CAP, 0, 0, NULL, 0, NULL, 0, first, status), counts, first,
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
  for (int half = 0; half < 4; ++half) {
    records(w, h, half, dets, counts);
    check_run(yfi_draw_records_yuv_host(base, bytes, format, im, dets, counts, FRAMES, CAP, half, 0x00C82D5Au, NULL, 0, NULL, 0, first, status),
              counts, first, status, 0);
    const uint8_t* p = uv[0] + (size_t)(h / 2 - 1) * (size_t)suv + (size_t)(w - 2);
    CHECK(y[0][ext_y - 1] == 0xC8 && p[0] == (format == YF_PIX_NV21 ? 0x5A : 0x2D) && p[1] == (format == YF_PIX_NV21 ? 0x2D : 0x5A));
    for (int stride = 4; stride <= 64; stride += (stride < 16 ? 4 : 24)) {
      const int pn = stride == 4 ? 1 : (stride == 16 ? 256 : 3);
      const size_t key_bytes = (size_t)(FRAMES * CAP - 1) * (size_t)stride + 4;
      uint8_t* keys = exact(key_bytes);
      uint32_t* pal = (uint32_t*)exact((size_t)pn * 4);
      check_run(yfi_draw_records_yuv_host(base, bytes, format, im, dets, counts, FRAMES, CAP, half, 0, keys, stride, pal, pn, first, status), counts,
                first, status, 0);
      free(keys); free(pal);
    }
  }
  for (int f = 0; f < FRAMES; ++f) { free(y[f]); free(uv[f]); }
  for (int f = 0; f < FRAMES; ++f) im[f].width = w - 1;                                    /* an odd side */
  check_run(yfi_draw_records_yuv_host(base, UINT64_MAX, format, im, dets, counts, FRAMES, CAP, 2, 0, NULL, 0, NULL, 0, first, status), counts, first,
            status, 1);
  for (int f = 0; f < FRAMES; ++f) { im[f].width = w; im[f].offset_uv = bytes - ext_uv; }
  check_run(yfi_draw_records_yuv_host(base, bytes - 1, format, im, dets, counts, FRAMES, CAP, 0, 0, NULL, 0, NULL, 0, first, status), counts, first,
            status, 1);
}

int main(void) {
  const int sizes[4][2] = {{1, 1}, {2, 7}, {23, 37}, {64, 48}};                           /* (W, H) */
  const int even[3][2] = {{2, 2}, {22, 34}, {48, 64}};
  for (int k = 0; k < 4; ++k)
    for (int format = 0; format < 4; ++format) {
      packed_case(sizes[k][0], sizes[k][1], format, 0);
      packed_case(sizes[k][0], sizes[k][1], format, 5);
    }
  for (int k = 0; k < 3; ++k)
    for (int format = YF_PIX_NV12; format <= YF_PIX_NV21; ++format) {
      yuv_case(even[k][0], even[k][1], format, 0, 0);
      yuv_case(even[k][0], even[k][1], format, 3, 6);
    }
  /* arguments the entries refuse: nothing is touched (the pointers are NULL) */
  uint32_t one = 0;
  CHECK(yfi_draw_records_host(NULL, 0, 0, NULL, NULL, NULL, 1, 1, 4, 0, NULL, 0, NULL, 0, NULL, NULL) == -1);
  CHECK(yfi_draw_records_host(NULL, 0, 0, NULL, NULL, NULL, 1, 1, 1, 0x01000000u, NULL, 0, NULL, 0, NULL, NULL) == -1);
  CHECK(yfi_draw_records_host(NULL, 0, 0, NULL, NULL, NULL, 1, 1, 1, 0, NULL, 4, NULL, 0, NULL, NULL) == -1);
  CHECK(yfi_draw_records_host(NULL, 0, 0, NULL, NULL, NULL, 1, 1, 1, 0, &one, 6, &one, 1, NULL, NULL) == -1);
  CHECK(yfi_draw_records_host(NULL, 0, 0, NULL, NULL, NULL, 1, 1, 1, 0, &one, 4, &one, 257, NULL, NULL) == -1);
  CHECK(yfi_draw_records_host(NULL, 0, YF_PIX_NV12, NULL, NULL, NULL, 1, 1, 1, 0, NULL, 0, NULL, 0, NULL, NULL) == -1);
  CHECK(yfi_draw_records_yuv_host(NULL, 0, YF_PIX_BGR8, NULL, NULL, NULL, 1, 1, 1, 0, NULL, 0, NULL, 0, NULL, NULL) == -1);
  printf("draw: ok\n");
  return 0;
}
