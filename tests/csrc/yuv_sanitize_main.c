/* The host prepare of NV12 / NV21 surfaces (csrc/yf_images_yuv.h through csrc/yf_images_host.c) under ASan + UBSan: a program of its own,
 * compiled together with yf_images_host.c by tests/test_images_yuv_sanitize.py.  The Y plane and the UV plane of a surface are two
 * allocations of exactly their extents ((rows - 1) * stride + width bytes), handed over as one base with two offsets, so an index one byte
 * before or past either plane is a report.  It runs every shape of the GPU tests at both frame sizes, as int8 and as fp16 frames, both
 * chroma orders, packed and padded strides, and the descriptor check on the cases whose sums overflow 64 bits. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/yf_images.h"

int yfi_yuv_image_ok_host(uint64_t offset_y, uint64_t offset_uv, int64_t h, int64_t w, int64_t stride_y, int64_t stride_uv, uint64_t bytes);
int yfi_prepare_yuv_host(const uint8_t* base, uint64_t bytes, const yf_image_yuv* im, int v_first, int out_hw, int f16, void* frame);
void yfi_yuv_rgb_host(const uint8_t* yuv, long n, uint8_t* rgb);

static uint32_t g_seed = 2024u;
static uint32_t rnd(void) { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

#define CHECK(c) do { if (!(c)) { printf("yuv: FAILED %s (line %d)\n", #c, __LINE__); exit(1); } } while (0)

static uint8_t* exact(size_t bytes) {
  uint8_t* p = malloc(bytes);
  CHECK(p);
  for (size_t i = 0; i < bytes; ++i) p[i] = (uint8_t)rnd();
  return p;
}

/* one surface in two exact allocations; the base is the lower of the two, the buffer's size the end of the higher */
static void surface_case(int h, int w, int pad_y, int pad_uv) {
  const int64_t sy = w + pad_y, suv = w + pad_uv;
  const size_t ext_y = (size_t)(h - 1) * (size_t)sy + (size_t)w, ext_uv = (size_t)(h / 2 - 1) * (size_t)suv + (size_t)w;
  uint8_t* y = exact(ext_y);
  uint8_t* uv = exact(ext_uv);
  const uint8_t* base = y < uv ? y : uv;
  yf_image_yuv im = {(uint64_t)((uintptr_t)y - (uintptr_t)base), (uint64_t)((uintptr_t)uv - (uintptr_t)base), h, w, sy, suv};
  const uint64_t end_y = im.offset_y + ext_y, end_uv = im.offset_uv + ext_uv;
  const uint64_t bytes = end_y > end_uv ? end_y : end_uv;
  const int outs[2] = {56, 160};
  for (int o = 0; o < 2; ++o)
    for (int v_first = 0; v_first < 2; ++v_first)
      for (int f16 = 0; f16 < (outs[o] == 56 ? 2 : 1); ++f16) {
        const size_t fb = (size_t)outs[o] * outs[o] * 3 * (f16 ? 2 : 1);
        uint8_t* frame = exact(fb);
        CHECK(yfi_prepare_yuv_host(base, bytes, &im, v_first, outs[o], f16, frame) == 0);
        if (!f16 && h == outs[o] && w == outs[o]) {                       /* the identity size: output pixel (0, 0) is source pixel (0, 0) */
          const uint8_t yuv[3] = {y[0], uv[v_first ? 1 : 0], uv[v_first ? 0 : 1]};
          uint8_t rgb[3];
          yfi_yuv_rgb_host(yuv, 1, rgb);
          CHECK(((int8_t*)frame)[0] == (int8_t)(rgb[0] - 128) && ((int8_t*)frame)[2] == (int8_t)(rgb[2] - 128));
        }
        free(frame);
      }
  /* one byte less of buffer, a stride below the width, odd sides: status 1, the fill, and no read (the planes are still exact) */
  uint8_t* frame = exact(56 * 56 * 3 * 2);
  CHECK(yfi_prepare_yuv_host(base, bytes - 1, &im, 0, 56, 0, frame) == 1 && frame[0] == 0x80 && frame[56 * 56 * 3 - 1] == 0x80);
  yf_image_yuv bad = im;
  bad.stride_uv = w - 1;
  CHECK(yfi_prepare_yuv_host(base, bytes, &bad, 0, 56, 1, frame) == 1 && frame[0] == 0 && frame[56 * 56 * 3 * 2 - 1] == 0);
  bad = im; bad.height = h + 1;
  CHECK(yfi_prepare_yuv_host(base, UINT64_MAX, &bad, 1, 56, 0, frame) == 1);
  bad = im; bad.width = w - 1;
  CHECK(yfi_prepare_yuv_host(base, UINT64_MAX, &bad, 1, 56, 0, frame) == 1);
  free(frame); free(y); free(uv);
}

static void descriptor_cases(void) {
  const uint64_t big = 1ull << 63;
  CHECK(yfi_yuv_image_ok_host(0, 16, 4, 4, 4, 4, 24) == 1);
  CHECK(yfi_yuv_image_ok_host(0, 16, 4, 4, 4, 4, 23) == 0);
  CHECK(yfi_yuv_image_ok_host(8, 0, 4, 4, 4, 4, 24) == 1);                              /* UV before Y */
  CHECK(yfi_yuv_image_ok_host(9, 0, 4, 4, 4, 4, 24) == 0);
  CHECK(yfi_yuv_image_ok_host(0, 16, 4, 4, 3, 4, 1000) == 0 && yfi_yuv_image_ok_host(0, 16, 4, 4, 4, 3, 1000) == 0);
  CHECK(yfi_yuv_image_ok_host(0, 16, 3, 4, 4, 4, 1000) == 0 && yfi_yuv_image_ok_host(0, 16, 4, 5, 8, 8, 1000) == 0);
  CHECK(yfi_yuv_image_ok_host(0, 16, 0, 4, 4, 4, 1000) == 0 && yfi_yuv_image_ok_host(0, 16, 4, 16386, 20000, 20000, UINT64_MAX) == 0);
  CHECK(yfi_yuv_image_ok_host(0, 0, 16384, 16384, 16384, 16384, UINT64_MAX) == 1);
  /* sums that wrap in 64 bits */
  CHECK(yfi_yuv_image_ok_host(UINT64_MAX, 0, 4, 4, 4, 4, UINT64_MAX) == 0);
  CHECK(yfi_yuv_image_ok_host(0, UINT64_MAX - 6, 4, 4, 4, 4, UINT64_MAX) == 0);
  CHECK(yfi_yuv_image_ok_host(0, UINT64_MAX - 8, 4, 4, 4, 4, UINT64_MAX) == 1);
  CHECK(yfi_yuv_image_ok_host(big, big + 16, 4, 4, 4, 4, big + 24) == 1);
  CHECK(yfi_yuv_image_ok_host(0, 0, 4, 4, INT64_MAX, 4, UINT64_MAX) == 0);
  CHECK(yfi_yuv_image_ok_host(0, 0, 4, 4, 4, INT64_MAX, UINT64_MAX) == 1);                /* one step of 2^63 - 1, then 4 bytes: it fits */
  CHECK(yfi_yuv_image_ok_host(0, 0, 6, 4, 4, INT64_MAX, UINT64_MAX) == 0);                /* two steps do not */
  CHECK(yfi_yuv_image_ok_host(0, 0, 16384, 16384, INT64_MAX, INT64_MAX, UINT64_MAX) == 0);
  CHECK(yfi_yuv_image_ok_host(0, 0, 4, 4, INT64_MIN, 4, UINT64_MAX) == 0);
  CHECK(yfi_yuv_image_ok_host(0, 0, INT64_MIN, INT64_MAX, 4, 4, UINT64_MAX) == 0);
}

int main(void) {
  const int shapes[12][2] = {{2, 2}, {2, 4}, {4, 2}, {6, 10}, {54, 58}, {56, 56}, {58, 54}, {112, 112}, {362, 410}, {450, 306},
                             {2, 16384}, {16384, 2}};
  for (int k = 0; k < 12; ++k) {
    surface_case(shapes[k][0], shapes[k][1], 0, 0);
    surface_case(shapes[k][0], shapes[k][1], 3, 6);
  }
  descriptor_cases();
  printf("yuv: ok\n");
  return 0;
}
