/* The host build of the area-averaged frames (csrc/yf_images_area.h through csrc/yf_images_host.c) under ASan + UBSan: a program of its
 * own, compiled together with yf_images_host.c by tests/test_area_sanitize.py.  Every packed picture, every Y plane and UV plane of a
 * surface and every frame is an allocation of exactly its extent ((rows - 1) * stride + width * C bytes; S * S * 3 elements), so a load
 * or a store one byte before or past any of them is a report.  It runs the shapes of the tests (1 x 1, 1 x 7, 7 x 1, 55 x 57, 56 x 56,
 * 57 x 57, 112 x 112, 113 x 111, 167 x 300, 2 x 16384, 16384 x 2, 16384 x 3, 3 x 16384; surfaces with even sides) in every format, at
 * both frame sides and as fp16 frames, under both fits, packed and padded strides; checks on the way what needs no restatement (a
 * constant picture gives a constant frame, the pad lies exactly outside the fit); then descriptors of random bytes against a small
 * buffer -- whatever they say, a valid one is read inside the buffer and an invalid one gives status 1 and a frame of -128 (fp16: 0)
 * --; then invalid descriptors over memory that has been freed, which must not be read. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/yf_images.h"

void yfi_fit_host(int64_t h, int64_t w, int64_t S, int32_t* out);
int yfi_prepare_area_host(const uint8_t* base, uint64_t bytes, int format, const yf_image* im, int out_hw, int fit, int pad, int f16, void* frame);
int yfi_prepare_area_yuv_host(const uint8_t* base, uint64_t bytes, const yf_image_yuv* im, int v_first, int out_hw, int fit, int pad, int f16,
                              void* frame);
int yfi_area_axis_host(int32_t n_in, int32_t n_out, int32_t* firsts, int32_t* lasts, int64_t* sums);

static uint32_t g_seed = 160056u;
static uint32_t rnd(void) { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

#define CHECK(c) do { if (!(c)) { printf("area: FAILED %s (line %d)\n", #c, __LINE__); exit(1); } } while (0)

/* an allocation of exactly `bytes` bytes: random ones, or all `value` (0..255) */
static uint8_t* exact(size_t bytes, int value) {
  uint8_t* p = malloc(bytes ? bytes : 1);
  CHECK(p);
  for (size_t i = 0; i < bytes; ++i) p[i] = value < 0 ? (uint8_t)rnd() : (uint8_t)value;
  return p;
}

static const int SIDES[3] = {56, 56, 160};       /* the three kinds of frame: int8 at 56, fp16 at 56, int8 at 160 */
static const int F16[3] = {0, 1, 0};
static long g_frames;

static size_t frame_bytes(int k) { return (size_t)SIDES[k] * SIDES[k] * 3 * (F16[k] ? 2 : 1); }

/* value >= 0: the picture was all `value` (YUV: not checked, the conversion is the Python tests' matter) */
static void check_frame(const void* frame, int k, int fit, int pad, int status, int h, int w, int value) {
  const int S = SIDES[k], f16 = F16[k];
  const size_t count = (size_t)S * S * 3;
  if (status == 1) {
    for (size_t i = 0; i < count; ++i) CHECK(f16 ? ((const uint16_t*)frame)[i] == 0 : ((const int8_t*)frame)[i] == -128);
    return;
  }
  CHECK(status == 0);
  ++g_frames;
  if (f16) return;                                /* the halves: the Python tests compare them */
  int32_t r[4] = {0, 0, S, S};
  if (fit == YF_FIT_LETTERBOX) yfi_fit_host(h, w, S, r);
  for (int y = 0; y < S; ++y)
    for (int x = 0; x < S; ++x) {
      const int in = x >= r[0] && x < r[0] + r[2] && y >= r[1] && y < r[1] + r[3];
      if (in && value < 0) continue;
      for (int c = 0; c < 3; ++c) CHECK(((const int8_t*)frame)[((size_t)y * S + x) * 3 + c] == (int8_t)((in ? value : pad) - 128));
    }
}

static void packed(int h, int w, int format, int extra, int value) {
  const int C = format < 2 ? 3 : 4;
  const int64_t rs = (int64_t)w * C + extra;
  const size_t bytes = (size_t)(h - 1) * (size_t)rs + (size_t)w * C;
  uint8_t* px = exact(bytes, value);
  const yf_image im = {0, h, w, rs};
  for (int k = 0; k < 3; ++k)
    for (int fit = 0; fit < 2; ++fit) {
      const int pad = fit ? 114 : 231;
      void* frame = exact(frame_bytes(k), -1);
      check_frame(frame, k, fit, pad, yfi_prepare_area_host(px, bytes, format, &im, SIDES[k], fit, pad, F16[k], frame), h, w, value);
      free(frame);
    }
  free(px);
}

/* the two planes are allocations of their own, handed over as offsets from the lower one */
static void surface(int h, int w, int v_first, int extra_y, int extra_uv) {
  const int64_t sy = w + extra_y, suv = w + extra_uv;
  const size_t by = (size_t)(h - 1) * (size_t)sy + (size_t)w, buv = (size_t)(h / 2 - 1) * (size_t)suv + (size_t)w;
  uint8_t* y = exact(by, -1);
  uint8_t* uv = exact(buv, -1);
  const uint8_t* base = y < uv ? y : uv;
  const uint8_t* top = y < uv ? uv + buv : y + by;
  const yf_image_yuv im = {(uint64_t)(y - base), (uint64_t)(uv - base), h, w, sy, suv};
  for (int k = 0; k < 3; ++k)
    for (int fit = 0; fit < 2; ++fit) {
      void* frame = exact(frame_bytes(k), -1);
      check_frame(frame, k, fit, 7, yfi_prepare_area_yuv_host(base, (uint64_t)(top - base), &im, v_first, SIDES[k], fit, 7, F16[k], frame), h, w, -1);
      free(frame);
    }
  free(y); free(uv);
}

/* descriptors of random bytes against a buffer of exactly `bytes` bytes: about one in four is made plausible, so that valid ones occur */
static void random_descriptors(void) {
  const size_t bytes = 4096;
  uint8_t* px = exact(bytes, -1);
  int valid = 0, invalid = 0;
  for (int t = 0; t < 4000; ++t) {
    yf_image im;
    yf_image_yuv iy;
    uint8_t* p = (uint8_t*)&im;
    for (size_t i = 0; i < sizeof im; ++i) p[i] = (uint8_t)rnd();
    p = (uint8_t*)&iy;
    for (size_t i = 0; i < sizeof iy; ++i) p[i] = (uint8_t)rnd();
    if (t % 4 == 0) {
      im.height = 1 + (int32_t)(rnd() % 40u); im.width = 1 + (int32_t)(rnd() % 40u); im.offset = rnd() % 2048u;
      im.row_stride = (int64_t)im.width * 4 + (int64_t)(rnd() % 9u) - 2;
      iy.height = 2 * (1 + (int32_t)(rnd() % 20u)); iy.width = 2 * (1 + (int32_t)(rnd() % 20u));
      iy.offset_y = rnd() % 2048u; iy.offset_uv = rnd() % 3072u;
      iy.stride_y = iy.width + (int64_t)(rnd() % 5u) - 1; iy.stride_uv = iy.width + (int64_t)(rnd() % 5u) - 1;
    }
    const int k = t % 3, fit = (t >> 2) & 1;
    void* frame = exact(frame_bytes(k), -1);
    int st = yfi_prepare_area_host(px, bytes, t % 4, &im, SIDES[k], fit, 114, F16[k], frame);
    CHECK(st == 0 || st == 1);
    check_frame(frame, k, fit, 114, st, im.height, im.width, -1);
    if (st) ++invalid; else ++valid;
    st = yfi_prepare_area_yuv_host(px, bytes, &iy, t & 1, SIDES[k], fit, 114, F16[k], frame);
    CHECK(st == 0 || st == 1);
    check_frame(frame, k, fit, 114, st, iy.height, iy.width, -1);
    if (st) ++invalid; else ++valid;
    free(frame);
  }
  CHECK(valid > 100 && invalid > 100);
  free(px);
}

/* invalid descriptors whose pixels are memory that has been freed: never read */
static void invalid_over_freed(void) {
  const size_t bytes = 300;
  uint8_t* px = exact(bytes, -1);
  free(px);
  const yf_image bad[5] = {{0, 10, 10, 29}, {0, 11, 10, 30}, {1, 10, 10, 30}, {0, 0, 10, 30}, {0, 10, 16385, 30}};
  const yf_image_yuv bad_yuv[4] = {{0, 260, 10, 10, 10, 10}, {0, 100, 11, 10, 10, 10}, {0, 100, 10, 10, 9, 10}, {0, 251, 10, 10, 10, 10}};
  for (int k = 0; k < 3; ++k) {
    void* frame = exact(frame_bytes(k), -1);
    for (int i = 0; i < 5; ++i) check_frame(frame, k, i & 1, 114, yfi_prepare_area_host(px, bytes, 0, &bad[i], SIDES[k], i & 1, 114, F16[k], frame), 1, 1, -1);
    for (int i = 0; i < 4; ++i)
      check_frame(frame, k, i & 1, 114, yfi_prepare_area_yuv_host(px, bytes, &bad_yuv[i], i & 1, SIDES[k], i & 1, 114, F16[k], frame), 2, 2, -1);
    free(frame);
  }
}

int main(void) {
  static const int SHAPES[13][2] = {{1, 1}, {1, 7}, {7, 1}, {55, 57}, {56, 56}, {57, 57}, {112, 112}, {113, 111}, {167, 300}, {2, 16384}, {16384, 2},
                                    {16384, 3}, {3, 16384}};
  for (int s = 0; s < 13; ++s)
    for (int format = 0; format < 4; ++format) packed(SHAPES[s][0], SHAPES[s][1], format, (s + format) % 3 == 0 ? 0 : 1 + (s + format) % 7, -1);
  /* constant pictures: constant frames; 16384 x 3 and 3 x 16384 of 255 are the 32-bit row-sum bound */
  static const int CONST[5][2] = {{16384, 3}, {3, 16384}, {1, 1}, {57, 55}, {300, 167}};
  static const int VALUES[4] = {255, 0, 1, 128};
  for (int s = 0; s < 5; ++s)
    for (int v = 0; v < (s < 2 ? 1 : 4); ++v) packed(CONST[s][0], CONST[s][1], s % 4, s, VALUES[v]);
  static const int SURF[8][2] = {{2, 2}, {2, 8}, {8, 2}, {54, 58}, {58, 58}, {114, 110}, {2, 16384}, {16384, 2}};
  for (int s = 0; s < 8; ++s)
    for (int v_first = 0; v_first < 2; ++v_first) surface(SURF[s][0], SURF[s][1], v_first, s % 2 ? 3 : 0, s % 3 ? 1 : 0);
  random_descriptors();
  invalid_over_freed();
  /* the axes the shapes above did not take, through the span the kernels use */
  static int32_t firsts[160], lasts[160];
  static int64_t sums[160];
  for (int n_in = 1; n_in <= 16384; n_in += 1 + n_in / 64)
    for (int k = 0; k < 2; ++k) {
      const int n_out = k ? 160 : 56;
      CHECK(yfi_area_axis_host(n_in, n_out, firsts, lasts, sums) == 0);
      for (int d = 0; d < n_out; ++d) CHECK(sums[d] == n_in && firsts[d] >= 0 && lasts[d] < n_in);
    }
  printf("area: ok (%ld frames)\n", g_frames);
  return 0;
}
