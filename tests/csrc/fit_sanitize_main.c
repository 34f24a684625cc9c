/* The host build of the letterboxed frames and their decodes (csrc/yf_images_fit.h through csrc/yf_images_host.c) under ASan + UBSan: a
 * program of its own, compiled together with yf_images_host.c by tests/test_fit_sanitize.py.  Every packed picture, every Y plane and UV
 * plane of a surface, every frame, every head and every record array is an allocation of exactly its extent ((rows - 1) * stride +
 * width * C bytes; S * S * 3 elements; cap records), so a load or a store one byte before or past any of them is a report.  It runs
 * the shapes of the tests (1 x 1, 57 x 56, 56 x 57, 2 x 1, 1 x 2, 3 x 200, 200 x 3, 410 x 362, 1 x 16384 and 16384 x 1; surfaces: 2 x 2,
 * 2 x 400, 400 x 2, 58 x 56, 362 x 410) in every format, at both frame sides and as fp16 frames, pads 0, 114 and 255, packed and padded
 * strides (odd chroma strides among them); then descriptors of random bytes against a small buffer -- whatever they say, a valid one
 * is read inside the buffer and an invalid one gives status 1 and a frame of -128 (fp16: 0) --; then invalid descriptors over memory
 * that has been freed, which must not be read; and the decodes on heads and logits of random bytes with sides of every kind, caps of 1,
 * the count and every candidate. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/yf_images.h"

void yfi_fit_host(int64_t h, int64_t w, int64_t S, int32_t* out);
int yfi_prepare_fit_host(const uint8_t* base, uint64_t bytes, int format, const yf_image* im, int out_hw, int pad, int f16, void* frame);
int yfi_prepare_fit_yuv_host(const uint8_t* base, uint64_t bytes, const yf_image_yuv* im, int v_first, int out_hw, int pad, int f16, void* frame);
int yfi_decode_fit_host(const int8_t* head, int32_t frame, int32_t height, int32_t width, int32_t status, int out_hw, yf_det* dets, int cap);
int yfi_decode_f32_fit_host(const float* logits, int32_t frame, int32_t height, int32_t width, int32_t status, yf_det* dets, int cap);

static uint32_t g_seed = 5616u;
static uint32_t rnd(void) { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

#define CHECK(c) do { if (!(c)) { printf("fit: FAILED %s (line %d)\n", #c, __LINE__); exit(1); } } while (0)

static uint8_t* exact(size_t bytes) {
  uint8_t* p = malloc(bytes ? bytes : 1);
  CHECK(p);
  for (size_t i = 0; i < bytes; ++i) p[i] = (uint8_t)rnd();
  return p;
}

static const int SIDES[3] = {56, 56, 160};       /* the three kinds of frame: int8 at 56, fp16 at 56, int8 at 160 */
static const int F16[3] = {0, 1, 0};
static const int PADS[3] = {0, 114, 255};
static long g_frames, g_records;

/* a frame of exactly its extent, written by `status = prepare(...)`; a valid picture's frame shows the pad exactly outside its fit */
static void check_frame(const void* frame, int S, int f16, int pad, int status, int h, int w) {
  const size_t count = (size_t)S * S * 3;
  if (status == 1) {
    for (size_t i = 0; i < count; ++i) CHECK(f16 ? ((const uint16_t*)frame)[i] == 0 : ((const int8_t*)frame)[i] == -128);
    return;
  }
  CHECK(status == 0);
  int32_t fit[4];
  yfi_fit_host(h, w, S, fit);
  CHECK(fit[0] >= 0 && fit[1] >= 0 && fit[2] >= 1 && fit[3] >= 1 && fit[0] + fit[2] <= S && fit[1] + fit[3] <= S);
  if (f16) return;                                /* the halves: the Python tests compare them */
  for (int y = 0; y < S; ++y)
    for (int x = 0; x < S; ++x) {
      if (x >= fit[0] && x < fit[0] + fit[2] && y >= fit[1] && y < fit[1] + fit[3]) continue;
      for (int c = 0; c < 3; ++c) CHECK(((const int8_t*)frame)[((size_t)y * S + x) * 3 + c] == (int8_t)(pad - 128));
    }
  ++g_frames;
}

static void packed(int h, int w, int format, int extra) {
  const int C = format < 2 ? 3 : 4;
  const int64_t rs = (int64_t)w * C + extra;
  const size_t bytes = (size_t)(h - 1) * (size_t)rs + (size_t)w * C;
  uint8_t* px = exact(bytes);
  const yf_image im = {0, h, w, rs};
  for (int k = 0; k < 3; ++k)
    for (int p = 0; p < 3; ++p) {
      const size_t fb = (size_t)SIDES[k] * SIDES[k] * 3 * (F16[k] ? 2 : 1);
      void* frame = exact(fb);
      check_frame(frame, SIDES[k], F16[k], PADS[p], yfi_prepare_fit_host(px, bytes, format, &im, SIDES[k], PADS[p], F16[k], frame), h, w);
      free(frame);
    }
  free(px);
}

/* the two planes are allocations of their own, handed over as offsets from the lower one */
static void surface(int h, int w, int v_first, int extra_y, int extra_uv) {
  const int64_t sy = w + extra_y, suv = w + extra_uv;
  const size_t by = (size_t)(h - 1) * (size_t)sy + (size_t)w, buv = (size_t)(h / 2 - 1) * (size_t)suv + (size_t)w;
  uint8_t* y = exact(by);
  uint8_t* uv = exact(buv);
  const uint8_t* base = y < uv ? y : uv;
  const uint8_t* top = y < uv ? uv + buv : y + by;
  const yf_image_yuv im = {(uint64_t)(y - base), (uint64_t)(uv - base), h, w, sy, suv};
  for (int k = 0; k < 3; ++k)
    for (int p = 0; p < 3; ++p) {
      const size_t fb = (size_t)SIDES[k] * SIDES[k] * 3 * (F16[k] ? 2 : 1);
      void* frame = exact(fb);
      check_frame(frame, SIDES[k], F16[k], PADS[p],
                  yfi_prepare_fit_yuv_host(base, (uint64_t)(top - base), &im, v_first, SIDES[k], PADS[p], F16[k], frame), h, w);
      free(frame);
    }
  free(y); free(uv);
}

/* descriptors of random bytes against a buffer of exactly `bytes` bytes: about one in four is made plausible, so that valid ones occur */
static void random_descriptors(void) {
  const size_t bytes = 4096;
  uint8_t* px = exact(bytes);
  int valid = 0, invalid = 0;
  for (int t = 0; t < 6000; ++t) {
    yf_image im;
    yf_image_yuv iy;
    uint8_t* p = (uint8_t*)&im;
    for (size_t i = 0; i < sizeof im; ++i) p[i] = (uint8_t)rnd();
    p = (uint8_t*)&iy;
    for (size_t i = 0; i < sizeof iy; ++i) p[i] = (uint8_t)rnd();
    if (t % 4 == 0) {
      im.height = 1 + (int32_t)(rnd() % 40u); im.width = 1 + (int32_t)(rnd() % 40u); im.offset = rnd() % 2048u;
      im.row_stride = (int64_t)im.width * 4 + (int64_t)(rnd() % 9u) - 2;
      iy.height = 2 * (1 + (int32_t)(rnd() % 20u)) + (t % 16 == 0); iy.width = 2 * (1 + (int32_t)(rnd() % 20u));
      iy.offset_y = rnd() % 2048u; iy.offset_uv = rnd() % 3072u; iy.stride_y = iy.width + (int64_t)(rnd() % 5u) - 1; iy.stride_uv = iy.width + (int64_t)(rnd() % 5u) - 1;
    }
    const int k = t % 3, format = (int)(rnd() % 4u), pad = PADS[rnd() % 3u];
    const size_t fb = (size_t)SIDES[k] * SIDES[k] * 3 * (F16[k] ? 2 : 1);
    void* frame = exact(fb);
    int st = yfi_prepare_fit_host(px, bytes, format, &im, SIDES[k], pad, F16[k], frame);
    check_frame(frame, SIDES[k], F16[k], pad, st, im.height, im.width);
    st ? ++invalid : ++valid;
    st = yfi_prepare_fit_yuv_host(px, bytes, &iy, (int)(rnd() & 1u), SIDES[k], pad, F16[k], frame);
    check_frame(frame, SIDES[k], F16[k], pad, st, iy.height, iy.width);
    st ? ++invalid : ++valid;
    free(frame);
  }
  CHECK(valid > 500 && invalid > 500);
  free(px);
}

/* an invalid descriptor's picture is never read: its memory has been freed, and so has a base that no offset makes valid */
static void freed_pictures(void) {
  uint8_t* px = exact(300);
  free(px);
  const yf_image bad[4] = {{0, 10, 10, 29}, {0, 11, 10, 30}, {271, 1, 10, 30}, {0, 0, 0, 0}};         /* stride, rows, offset, sides: 300 bytes */
  const yf_image_yuv ybad[3] = {{0, 260, 10, 10, 10, 10}, {0, 100, 11, 10, 10, 10}, {0, 251, 10, 10, 10, 10}};
  for (int k = 0; k < 3; ++k) {
    const size_t fb = (size_t)SIDES[k] * SIDES[k] * 3 * (F16[k] ? 2 : 1);
    void* frame = exact(fb);
    for (int i = 0; i < 4; ++i) check_frame(frame, SIDES[k], F16[k], 114, yfi_prepare_fit_host(px, 300, 0, &bad[i], SIDES[k], 114, F16[k], frame) == 1 ? 1 : -9, 0, 0);
    for (int i = 0; i < 3; ++i) check_frame(frame, SIDES[k], F16[k], 114, yfi_prepare_fit_yuv_host(px, 300, &ybad[i], i & 1, SIDES[k], 114, F16[k], frame) == 1 ? 1 : -9, 0, 0);
    free(frame);
  }
}

static const int32_t DSIDES[12][2] = {{1080, 1920}, {1920, 1080}, {300, 300}, {362, 410}, {57, 56}, {1, 16384}, {16384, 1}, {16384, 16384},
                                      {3, 200}, {1, 1}, {0, 5}, {5, 16385}};

static void decodes(void) {
  for (int t = 0; t < 60; ++t) {
    const int S = t % 2 ? 160 : 56, G = S / 8, all = 3 * G * G;
    int8_t* head = (int8_t*)exact((size_t)G * G * 18);
    const int32_t h = DSIDES[t % 12][0], w = DSIDES[t % 12][1];
    yf_det* one = (yf_det*)exact(sizeof(yf_det));
    const int count = yfi_decode_fit_host(head, t, h, w, 0, S, one, 1);
    CHECK(count >= 0 && count <= all && (t % 12 < 10 || count == 0));
    if (count > 0) {
      yf_det* just = (yf_det*)exact(sizeof(yf_det) * (size_t)count);
      yf_det* every = (yf_det*)exact(sizeof(yf_det) * (size_t)all);
      CHECK(yfi_decode_fit_host(head, t, h, w, 0, S, just, count) == count && yfi_decode_fit_host(head, t, h, w, 0, S, every, all) == count);
      CHECK(memcmp(just, every, sizeof(yf_det) * (size_t)count) == 0 && memcmp(one, every, sizeof(yf_det)) == 0);
      CHECK(yfi_decode_fit_host(head, t, h, w, 1, S, just, count) == 0);
      g_records += count;
      free(just); free(every);
    }
    free(one); free(head);
    float* logits = (float*)exact(sizeof(float) * 7 * 7 * 18);            /* random bits: NaN, infinities, subnormals, huge values */
    if (t % 3 == 0) for (int i = 4; i < 882; i += 6) logits[i] = 6.0f;  /* every candidate fires */
    yf_det* f1 = (yf_det*)exact(sizeof(yf_det));
    const int c32 = yfi_decode_f32_fit_host(logits, t, h, w, 0, f1, 1);
    CHECK(c32 >= 0 && c32 <= 147 && (t % 12 < 10 || c32 == 0) && (t % 3 != 0 || t % 12 >= 10 || c32 == 147));
    if (c32 > 0) {
      yf_det* just = (yf_det*)exact(sizeof(yf_det) * (size_t)c32);
      CHECK(yfi_decode_f32_fit_host(logits, t, h, w, 0, just, c32) == c32 && memcmp(just, f1, sizeof(yf_det)) == 0);
      g_records += c32;
      free(just);
    }
    free(f1); free(logits);
  }
}

int main(void) {
  const int shapes[10][2] = {{1, 1}, {57, 56}, {56, 57}, {2, 1}, {1, 2}, {3, 200}, {200, 3}, {362, 410}, {1, 16384}, {16384, 1}};
  for (int s = 0; s < 10; ++s)
    for (int format = 0; format < 4; ++format) {
      packed(shapes[s][0], shapes[s][1], format, 0);
      if (s < 8) packed(shapes[s][0], shapes[s][1], format, 1 + (int)(rnd() % 13u));
    }
  const int surfaces[5][2] = {{2, 2}, {2, 400}, {400, 2}, {58, 56}, {362, 410}};
  for (int s = 0; s < 5; ++s)
    for (int v_first = 0; v_first < 2; ++v_first) {
      surface(surfaces[s][0], surfaces[s][1], v_first, 0, 0);
      surface(surfaces[s][0], surfaces[s][1], v_first, 3, 5);            /* odd pitches on both planes */
    }
  random_descriptors();
  freed_pictures();
  decodes();
  printf("fit: ok (%ld int8 frames checked for their padding, %ld records)\n", g_frames, g_records);
  return 0;
}
