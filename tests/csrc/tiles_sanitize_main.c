/* The planner and the host merge of the tiled detection (csrc/yf_images_tiles.h through csrc/yf_images_host.c) under ASan + UBSan: a
 * program of its own, compiled together with yf_images_host.c by tests/test_tiles_sanitize.py.  Every array is allocated at exactly the
 * size the call may touch, so one element too far is a report.  It runs the grid's edge lengths, the count cases of the merge (0,
 * negative, cap, above cap, INT32_MIN), the edge values (INT32_MIN, INT32_MAX, INT32_MAX - 5 at x0 = 16383), the out_cap cuts, and
 * `first` arrays that are not well formed: descending, negative, beyond t, overlapping ranges -- for those only "no access leaves the
 * buffers" is promised. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/yf_images.h"

long yfi_plan_tiles_host(const yf_image* images, long n, int format, int tile_h, int tile_w, int stride_y, int stride_x, int whole,
                         yf_tile* tiles, yf_image* tile_images, int32_t* first, long tiles_cap);
long yfi_gather_tiles_host(const yf_det* dets, const int32_t* counts, long t, int cap, const yf_tile* tiles, const int32_t* first,
                           long n, yf_det* out, int32_t* out_counts, int out_cap);

static uint32_t g_seed = 12345u;
static uint32_t rnd(void) { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

#define CHECK(c) do { if (!(c)) { printf("tiles: FAILED %s (line %d)\n", #c, __LINE__); exit(1); } } while (0)

static void* exact(size_t bytes) { void* p = malloc(bytes ? bytes : 1); CHECK(p); memset(p, 0xA5, bytes); return p; }

static void plan_cases(void) {
  const int T = 8;
  const int strides[3] = {1, 4, 8};
  for (int si = 0; si < 3; ++si) {
    const int S = strides[si];
    const int lens[8] = {1, T - 1, T, T + 1, T + S - 1, T + S, T + S + 1, 16384};
    for (int whole = 0; whole < 2; ++whole)
      for (int a = 0; a < 8; ++a)
        for (int b = 0; b < 8; ++b) {
          if (a == 7 && b == 7) continue;                                   /* 16384 x 16384 is counted below */
          yf_image parent[2] = {{64, lens[a], lens[b], (int64_t)lens[b] * 3 + 5}, {1 << 20, lens[b], lens[a], (int64_t)lens[a] * 3}};
          const long t = yfi_plan_tiles_host(parent, 2, YF_PIX_RGB8, T, T, S, S, whole, NULL, NULL, NULL, 0);
          CHECK(t >= 2);
          yf_tile* tiles = exact((size_t)t * sizeof *tiles);
          yf_image* desc = exact((size_t)t * sizeof *desc);
          int32_t* first = exact(3 * sizeof *first);
          CHECK(yfi_plan_tiles_host(parent, 2, YF_PIX_RGB8, T, T, S, S, whole, tiles, desc, first, t) == t);
          CHECK(yfi_plan_tiles_host(parent, 2, YF_PIX_RGB8, T, T, S, S, whole, tiles, desc, first, t - 1) == -1);
          CHECK(first[0] == 0 && first[1] > 0 && first[1] < first[2] && first[2] == t);
          for (long j = 0; j < t; ++j) {
            const yf_image* p = &parent[j >= first[1]];
            CHECK(tiles[j].image == (j >= first[1]) && tiles[j].x0 >= 0 && tiles[j].y0 >= 0);
            CHECK(tiles[j].x0 + tiles[j].width <= p->width && tiles[j].y0 + tiles[j].height <= p->height);
            CHECK(desc[j].row_stride == p->row_stride && desc[j].height == tiles[j].height && desc[j].width == tiles[j].width);
            CHECK(desc[j].offset == p->offset + (uint64_t)tiles[j].y0 * (uint64_t)p->row_stride + (uint64_t)tiles[j].x0 * 3u);
          }
          free(tiles); free(desc); free(first);
        }
  }
  yf_image big = {0, 16384, 16384, 16384 * 4};
  CHECK(yfi_plan_tiles_host(&big, 1, YF_PIX_BGRA8, 8, 8, 1, 1, 1, NULL, NULL, NULL, 0) == 16377l * 16377l + 1);
  yf_image huge[8];
  for (int i = 0; i < 8; ++i) huge[i] = big;
  CHECK(yfi_plan_tiles_host(huge, 8, YF_PIX_BGRA8, 1, 1, 1, 1, 0, NULL, NULL, NULL, 0) == -1);           /* 2^31 tiles */
  yf_image odd = {UINT64_MAX - 3, 40, 40, INT64_MAX};                                                     /* the sums wrap, defined */
  yf_tile tl[26]; yf_image td[26]; int32_t fr[2];
  CHECK(yfi_plan_tiles_host(&odd, 1, YF_PIX_BGR8, 16, 16, 8, 8, 1, tl, td, fr, 26) == 17);
  odd.height = 0;
  CHECK(yfi_plan_tiles_host(&odd, 1, YF_PIX_BGR8, 16, 16, 8, 8, 1, tl, td, fr, 26) == -1);
  CHECK(yfi_plan_tiles_host(&big, 1, 9, 16, 16, 8, 8, 1, tl, td, fr, 26) == -1);
  CHECK(yfi_plan_tiles_host(&big, 1, 0, 16, 16, 17, 8, 1, tl, td, fr, 26) == -1);
  CHECK(yfi_plan_tiles_host(&big, 1, 0, 16, 0, 8, 8, 1, tl, td, fr, 26) == -1);
}

static int32_t edge(void) {
  const uint32_t k = rnd() % 20u;
  return k == 0 ? INT32_MIN : (k == 1 ? INT32_MAX : (k == 2 ? INT32_MAX - 5 : (int32_t)(rnd() % 22000u) - 2000));
}

/* t tiles of `cap` records, n + 1 entries of `first` (anything), merged into exactly n * out_cap records */
static void gather_case(long t, int cap, const int32_t* first, long n, int out_cap, int well_formed) {
  yf_det* dets = exact((size_t)t * (size_t)cap * sizeof *dets);
  int32_t* counts = exact((size_t)t * sizeof *counts);
  yf_tile* tiles = exact((size_t)t * sizeof *tiles);
  yf_det* out = exact((size_t)n * (size_t)out_cap * sizeof *out);
  int32_t* oc = exact((size_t)n * sizeof *oc);
  const int32_t pool[10] = {0, 0, 1, 2, cap, cap + 1, -1, INT32_MIN, INT32_MAX, cap / 2};
  for (long j = 0; j < t; ++j) {
    counts[j] = pool[rnd() % 10u];
    tiles[j] = (yf_tile){-5, j % 7 == 0 ? 16383 : (int32_t)(rnd() % 16384u), (int32_t)(rnd() % 16384u), 1, 1};
    for (int r = 0; r < cap; ++r) {
      yf_det* d = &dets[j * cap + r];
      d->frame = (int32_t)j; d->anchor = (uint8_t)rnd(); d->row = (uint8_t)rnd(); d->col = (uint8_t)rnd(); d->q_conf = (int8_t)rnd();
      d->conf = (float)(rnd() % 1000u) / 1000.f;
      d->x1 = edge(); d->y1 = edge(); d->x2 = edge(); d->y2 = edge();
    }
  }
  CHECK(yfi_gather_tiles_host(dets, counts, t, cap, tiles, first, n, out, oc, out_cap) == n);
  if (well_formed)
    for (long i = 0; i < n; ++i) {
      int64_t total = 0;
      for (long j = first[i]; j < first[i + 1]; ++j) {
        const int m = counts[j] < 0 ? 0 : (counts[j] > cap ? cap : counts[j]);
        for (int r = 0; r < m && total + r < out_cap; ++r) {
          const yf_det* s = &dets[j * cap + r];
          const yf_det* d = &out[i * out_cap + total + r];
          int64_t x1 = (int64_t)s->x1 + tiles[j].x0, y2 = (int64_t)s->y2 + tiles[j].y0;
          if (x1 > INT32_MAX) x1 = INT32_MAX;
          if (y2 > INT32_MAX) y2 = INT32_MAX;
          CHECK(d->frame == i && d->x1 == x1 && d->y2 == y2 && d->anchor == s->anchor && d->q_conf == s->q_conf);
          CHECK(memcmp(&d->conf, &s->conf, 4) == 0);
        }
        total += m;
      }
      CHECK(oc[i] == total);
      const unsigned char* raw = (const unsigned char*)out;
      for (int64_t k = total < out_cap ? total : out_cap; k < out_cap; ++k) CHECK(raw[((size_t)i * out_cap + k) * 28] == 0xA5);
    }
  free(dets); free(counts); free(tiles); free(out); free(oc);
}

int main(void) {
  plan_cases();
  const int caps[3] = {1, 147, 1200};
  const int32_t per_image[9] = {0, 1, 63, 64, 65, 255, 256, 257, 3};
  int32_t first[10] = {0};
  for (int i = 0; i < 9; ++i) first[i + 1] = first[i] + per_image[i];
  const long t = first[9];
  for (int c = 0; c < 3; ++c) {
    const int out_caps[4] = {1, caps[c], caps[c] + 1 > 1200 ? 1199 : caps[c] + 1, 1200};
    for (int o = 0; o < 4; ++o) gather_case(t, caps[c], first, 9, out_caps[o], 1);
    gather_case(t, caps[c], first, 0, 5, 1);                                                  /* n = 0 */
    gather_case(0, caps[c], (const int32_t[4]){0, 0, 0, 0}, 3, 5, 0);                         /* t = 0 */
  }
  /* malformed `first`: exact buffers, any content */
  const int32_t descending[5] = {40, 30, 20, 10, 0};
  const int32_t negative[5] = {-7, -1, INT32_MIN, 5, -2};
  const int32_t beyond[5] = {0, 39, 41, 4000, INT32_MAX};
  const int32_t overlapping[5] = {0, 30, 10, 40, 40};
  const int32_t all_of_it[5] = {INT32_MIN, INT32_MAX, INT32_MIN, INT32_MAX, 0};
  const int32_t* bad[5] = {descending, negative, beyond, overlapping, all_of_it};
  for (int k = 0; k < 5; ++k)
    for (int c = 0; c < 3; ++c) { gather_case(40, caps[c], bad[k], 4, 7, 0); gather_case(40, caps[c], bad[k], 4, 1200, 0); }
  printf("tiles: ok\n");
  return 0;
}
