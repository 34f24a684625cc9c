/* The host build of the appearance descriptors and of the re-identification (csrc/yf_images_describe.h, csrc/yf_images_reid.h through
 * csrc/yf_images_host.c) under ASan + UBSan: a program of its own, compiled together with yf_images_host.c by
 * tests/test_reid_sanitize.py.  The pixel buffer, the picture descriptors, the records, the counts, the descriptors, the states, the
 * infos, the kinds and the status are allocations of exactly their extent, so a load or a store one byte before or past one of them is a
 * report, and a signed overflow in the region arithmetic or the distance is one too.  Inputs: pictures that end with the buffer's last
 * byte, in all six formats, with odd strides; records of random bytes, at the int32 extremes and small ones inside the picture; counts of
 * every kind (negative, 0, the cap, above it, the int32 extremes); picture descriptors of random bytes (refused one by one); states of
 * random bytes, states with duplicated aliases and a clock at UINT32_MAX, tracker ids of random bytes, 0, small ones that repeat;
 * descriptors of random bytes (flags too) and all-0 / all-255 ones (the largest distance); out_cap 1, 64 and 70; both layouts; d_info_out
 * the input itself; d_what and d_status given or NULL; and calls the checks refuse, which must touch nothing (their arrays have been
 * freed). */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/yf_images.h"

long yfi_describe_records_host(const uint8_t* base, uint64_t bytes, int format, const yf_image* images, const yf_det* dets, const int32_t* counts,
                               long n, int cap, int margin_permille, int flags, yf_face_desc* desc, int32_t* first, int32_t* status);
long yfi_describe_records_yuv_host(const uint8_t* base, uint64_t bytes, int format, const yf_image_yuv* images, const yf_det* dets,
                                   const int32_t* counts, long n, int cap, int margin_permille, int flags, yf_face_desc* desc, int32_t* first,
                                   int32_t* status);
long yf_images_reid_host(const void* info, const void* out_counts, const void* desc, int out_cap, long streams, long steps, int layout,
                         const yf_reid_params* params, void* state, void* info_out, int32_t* what, int32_t* status, void* stream);
size_t yf_images_reid_state_bytes_host(long streams);
int32_t yfi_reid_distance_host(const uint8_t* a, const uint8_t* b);

static uint32_t g_seed = 9191u;
static uint32_t rnd(void) { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

#define CHECK(c) do { if (!(c)) { printf("reid: FAILED %s (line %d)\n", #c, __LINE__); exit(1); } } while (0)

static void* exact(size_t bytes, int random) {
  uint8_t* p = malloc(bytes ? bytes : 1);
  CHECK(p);
  for (size_t i = 0; i < bytes; ++i) p[i] = random ? (uint8_t)rnd() : 0xA5;
  return p;
}

static long g_calls = 0;
static const int32_t EDGE[8] = {INT32_MIN, INT32_MIN + 1, -1, 0, 1, 7, INT32_MAX - 1, INT32_MAX};
static const int32_t COUNTS[10] = {INT32_MIN, -1, 0, 1, 2, 63, 64, 65, 1000, INT32_MAX};

/* ---- descriptors ----  n pictures of h x w laid end to end, the last ending with the buffer; box_kind 0: random bytes, 1: extremes,
 * 2: inside the picture; desc_kind 0: valid descriptors, 1: random bytes */
static void describe(int format, long n, int h, int w, int pad, int cap, int box_kind, int count_kind, int desc_kind, int margin, int flags) {
  const int yuv = format >= YF_PIX_NV12, C = yuv ? 1 : (format >= YF_PIX_BGRA8 ? 4 : 3);
  const size_t stride = (size_t)w * (size_t)C + (size_t)pad;
  const size_t plane = stride * (size_t)(h - 1) + (size_t)w * (size_t)C;              /* the last row has no padding behind it */
  const size_t plane_uv = yuv ? stride * (size_t)(h / 2 - 1) + (size_t)w : 0;
  const size_t bytes = (size_t)n * (plane + plane_uv);
  uint8_t* px = exact(bytes, 1);
  yf_image* im = yuv ? NULL : exact(sizeof(yf_image) * (size_t)n, desc_kind);
  yf_image_yuv* iy = yuv ? exact(sizeof(yf_image_yuv) * (size_t)n, desc_kind) : NULL;
  for (long i = 0; desc_kind == 0 && i < n; ++i) {
    const size_t at = (size_t)i * (plane + plane_uv);
    if (yuv) { iy[i].offset_y = at; iy[i].offset_uv = at + plane; iy[i].height = h; iy[i].width = w; iy[i].stride_y = (int64_t)stride; iy[i].stride_uv = (int64_t)stride; }
    else { im[i].offset = at; im[i].height = h; im[i].width = w; im[i].row_stride = (int64_t)stride; }
  }
  yf_det* dets = exact(sizeof(yf_det) * (size_t)n * (size_t)cap, 1);
  int32_t* counts = exact(4 * (size_t)n, 0);
  for (long i = 0; i < n; ++i) {
    counts[i] = count_kind == 0 ? COUNTS[rnd() % 10u] : count_kind == 1 ? cap : (int32_t)(rnd() % (uint32_t)(cap + 1));
    for (int j = 0; j < cap; ++j) {
      yf_det* d = &dets[(size_t)i * (size_t)cap + (size_t)j];
      if (box_kind == 1) { d->x1 = EDGE[rnd() % 8u]; d->y1 = EDGE[rnd() % 8u]; d->x2 = EDGE[rnd() % 8u]; d->y2 = EDGE[rnd() % 8u]; }
      if (box_kind == 2) { d->x1 = (int32_t)(rnd() % (uint32_t)w) - 3; d->y1 = (int32_t)(rnd() % (uint32_t)h) - 3; d->x2 = d->x1 + (int32_t)(rnd() % 40u);
                           d->y2 = d->y1 + (int32_t)(rnd() % 40u); }
    }
  }
  yf_face_desc* desc = exact(sizeof(yf_face_desc) * (size_t)n * (size_t)cap, 0);
  int32_t* first = exact(4 * (size_t)(n + 1), 0);
  int32_t* status = exact(4 * (size_t)n, 0);
  const long rc = yuv ? yfi_describe_records_yuv_host(px, bytes, format, iy, dets, counts, n, cap, margin, flags, desc, first, status)
                      : yfi_describe_records_host(px, bytes, format, im, dets, counts, n, cap, margin, flags, desc, first, status);
  CHECK(rc == n && first[0] == 0);
  for (long i = 0; i < n; ++i) {
    const int m = counts[i] < 0 ? 0 : counts[i] > cap ? cap : counts[i];
    CHECK(first[i + 1] - first[i] == m && (status[i] == 0 || status[i] == 1) && (desc_kind == 1 || status[i] == 0));
    for (int j = 0; j < cap; ++j) {
      const yf_face_desc* d = &desc[(size_t)i * (size_t)cap + (size_t)j];
      CHECK(j < m ? d->flags <= 1u : d->flags == 0xA5A5A5A5u);
      if (j < m && d->flags == 0) for (int k = 0; k < YF_DESC_BYTES; ++k) CHECK(d->v[k] == 0);
      if (j < m && status[i] == 1) CHECK(d->flags == 0);
    }
  }
  free(px); free(im); free(iy); free(dets); free(counts); free(desc); free(first); free(status);
  ++g_calls;
}

/* ---- re-identification ----  state_kind 0: zero, 1: random bytes, 2: random bytes with the aliases drawn from 1 .. 6 and the clock at
 * UINT32_MAX; id_kind 0: random bytes, 1: 0 .. 6 (void ones, repeats, the aliases of kind 2); desc_kind 0: random bytes, flags too, 1:
 * valid and all 0 or all 255 in halves; in_place: d_info_out is d_info */
static void reid(long streams, long steps, int layout, int out_cap, int state_kind, int id_kind, int desc_kind, int count_kind, int with_outputs,
                 int in_place, yf_reid_params p) {
  const size_t n = (size_t)(streams * steps);
  yf_track_info* info = exact(sizeof(yf_track_info) * n * (size_t)out_cap, 1);
  yf_face_desc* desc = exact(sizeof(yf_face_desc) * n * (size_t)out_cap, 1);
  int32_t* counts = exact(4 * n, 0);
  yf_track_info* info_out = in_place ? info : exact(sizeof(yf_track_info) * n * (size_t)out_cap, 0);
  int32_t* what = with_outputs ? exact(4 * n * (size_t)out_cap, 0) : NULL;
  int32_t* status = with_outputs ? exact(4 * n, 0) : NULL;
  yf_reid_state* st = exact(sizeof(yf_reid_state) * (size_t)streams, state_kind != 0);
  if (state_kind == 0) memset(st, 0, sizeof(yf_reid_state) * (size_t)streams);
  for (long s = 0; state_kind == 2 && s < streams; ++s) {
    st[s].clock = UINT32_MAX;
    for (int e = 0; e < YF_REID_ENTRIES; ++e) st[s].entry[e].alias = 1u + rnd() % 6u;
  }
  for (size_t f = 0; f < n; ++f) {
    counts[f] = count_kind == 0 ? COUNTS[rnd() % 10u] : count_kind == 1 ? out_cap : (int32_t)(rnd() % (uint32_t)(out_cap + 1));
    for (int j = 0; j < out_cap; ++j) {
      const size_t at = f * (size_t)out_cap + (size_t)j;
      if (id_kind == 1) { info[at].id = rnd() % 7u; info[at].misses = (int32_t)(rnd() % 3u) - 1; }
      if (desc_kind == 1) { desc[at].flags = 1u; for (int k = 0; k < YF_DESC_BYTES; ++k) desc[at].v[k] = ((k < 32) == ((j & 1) != 0)) ? 255 : 0; }
    }
  }
  const uint32_t clock0 = st[0].clock;
  CHECK(yf_images_reid_host(info, counts, desc, out_cap, streams, steps, layout, &p, st, info_out, what, status, NULL) == streams * steps);
  CHECK(st[0].clock == clock0 + (uint32_t)steps);
  for (size_t f = 0; with_outputs && f < n; ++f) {
    const int all = counts[f] < 0 ? 0 : counts[f] > out_cap ? out_cap : counts[f];
    CHECK(status[f] >= 0 && status[f] <= 3);
    for (int j = 0; j < out_cap; ++j) {
      const int32_t k = what[f * (size_t)out_cap + (size_t)j];
      CHECK(j < all ? (k >= 0 && k <= 3 && (j < 64 || k == 0)) : k == -1515870811);        /* 0xA5A5A5A5: not written */
      if (!in_place && j >= all) CHECK(info_out[f * (size_t)out_cap + (size_t)j].id == 0xA5A5A5A5u);
    }
  }
  free(info); free(desc); free(counts); if (!in_place) free(info_out);
  free(what); free(status); free(st);
  ++g_calls;
}

/* calls the checks refuse: their arrays have been freed, so any access is a report */
static void refused(void) {
  void* p[8];
  for (int k = 0; k < 8; ++k) p[k] = exact(64, 0);
  for (int k = 0; k < 8; ++k) free(p[k]);
  const yf_reid_params ok = {1000, 30, 64}, far = {-1, 30, 64}, old = {1000, -1, 64}, mix = {1000, 30, 257};
  CHECK(yf_images_reid_host(p[0], p[1], p[2], 0, 1, 1, 0, &ok, p[3], p[4], NULL, NULL, NULL) == -1);
  CHECK(yf_images_reid_host(p[0], p[1], p[2], 4, 1, 1, 2, &ok, p[3], p[4], NULL, NULL, NULL) == -1);
  CHECK(yf_images_reid_host(p[0], p[1], p[2], 4, 1, 1, 0, &far, p[3], p[4], NULL, NULL, NULL) == -1);
  CHECK(yf_images_reid_host(p[0], p[1], p[2], 4, 1, 1, 0, &old, p[3], p[4], NULL, NULL, NULL) == -1);
  CHECK(yf_images_reid_host(p[0], p[1], p[2], 4, 1, 1, 0, &mix, p[3], p[4], NULL, NULL, NULL) == -1);
  CHECK(yf_images_reid_host(p[0], p[1], p[2], 4, 1, 1, 0, NULL, p[3], p[4], NULL, NULL, NULL) == -1);
  CHECK(yf_images_reid_host(p[0], p[1], p[2], 4, -1, 1, 0, &ok, p[3], p[4], NULL, NULL, NULL) == -1);
  CHECK(yf_images_reid_host(p[0], p[1], p[2], 4, 65536, 32768, 0, &ok, p[3], p[4], NULL, NULL, NULL) == -1);
  CHECK(yf_images_reid_host(NULL, p[1], p[2], 4, 1, 1, 0, &ok, p[3], p[4], NULL, NULL, NULL) == -1);
  CHECK(yf_images_reid_host(p[0], p[1], p[2], 4, 1, 1, 0, &ok, NULL, p[4], NULL, NULL, NULL) == -1);
  CHECK(yf_images_reid_host(p[0], p[1], (char*)p[2] + 2, 4, 1, 1, 0, &ok, p[3], p[4], NULL, NULL, NULL) == -1);
  CHECK(yf_images_reid_host(p[0], p[1], p[2], 4, 1, 1, 0, &ok, (char*)p[3] + 4, p[4], NULL, NULL, NULL) == -1);
  /* an empty batch is taken after the checks and touches nothing either */
  CHECK(yf_images_reid_host(p[0], p[1], p[2], 4, 0, 5, 0, &ok, p[3], p[4], NULL, NULL, NULL) == 0);
  CHECK(yf_images_reid_host(p[0], p[1], p[2], 4, 3, 0, 1, &ok, p[3], p[4], NULL, NULL, NULL) == 0);
  CHECK(yf_images_reid_state_bytes_host(2) == 2 * sizeof(yf_reid_state) && yf_images_reid_state_bytes_host(0) == 0);
  CHECK(yfi_describe_records_host(p[0], 64, YF_PIX_NV12, p[1], p[2], p[3], 1, 4, 0, 0, p[4], p[5], p[6]) == -1);
  CHECK(yfi_describe_records_yuv_host(p[0], 64, YF_PIX_BGR8, p[1], p[2], p[3], 1, 4, 0, 0, p[4], p[5], p[6]) == -1);
  CHECK(yfi_describe_records_host(p[0], 64, YF_PIX_BGR8, p[1], p[2], p[3], 1, 0, 0, 0, p[4], p[5], p[6]) == -1);
  CHECK(yfi_describe_records_host(p[0], 64, YF_PIX_BGR8, p[1], p[2], p[3], -1, 4, 0, 0, p[4], p[5], p[6]) == -1);
  CHECK(yfi_describe_records_host(p[0], 64, YF_PIX_BGR8, p[1], p[2], p[3], 1, 4, 1001, 0, p[4], p[5], p[6]) == -1);
  CHECK(yfi_describe_records_host(p[0], 64, YF_PIX_BGR8, p[1], p[2], p[3], 1, 4, 0, 2, p[4], p[5], p[6]) == -1);
  CHECK(yfi_describe_records_host(p[0], 64, YF_PIX_BGR8, p[1], p[2], p[3], 1, 4, 0, 0, NULL, p[5], p[6]) == -1);
  CHECK(yfi_describe_records_host(p[0], 64, YF_PIX_BGR8, (char*)p[1] + 4, p[2], p[3], 1, 4, 0, 0, p[4], p[5], p[6]) == -1);
  CHECK(yfi_describe_records_host(p[0], 64, YF_PIX_BGR8, p[1], p[2], p[3], 0, 4, 0, 0, p[4], p[5], p[6]) == 0);
  g_calls += 24;
}

int main(void) {
  static const int CAPS[3] = {1, 64, 70};
  for (int format = 0; format < 6; ++format)
    for (int box_kind = 0; box_kind < 3; ++box_kind)
      for (int desc_kind = 0; desc_kind < 2; ++desc_kind) {
        const int yuv = format >= 4, h = yuv ? 2 * (4 + (int)(rnd() % 20u)) : 8 + (int)(rnd() % 40u), w = yuv ? 2 * (4 + (int)(rnd() % 30u)) : 8 + (int)(rnd() % 60u);
        describe(format, 1 + (long)(rnd() % 3u), h, w, (int)(rnd() % 4u), 1 + (int)(rnd() % 6u), box_kind, (int)(rnd() % 3u), desc_kind,
                 (int)(rnd() % 3u) * 500, (int)(rnd() % 2u));
      }
  describe(YF_PIX_RGB8, 1, 8, 8, 0, 2, 2, 1, 0, 1000, 1);
  for (int layout = 0; layout < 2; ++layout)
    for (int state_kind = 0; state_kind < 3; ++state_kind)
      for (int id_kind = 0; id_kind < 2; ++id_kind)
        for (int desc_kind = 0; desc_kind < 2; ++desc_kind)
          for (int in_place = 0; in_place < 2; ++in_place) {
            const yf_reid_params p = {(int32_t)(rnd() % 3u) * 522240, (int32_t)(rnd() % 3u), (int32_t)(rnd() % 3u) * 128};
            reid(1 + (long)(rnd() % 3u), 1 + (long)(rnd() % 5u), layout, CAPS[rnd() % 3u], state_kind, id_kind, desc_kind, (int)(rnd() % 3u),
                 (int)(rnd() % 2u), in_place, p);
          }
  /* the full frame against the full table, every distance eligible; and the largest parameters */
  for (int layout = 0; layout < 2; ++layout) {
    const yf_reid_params wide = {INT32_MAX, INT32_MAX, 256}, tight = {0, 0, 0};
    reid(2, 4, layout, 64, 1, 0, 1, 1, 1, 0, wide);
    reid(2, 4, layout, 70, 2, 1, 1, 1, 1, 1, wide);
    reid(1, 6, layout, 64, 1, 0, 0, 1, 1, 0, tight);
  }
  uint8_t* a = exact(64, 0);
  uint8_t* b = exact(64, 0);
  for (int k = 0; k < 64; ++k) { a[k] = k < 32 ? 255 : 0; b[k] = k < 32 ? 0 : 255; }
  CHECK(yfi_reid_distance_host(a, b) == 64 * 64 * 255 && yfi_reid_distance_host(a, a) == 0);
  free(a); free(b);
  refused();
  printf("reid: ok (%ld calls)\n", g_calls);
  return 0;
}
