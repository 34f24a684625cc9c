/* The host build of the score of tracks against labelled identities (csrc/yf_images_score.h through csrc/yf_images_host.c) under ASan +
 * UBSan: a program of its own, compiled together with yf_images_host.c by tests/test_track_score_sanitize.py.  The states, the
 * ground-truth rows, the records, the infos, the counts, the matches and the status are allocations of exactly their extent, so a load
 * or a store one byte before or past one of them is a report -- the state is indexed by ground-truth ids, which are untrusted -- and a
 * signed overflow in a saturating counter or in the search is one too.  Inputs: states of random bytes and states with every counter at
 * UINT64_MAX and every table entry at INT32_MAX; ids of random bytes, ids drawn from {0, 1, 2, 255, 256, 257, INT32_MAX, UINT32_MAX} and
 * small ids that repeat; boxes of random bytes, boxes with int32 extremes, small boxes that meet each other and 64 x 64 identical boxes;
 * counts of every kind (negative, 0, the cap, above it, the int32 extremes); gt_cap 1, 7 and 64, out_cap 1, 64 and 70; both layouts;
 * d_match and d_status given or NULL; the summary over every state; and calls the check refuses, which must touch nothing (their arrays
 * have been freed). */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/yf_images.h"

long yf_images_score_tracks_host(const void* out, const void* info, const void* out_counts, int out_cap, const void* gt, const void* gt_counts,
                                 int gt_cap, long streams, long steps, int layout, double score_iou, void* state, int32_t* match,
                                 int32_t* status, void* stream);
int yf_images_score_summary_host(const void* host_states, long streams, yf_score_summary* out);
size_t yf_images_score_state_bytes_host(long streams);

static uint32_t g_seed = 8181u;
static uint32_t rnd(void) { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

#define CHECK(c) do { if (!(c)) { printf("score: FAILED %s (line %d)\n", #c, __LINE__); exit(1); } } while (0)

static void* exact(size_t bytes, int random) {
  uint8_t* p = malloc(bytes ? bytes : 1);
  CHECK(p);
  for (size_t i = 0; i < bytes; ++i) p[i] = random ? (uint8_t)rnd() : 0xA5;
  return p;
}

static long g_calls = 0;
static const int32_t EDGE[8] = {INT32_MIN, INT32_MIN + 1, -1, 0, 1, 7, INT32_MAX - 1, INT32_MAX};
static const uint32_t IDS[8] = {0u, 1u, 2u, 255u, 256u, 257u, (uint32_t)INT32_MAX, UINT32_MAX};
static const int32_t COUNTS[10] = {INT32_MIN, -1, 0, 1, 2, 63, 64, 65, 1000, INT32_MAX};

/* kind 0: random bytes; 1: extremes; 2: small boxes near the origin, which meet each other; 3: all the box (12, 10, 51, 59) */
static void box_of(int32_t* b, int kind) {
  if (kind == 1) for (int e = 0; e < 4; ++e) b[e] = EDGE[rnd() % 8u];
  if (kind == 2) { b[0] = (int32_t)(rnd() % 60u); b[1] = (int32_t)(rnd() % 60u); b[2] = b[0] + 5 + (int32_t)(rnd() % 40u); b[3] = b[1] + 5 + (int32_t)(rnd() % 40u); }
  if (kind == 3) { b[0] = 12; b[1] = 10; b[2] = 51; b[3] = 59; }
}

/* ids 0: random bytes; 1: drawn from IDS; 2: 1 .. 12, which repeat; 3: 1 + the place in its row (distinct) */
static uint32_t id_of(uint32_t now, int kind, int place) {
  return kind == 0 ? now : kind == 1 ? IDS[rnd() % 8u] : kind == 2 ? 1u + rnd() % 12u : 1u + (uint32_t)place;
}

/* states 0: zero; 1: random bytes; 2: every counter at UINT64_MAX, every entry of present and tracked at INT32_MAX, last small ids */
static yf_score_state* states_of(long streams, int kind) {
  yf_score_state* st = exact(sizeof(yf_score_state) * (size_t)streams, kind == 1);
  if (kind == 1) return st;
  memset(st, 0, sizeof(yf_score_state) * (size_t)streams);
  if (kind == 2)
    for (long s = 0; s < streams; ++s) {
      st[s].frames = st[s].gt = st[s].hyp = st[s].matches = st[s].misses = st[s].false_positives = st[s].switches = st[s].overlap = UINT64_MAX;
      for (int o = 0; o < YF_SCORE_MAX_IDS; ++o) { st[s].last[o] = 1u + rnd() % 12u; st[s].present[o] = INT32_MAX; st[s].tracked[o] = INT32_MAX; }
    }
  return st;
}

static void summarise(const yf_score_state* st, long streams) {
  yf_score_summary* out = exact(sizeof *out, 0);
  CHECK(yf_images_score_summary_host(st, streams, out) == 0);
  CHECK(out->objects >= 0 && out->objects <= streams * YF_SCORE_MAX_IDS && out->mostly_tracked <= out->objects && out->mostly_lost <= out->objects);
  CHECK(out->mota == out->mota && out->motp == out->motp && out->motp >= 0.0);
  free(out);
  uint8_t* odd = exact(sizeof(yf_score_state) * (size_t)streams + 1, 0);          /* any alignment */
  yf_score_summary again;
  memcpy(odd + 1, st, sizeof(yf_score_state) * (size_t)streams);
  CHECK(yf_images_score_summary_host(odd + 1, streams, &again) == 0);
  free(odd);
}

static void run(long streams, long steps, int layout, int gt_cap, int out_cap, double score_iou, int state_kind, int id_kind, int box_kind,
                int count_kind, int with_outputs) {
  const size_t n = (size_t)(streams * steps);
  yf_gt_track* gt = exact(sizeof(yf_gt_track) * n * (size_t)gt_cap, 1);
  yf_det* out = exact(sizeof(yf_det) * n * (size_t)out_cap, 1);
  yf_track_info* info = exact(sizeof(yf_track_info) * n * (size_t)out_cap, 1);
  int32_t* gt_counts = exact(4 * n, 0);
  int32_t* out_counts = exact(4 * n, 0);
  int32_t* match = with_outputs ? exact(4 * n * (size_t)gt_cap, 0) : NULL;
  int32_t* status = with_outputs ? exact(4 * n, 0) : NULL;
  yf_score_state* st = states_of(streams, state_kind);
  for (size_t f = 0; f < n; ++f) {
    gt_counts[f] = count_kind == 0 ? COUNTS[rnd() % 10u] : count_kind == 1 ? gt_cap : (int32_t)(rnd() % (uint32_t)(gt_cap + 1));
    out_counts[f] = count_kind == 0 ? COUNTS[rnd() % 10u] : count_kind == 1 ? out_cap : (int32_t)(rnd() % (uint32_t)(out_cap + 1));
    for (int i = 0; i < gt_cap; ++i) {
      yf_gt_track* r = &gt[f * (size_t)gt_cap + (size_t)i];
      int32_t b[4] = {r->x1, r->y1, r->x2, r->y2};
      box_of(b, box_kind);
      r->id = id_of(r->id, id_kind, i); r->x1 = b[0]; r->y1 = b[1]; r->x2 = b[2]; r->y2 = b[3];
    }
    for (int j = 0; j < out_cap; ++j) {
      yf_det* d = &out[f * (size_t)out_cap + (size_t)j];
      int32_t b[4] = {d->x1, d->y1, d->x2, d->y2};
      box_of(b, box_kind);
      d->x1 = b[0]; d->y1 = b[1]; d->x2 = b[2]; d->y2 = b[3];
      info[f * (size_t)out_cap + (size_t)j].id = id_of(info[f * (size_t)out_cap + (size_t)j].id, id_kind, 63 - j % 64);
    }
  }
  const uint64_t frames0 = st[0].frames;
  CHECK(yf_images_score_tracks_host(out, info, out_counts, out_cap, gt, gt_counts, gt_cap, streams, steps, layout, score_iou, st, match, status, NULL)
        == streams * steps);
  CHECK(st[0].frames == frames0 + (uint64_t)steps);
  for (size_t f = 0; with_outputs && f < n; ++f) {
    const int lim = gt_cap < 64 ? gt_cap : 64, g = gt_counts[f] < 0 ? 0 : gt_counts[f] > lim ? lim : gt_counts[f];
    CHECK(status[f] >= 0 && status[f] <= 15);
    for (int i = 0; i < gt_cap; ++i) {
      const int32_t m = match[f * (size_t)gt_cap + (size_t)i];
      CHECK(i < g ? (m >= -1 && m < 64 && m < out_cap) : m == -1515870811);             /* 0xA5A5A5A5: not written */
    }
  }
  if (state_kind == 0 && id_kind == 3 && box_kind == 3 && count_kind == 1 && gt_cap == 64 && out_cap >= 64)          /* every pair at IoU 1 */
    for (long s = 0; s < streams; ++s) CHECK(st[s].matches == 64u * (uint64_t)steps && st[s].misses == 0 && st[s].overlap == st[s].matches * ((1u << 30) + 1u));
  summarise(st, streams);
  free(gt); free(out); free(info); free(gt_counts); free(out_counts); free(match); free(status); free(st);
  ++g_calls;
}

/* calls the check refuses: their arrays have been freed, so any access is a report */
static void refused(void) {
  void* p[6];
  for (int k = 0; k < 6; ++k) { p[k] = exact(64, 0); }
  for (int k = 0; k < 6; ++k) free(p[k]);
  const double nan_iou = NAN;
  CHECK(yf_images_score_tracks_host(p[0], p[1], p[2], 0, p[3], p[4], 4, 1, 1, 0, 0.5, p[5], NULL, NULL, NULL) == -1);
  CHECK(yf_images_score_tracks_host(p[0], p[1], p[2], 4, p[3], p[4], 0, 1, 1, 0, 0.5, p[5], NULL, NULL, NULL) == -1);
  CHECK(yf_images_score_tracks_host(p[0], p[1], p[2], 4, p[3], p[4], 65, 1, 1, 0, 0.5, p[5], NULL, NULL, NULL) == -1);
  CHECK(yf_images_score_tracks_host(p[0], p[1], p[2], 4, p[3], p[4], 4, 1, 1, 2, 0.5, p[5], NULL, NULL, NULL) == -1);
  CHECK(yf_images_score_tracks_host(p[0], p[1], p[2], 4, p[3], p[4], 4, 1, 1, 0, nan_iou, p[5], NULL, NULL, NULL) == -1);
  CHECK(yf_images_score_tracks_host(p[0], p[1], p[2], 4, p[3], p[4], 4, -1, 1, 0, 0.5, p[5], NULL, NULL, NULL) == -1);
  CHECK(yf_images_score_tracks_host(p[0], p[1], p[2], 4, p[3], p[4], 4, 65536, 32768, 0, 0.5, p[5], NULL, NULL, NULL) == -1);
  CHECK(yf_images_score_tracks_host(NULL, p[1], p[2], 4, p[3], p[4], 4, 1, 1, 0, 0.5, p[5], NULL, NULL, NULL) == -1);
  CHECK(yf_images_score_tracks_host(p[0], p[1], p[2], 4, p[3], p[4], 4, 1, 1, 0, 0.5, NULL, NULL, NULL, NULL) == -1);
  CHECK(yf_images_score_tracks_host(p[0], p[1], p[2], 4, (char*)p[3] + 2, p[4], 4, 1, 1, 0, 0.5, p[5], NULL, NULL, NULL) == -1);
  CHECK(yf_images_score_tracks_host(p[0], p[1], p[2], 4, p[3], p[4], 4, 1, 1, 0, 0.5, (char*)p[5] + 4, NULL, NULL, NULL) == -1);
  /* an empty batch is taken after the checks and touches nothing either */
  CHECK(yf_images_score_tracks_host(p[0], p[1], p[2], 4, p[3], p[4], 4, 0, 5, 0, 0.5, p[5], NULL, NULL, NULL) == 0);
  CHECK(yf_images_score_tracks_host(p[0], p[1], p[2], 4, p[3], p[4], 4, 3, 0, 1, 0.5, p[5], NULL, NULL, NULL) == 0);
  CHECK(yf_images_score_summary_host(NULL, 1, NULL) == -1 && yf_images_score_summary_host(p[0], -1, NULL) == -1);
  CHECK(yf_images_score_state_bytes_host(2) == 2 * sizeof(yf_score_state) && yf_images_score_state_bytes_host(0) == 0);
  g_calls += 13;
}

int main(void) {
  static const int GT_CAPS[3] = {1, 7, 64}, OUT_CAPS[3] = {1, 64, 70};
  static const double IOUS[4] = {0.0, 0.3, 0.5, 1.0};
  for (int layout = 0; layout < 2; ++layout)
    for (int state_kind = 0; state_kind < 3; ++state_kind)
      for (int id_kind = 0; id_kind < 4; ++id_kind)
        for (int box_kind = 0; box_kind < 4; ++box_kind) {
          const int c = (int)(rnd() % 3u), o = (int)(rnd() % 3u);
          run(1 + (long)(rnd() % 3u), 1 + (long)(rnd() % 4u), layout, GT_CAPS[c], OUT_CAPS[o], IOUS[rnd() % 4u], state_kind, id_kind, box_kind,
              (int)(rnd() % 3u), (int)(rnd() % 2u));
        }
  /* the dense tables: every pair eligible at one weight, and small boxes that meet each other under ids that repeat */
  for (int layout = 0; layout < 2; ++layout) {
    run(2, 3, layout, 64, 64, 0.5, 0, 3, 3, 1, 1);
    run(1, 2, layout, 64, 70, 0.5, 2, 3, 3, 1, 1);
    run(2, 4, layout, 64, 64, 0.0, 1, 2, 2, 1, 1);
    run(3, 5, layout, 64, 64, 0.1, 2, 1, 2, 0, 1);
    run(2, 6, layout, 7, 64, 0.2, 2, 2, 2, 2, 0);
  }
  refused();
  printf("score: ok (%ld calls)\n", g_calls);
  return 0;
}
