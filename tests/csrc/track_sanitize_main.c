/* The host build of the tracker (csrc/yf_images_track.h through csrc/yf_images_host.c) under ASan + UBSan: a program of its own,
 * compiled together with yf_images_host.c by tests/test_track_sanitize.py.  The states, the record rows, the counts and every output
 * array are allocations of exactly their extent, so a load or a store one byte before or past one of them is a report, and signed
 * overflow in a counter or an edge difference is one too.  Inputs: states of random bytes (ids, counters and boxes of any value), states
 * whose counters sit at INT32_MAX and INT32_MIN and whose `issued` is about to wrap, full tables; records with INT32_MIN / INT32_MAX edges,
 * empty and inverted boxes and random bytes; counts of 0, below 0, above cap, above 64 and at the int32 extremes; cap 1, 64, 70 and 1200;
 * out_cap 1, 3 and 64; both layouts; match_iou from -1 to infinity, min_hits and max_misses up to INT32_MAX; with and without a status
 * array; and calls the check refuses, which must touch nothing (their arrays have been freed). */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/yf_images.h"

long yf_images_track_host(const void* dets, const void* counts, long streams, long steps, int layout, int cap, const yf_track_params* params,
                          void* state, void* out, void* info, void* out_counts, int out_cap, int32_t* status, void* stream);

static uint32_t g_seed = 5757u;
static uint32_t rnd(void) { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

#define CHECK(c) do { if (!(c)) { printf("track: FAILED %s (line %d)\n", #c, __LINE__); exit(1); } } while (0)

static void* exact(size_t bytes, int random) {
  uint8_t* p = malloc(bytes ? bytes : 1);
  CHECK(p);
  for (size_t i = 0; i < bytes; ++i) p[i] = random ? (uint8_t)rnd() : 0xA5;
  return p;
}

static const int32_t EDGE[8] = {INT32_MIN, INT32_MIN + 1, -1, 0, 1, 7, INT32_MAX - 1, INT32_MAX};

/* kind 0: random bytes; 1: edges drawn from EDGE (extremes, empty, inverted); 2: small boxes near the origin, which meet each other */
static void fill_records(yf_det* d, size_t count, int kind) {
  for (size_t i = 0; i < count; ++i) {
    if (kind == 0) continue;                                        /* `exact` made them random */
    if (kind == 1) { d[i].x1 = EDGE[rnd() % 8]; d[i].y1 = EDGE[rnd() % 8]; d[i].x2 = EDGE[rnd() % 8]; d[i].y2 = EDGE[rnd() % 8]; }
    else { d[i].x1 = (int32_t)(rnd() % 40u); d[i].y1 = (int32_t)(rnd() % 40u); d[i].x2 = d[i].x1 + (int32_t)(rnd() % 12u) - 1; d[i].y2 = d[i].y1 + (int32_t)(rnd() % 12u) - 1; }
  }
}

/* kind 0: zero; 1: random bytes; 2: random bytes with every id non-zero (a full table); 3: counters at the extremes, issued about to wrap */
static void fill_states(yf_track_state* st, long streams, int kind) {
  for (long s = 0; s < streams; ++s) {
    if (kind == 0) memset(&st[s], 0, sizeof st[s]);
    if (kind == 2) for (int k = 0; k < YF_TRACK_SLOTS; ++k) st[s].slot[k].id |= 1u;
    if (kind == 3) {
      st[s].issued = 0xFFFFFFFFu - (uint32_t)(rnd() % 3u);
      for (int k = 0; k < YF_TRACK_SLOTS; ++k) {
        yf_track* t = &st[s].slot[k];
        t->id = k % 5 == 0 ? 0u : rnd();
        t->hits = k % 2 ? INT32_MAX : INT32_MIN; t->misses = k % 3 ? INT32_MAX : INT32_MIN; t->age = k % 4 ? INT32_MAX : -1;
        t->det.x1 = EDGE[rnd() % 8]; t->det.y1 = EDGE[rnd() % 8]; t->det.x2 = EDGE[rnd() % 8]; t->det.y2 = EDGE[rnd() % 8];
      }
    }
  }
}

static long g_calls = 0;

static void run(long streams, long steps, int layout, int cap, int out_cap, yf_track_params p, int state_kind, int rec_kind, int with_status) {
  const long n = streams * steps;
  yf_track_state* st = exact(sizeof(yf_track_state) * (size_t)streams, 1);
  yf_det* dets = exact(sizeof(yf_det) * (size_t)n * (size_t)cap, 1);
  int32_t* counts = exact(4 * (size_t)n, 0);
  yf_det* out = exact(sizeof(yf_det) * (size_t)n * (size_t)out_cap, 0);
  yf_track_info* info = exact(sizeof(yf_track_info) * (size_t)n * (size_t)out_cap, 0);
  int32_t* oc = exact(4 * (size_t)n, 0);
  int32_t* status = with_status ? exact(4 * (size_t)n, 0) : NULL;
  fill_states(st, streams, state_kind);
  fill_records(dets, (size_t)n * (size_t)cap, rec_kind);
  const int32_t special[8] = {0, -1, INT32_MIN, INT32_MAX, cap, cap + 1, 64, 65};
  for (long f = 0; f < n; ++f) counts[f] = rnd() % 3u == 0 ? special[rnd() % 8] : (int32_t)(rnd() % (uint32_t)(cap + 1));
  CHECK(yf_images_track_host(dets, counts, streams, steps, layout, cap, &p, st, out, info, oc, out_cap, status, NULL) == n);
  for (long f = 0; f < n; ++f) {
    CHECK(oc[f] >= 0 && oc[f] <= YF_TRACK_SLOTS);
    if (status) CHECK((status[f] & ~3) == 0 && ((status[f] & 1) != 0) == (counts[f] > (cap < 64 ? cap : 64)));
    for (int r = 0; r < out_cap; ++r) {
      const yf_det* o = &out[f * out_cap + r];
      const yf_track_info* i = &info[f * out_cap + r];
      if (r < oc[f]) {
        CHECK(o->frame == (int32_t)f && i->id != 0 && i->hits >= p.min_hits);
        CHECK(r == 0 || i[-1].id <= i->id);                         /* ascending id */
      } else {
        CHECK((uint32_t)o->frame == 0xA5A5A5A5u && i->id == 0xA5A5A5A5u);           /* not touched */
      }
    }
  }
  for (long s = 0; s < streams; ++s)
    for (int k = 0; k < YF_TRACK_SLOTS; ++k) {
      const yf_track* t = &st[s].slot[k];
      if (steps > 0 && t->id != 0 && state_kind != 1 && state_kind != 2) CHECK(t->misses <= p.max_misses || t->misses < 0 || p.max_misses == INT32_MAX);
    }
  free(st); free(dets); free(counts); free(out); free(info); free(oc); free(status);
  ++g_calls;
}

int main(void) {
  const yf_track_params params[6] = {{0.3, 1, 5}, {0.0, 1, 0}, {1.0, 3, 2}, {-1.0, INT32_MAX, INT32_MAX}, {INFINITY, 1, 1}, {0.5, 2, INT32_MAX}};
  const int caps[4] = {1, 64, 70, 1200}, out_caps[3] = {1, 3, 64};
  for (int sk = 0; sk < 4; ++sk)
    for (int rk = 0; rk < 3; ++rk)
      for (int c = 0; c < 4; ++c)
        for (int pi = 0; pi < 6; ++pi) {
          const int layout = (sk + rk + c + pi) & 1;
          run(1 + (pi % 3), 1 + (c + rk) % 4, layout, caps[c], out_caps[(sk + pi) % 3], params[pi], sk, rk, (c + pi) & 1);
        }
  run(5, 9, YF_TRACK_TIME_MAJOR, 70, 64, params[0], 0, 2, 1);      /* a longer clip from the empty state: tracks live and die */
  run(5, 9, YF_TRACK_STREAM_MAJOR, 70, 2, params[2], 0, 2, 1);
  run(0, 4, YF_TRACK_TIME_MAJOR, 8, 4, params[0], 0, 2, 1);        /* empty batches: nothing is read or written */
  run(3, 0, YF_TRACK_STREAM_MAJOR, 8, 4, params[0], 1, 2, 0);

  /* refused calls: the arrays are freed memory */
  void* gone = exact(64, 0);
  free(gone);
  yf_track_params p = {0.3, 1, 5}, nan_iou = {NAN, 1, 5}, no_hits = {0.3, 0, 5}, neg_misses = {0.3, 1, -1};
  CHECK(yf_images_track_host(gone, gone, 1, 1, 0, 0, &p, gone, gone, gone, gone, 4, NULL, NULL) == -1);
  CHECK(yf_images_track_host(gone, gone, 1, 1, 0, 1201, &p, gone, gone, gone, gone, 4, NULL, NULL) == -1);
  CHECK(yf_images_track_host(gone, gone, 1, 1, 0, 4, &p, gone, gone, gone, gone, 0, NULL, NULL) == -1);
  CHECK(yf_images_track_host(gone, gone, 1, 1, 2, 4, &p, gone, gone, gone, gone, 4, NULL, NULL) == -1);
  CHECK(yf_images_track_host(gone, gone, -1, 1, 0, 4, &p, gone, gone, gone, gone, 4, NULL, NULL) == -1);
  CHECK(yf_images_track_host(gone, gone, 1, -1, 0, 4, &p, gone, gone, gone, gone, 4, NULL, NULL) == -1);
  CHECK(yf_images_track_host(gone, gone, 1l << 31, 1l << 31, 0, 4, &p, gone, gone, gone, gone, 4, NULL, NULL) == -1);
  CHECK(yf_images_track_host(gone, gone, 1, 1, 0, 4, &nan_iou, gone, gone, gone, gone, 4, NULL, NULL) == -1);
  CHECK(yf_images_track_host(gone, gone, 1, 1, 0, 4, &no_hits, gone, gone, gone, gone, 4, NULL, NULL) == -1);
  CHECK(yf_images_track_host(gone, gone, 1, 1, 0, 4, &neg_misses, gone, gone, gone, gone, 4, NULL, NULL) == -1);
  CHECK(yf_images_track_host(gone, gone, 1, 1, 0, 4, NULL, gone, gone, gone, gone, 4, NULL, NULL) == -1);
  CHECK(yf_images_track_host(NULL, gone, 1, 1, 0, 4, &p, gone, gone, gone, gone, 4, NULL, NULL) == -1);
  CHECK(yf_images_track_host(gone, gone, 1, 1, 0, 4, &p, (char*)gone + 4, gone, gone, gone, 4, NULL, NULL) == -1);
  CHECK(yf_images_track_host(gone, (char*)gone + 2, 1, 1, 0, 4, &p, gone, gone, gone, gone, 4, NULL, NULL) == -1);
  printf("track: ok, %ld calls\n", g_calls);
  return 0;
}
