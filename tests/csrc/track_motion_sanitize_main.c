/* The host build of the tracker with a motion model (csrc/yf_images_motion.h through csrc/yf_images_host.c) under ASan + UBSan: a program
 * of its own, compiled together with yf_images_host.c by tests/test_track_motion_sanitize.py.  The states, the record rows, the counts and
 * every output array are allocations of exactly their extent, so a load or a store one byte before or past one of them is a report, and
 * signed overflow in a counter, an edge difference or the filter's 64-bit chain is one too -- which is what proves the clamp of
 * yfi_motion_sat: with pos and vel at the int64 extremes nothing overflows.  Inputs: states of random bytes, states whose counters sit at
 * INT32_MAX and INT32_MIN, whose pos and vel sit at INT64_MIN, INT64_MAX and around the clamp and whose `issued` is about to wrap, full
 * tables; records with INT32_MIN / INT32_MAX edges, empty and inverted boxes and random bytes; counts of every kind; cap 1, 64, 70 and
 * 1200; out_cap 1, 3 and 64; both layouts; gains at and between their bounds, smooth 0 and 1; with and without a status array; and calls
 * the check refuses, which must touch nothing (their arrays have been freed). */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/yf_images.h"

long yf_images_track_motion_host(const void* dets, const void* counts, long streams, long steps, int layout, int cap,
                                 const yf_track_motion_params* params, void* state, void* out, void* info, void* out_counts, int out_cap,
                                 int32_t* status, void* stream);

static uint32_t g_seed = 6161u;
static uint32_t rnd(void) { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

#define CHECK(c) do { if (!(c)) { printf("motion: FAILED %s (line %d)\n", #c, __LINE__); exit(1); } } while (0)
#define LIMIT (1ll << 40)

static void* exact(size_t bytes, int random) {
  uint8_t* p = malloc(bytes ? bytes : 1);
  CHECK(p);
  for (size_t i = 0; i < bytes; ++i) p[i] = random ? (uint8_t)rnd() : 0xA5;
  return p;
}

static const int32_t EDGE[8] = {INT32_MIN, INT32_MIN + 1, -1, 0, 1, 7, INT32_MAX - 1, INT32_MAX};
static const int64_t WIDE[10] = {INT64_MIN, INT64_MIN + 1, -LIMIT - 1, -LIMIT, -1, 0, 256 * 20, LIMIT, LIMIT + 1, INT64_MAX};

/* kind 0: random bytes; 1: edges drawn from EDGE (extremes, empty, inverted); 2: small boxes near the origin, which meet each other */
static void fill_records(yf_det* d, size_t count, int kind) {
  for (size_t i = 0; i < count; ++i) {
    if (kind == 0) continue;                                        /* `exact` made them random */
    if (kind == 1) { d[i].x1 = EDGE[rnd() % 8]; d[i].y1 = EDGE[rnd() % 8]; d[i].x2 = EDGE[rnd() % 8]; d[i].y2 = EDGE[rnd() % 8]; }
    else { d[i].x1 = (int32_t)(rnd() % 40u); d[i].y1 = (int32_t)(rnd() % 40u); d[i].x2 = d[i].x1 + (int32_t)(rnd() % 12u) - 1; d[i].y2 = d[i].y1 + (int32_t)(rnd() % 12u) - 1; }
  }
}

/* kind 0: zero; 1: random bytes; 2: random bytes with every id non-zero (a full table); 3: counters at the int32 extremes, pos and vel
 * from WIDE, issued about to wrap; 4: a full table of small boxes near the origin with pos and vel from WIDE on some edges */
static void fill_states(yf_track_motion_state* st, long streams, int kind) {
  for (long s = 0; s < streams; ++s) {
    if (kind == 0) memset(&st[s], 0, sizeof st[s]);
    if (kind == 2) for (int k = 0; k < YF_TRACK_SLOTS; ++k) st[s].slot[k].base.id |= 1u;
    if (kind == 3 || kind == 4) {
      st[s].issued = 0xFFFFFFFFu - (uint32_t)(rnd() % 3u);
      for (int k = 0; k < YF_TRACK_SLOTS; ++k) {
        yf_track_motion* t = &st[s].slot[k];
        t->base.id = kind == 3 && k % 5 == 0 ? 0u : (rnd() | 1u);
        if (kind == 3) {
          t->base.hits = k % 2 ? INT32_MAX : INT32_MIN; t->base.misses = k % 3 ? INT32_MAX : INT32_MIN; t->base.age = k % 4 ? INT32_MAX : -1;
        } else {
          t->base.hits = 3; t->base.misses = (int32_t)(rnd() % 3u); t->base.age = 7;
        }
        for (int e = 0; e < 4; ++e) {
          const int64_t near = 256 * (int64_t)(rnd() % 40u + (e >= 2 ? 10u : 0u));
          t->pos[e] = kind == 4 && rnd() % 4u ? near : WIDE[rnd() % 10];
          t->vel[e] = kind == 4 && rnd() % 4u ? (int64_t)(rnd() % 1024u) - 512 : WIDE[rnd() % 10];
        }
      }
    }
  }
}

static long g_calls = 0;

static void run(long streams, long steps, int layout, int cap, int out_cap, yf_track_motion_params p, int state_kind, int rec_kind, int with_status) {
  const long n = streams * steps;
  yf_track_motion_state* st = exact(sizeof(yf_track_motion_state) * (size_t)streams, 1);
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
  CHECK(yf_images_track_motion_host(dets, counts, streams, steps, layout, cap, &p, st, out, info, oc, out_cap, status, NULL) == n);
  for (long f = 0; f < n; ++f) {
    CHECK(oc[f] >= 0 && oc[f] <= YF_TRACK_SLOTS);
    if (status) CHECK((status[f] & ~3) == 0 && ((status[f] & 1) != 0) == (counts[f] > (cap < 64 ? cap : 64)));
    for (int r = 0; r < out_cap; ++r) {
      const yf_det* o = &out[f * out_cap + r];
      const yf_track_info* i = &info[f * out_cap + r];
      if (r < oc[f]) {
        CHECK(o->frame == (int32_t)f && i->id != 0 && i->hits >= p.base.min_hits);
        CHECK(r == 0 || i[-1].id <= i->id);                         /* ascending id */
      } else {
        CHECK((uint32_t)o->frame == 0xA5A5A5A5u && i->id == 0xA5A5A5A5u);           /* not touched */
      }
    }
  }
  /* what a step wrote lies within the clamp: every slot that is occupied after at least one step */
  for (long s = 0; s < streams; ++s)
    for (int k = 0; k < YF_TRACK_SLOTS; ++k) {
      const yf_track_motion* t = &st[s].slot[k];
      if (steps > 0 && t->base.id != 0)
        for (int e = 0; e < 4; ++e) CHECK(t->pos[e] >= -LIMIT && t->pos[e] <= LIMIT && t->vel[e] >= -LIMIT && t->vel[e] <= LIMIT);
    }
  free(st); free(dets); free(counts); free(out); free(info); free(oc); free(status);
  ++g_calls;
}

int main(void) {
  const yf_track_motion_params params[6] = {{{0.3, 1, 5}, 192, 128, 256, 0}, {{0.0, 1, 0}, 256, 256, 256, 1}, {{1.0, 3, 2}, 0, 0, 0, 0},
                                            {{-1.0, INT32_MAX, INT32_MAX}, 256, 0, 13, 1}, {{INFINITY, 1, 1}, 1, 255, 255, 1},
                                            {{0.5, 2, INT32_MAX}, 77, 201, 128, 0}};
  const int caps[4] = {1, 64, 70, 1200}, out_caps[3] = {1, 3, 64};
  for (int sk = 0; sk < 5; ++sk)
    for (int rk = 0; rk < 3; ++rk)
      for (int c = 0; c < 4; ++c)
        for (int pi = 0; pi < 6; ++pi) {
          const int layout = (sk + rk + c + pi) & 1;
          run(1 + (pi % 3), 1 + (c + rk) % 4, layout, caps[c], out_caps[(sk + pi) % 3], params[pi], sk, rk, (c + pi) & 1);
        }
  run(5, 9, YF_TRACK_TIME_MAJOR, 70, 64, params[0], 0, 2, 1);      /* a longer clip from the empty state: tracks live, coast and die */
  run(5, 9, YF_TRACK_STREAM_MAJOR, 70, 2, params[1], 0, 2, 1);
  run(2, 9, YF_TRACK_TIME_MAJOR, 64, 64, params[1], 4, 2, 1);      /* full tables whose boxes the records meet, kept for ever: matches at the extremes */
  run(2, 9, YF_TRACK_STREAM_MAJOR, 64, 64, params[3], 4, 2, 0);
  run(0, 4, YF_TRACK_TIME_MAJOR, 8, 4, params[0], 0, 2, 1);        /* empty batches: nothing is read or written */
  run(3, 0, YF_TRACK_STREAM_MAJOR, 8, 4, params[0], 1, 2, 0);

  /* refused calls: the arrays are freed memory */
  void* gone = exact(64, 0);
  free(gone);
  yf_track_motion_params p = params[0], nan_iou = p, no_hits = p, neg_misses = p, alpha = p, beta = p, damp = p, smooth = p, alpha_neg = p;
  nan_iou.base.match_iou = NAN; no_hits.base.min_hits = 0; neg_misses.base.max_misses = -1;
  alpha.alpha = 257; alpha_neg.alpha = -1; beta.beta = INT32_MIN; damp.damp = INT32_MAX; smooth.smooth = 2;
  const yf_track_motion_params* bad[8] = {&nan_iou, &no_hits, &neg_misses, &alpha, &alpha_neg, &beta, &damp, &smooth};
  for (int k = 0; k < 8; ++k) CHECK(yf_images_track_motion_host(gone, gone, 1, 1, 0, 4, bad[k], gone, gone, gone, gone, 4, NULL, NULL) == -1);
  CHECK(yf_images_track_motion_host(gone, gone, 1, 1, 0, 0, &p, gone, gone, gone, gone, 4, NULL, NULL) == -1);
  CHECK(yf_images_track_motion_host(gone, gone, 1, 1, 0, 1201, &p, gone, gone, gone, gone, 4, NULL, NULL) == -1);
  CHECK(yf_images_track_motion_host(gone, gone, 1, 1, 0, 4, &p, gone, gone, gone, gone, 0, NULL, NULL) == -1);
  CHECK(yf_images_track_motion_host(gone, gone, 1, 1, 2, 4, &p, gone, gone, gone, gone, 4, NULL, NULL) == -1);
  CHECK(yf_images_track_motion_host(gone, gone, -1, 1, 0, 4, &p, gone, gone, gone, gone, 4, NULL, NULL) == -1);
  CHECK(yf_images_track_motion_host(gone, gone, 1, -1, 0, 4, &p, gone, gone, gone, gone, 4, NULL, NULL) == -1);
  CHECK(yf_images_track_motion_host(gone, gone, 1l << 31, 1l << 31, 0, 4, &p, gone, gone, gone, gone, 4, NULL, NULL) == -1);
  CHECK(yf_images_track_motion_host(gone, gone, 1, 1, 0, 4, NULL, gone, gone, gone, gone, 4, NULL, NULL) == -1);
  CHECK(yf_images_track_motion_host(NULL, gone, 1, 1, 0, 4, &p, gone, gone, gone, gone, 4, NULL, NULL) == -1);
  CHECK(yf_images_track_motion_host(gone, gone, 1, 1, 0, 4, &p, (char*)gone + 4, gone, gone, gone, 4, NULL, NULL) == -1);
  CHECK(yf_images_track_motion_host(gone, (char*)gone + 2, 1, 1, 0, 4, &p, gone, gone, gone, gone, 4, NULL, NULL) == -1);
  printf("motion: ok, %ld calls\n", g_calls);
  return 0;
}
