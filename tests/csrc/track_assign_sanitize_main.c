/* The host build of the optimal assignment (csrc/yf_images_assign.h through csrc/yf_images_host.c) under ASan + UBSan: a program of its
 * own, compiled together with yf_images_host.c by tests/test_track_assign_sanitize.py.  The states, the record rows, the counts, the
 * tables of weights and every output array are allocations of exactly their extent, so a load or a store one byte before or past one of
 * them is a report, and signed overflow in a potential, a reduced cost or the filter's 64-bit chain is one too -- the header's bound on
 * u, v and minv under UBSan's signed-overflow check.  Inputs: tables of weights all at the maximum 2^30 + 1, all at the minimum 1, the
 * staircase of both, random ones of few levels, with the potentials' extremes asserted through the result's optimality on the uniform
 * ones; through the entry, the 64 x 64 scenes of all-maximum weight (identical boxes, IoU 1) and all-minimum weight (huge boxes that
 * share one pixel, IoU 2^-41 at match_iou 0), states of random bytes, counters at the int32 extremes, pos and vel at the int64 extremes,
 * full tables, records with INT32_MIN / INT32_MAX edges, empty and inverted boxes; counts of every kind; cap 1, 64, 70 and 1200; both
 * layouts; both values of assign; and calls the check refuses, which must touch nothing (their arrays have been freed). */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/yf_images.h"

long yf_images_track_motion_assign_host(const void* dets, const void* counts, long streams, long steps, int layout, int cap,
                                        const yf_track_motion_params* params, int assign, void* state, void* out, void* info,
                                        void* out_counts, int out_cap, int32_t* status, void* stream);
int64_t yfi_assign_solve_host(const int32_t* weights, int m, int* slot_det, int* det_slot);

static uint32_t g_seed = 7171u;
static uint32_t rnd(void) { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

#define CHECK(c) do { if (!(c)) { printf("assign: FAILED %s (line %d)\n", #c, __LINE__); exit(1); } } while (0)
#define LIMIT (1ll << 40)
#define TOP ((1 << 30) + 1)

static void* exact(size_t bytes, int random) {
  uint8_t* p = malloc(bytes ? bytes : 1);
  CHECK(p);
  for (size_t i = 0; i < bytes; ++i) p[i] = random ? (uint8_t)rnd() : 0xA5;
  return p;
}

static long g_calls = 0;

/* the procedure on a table of m rows: kind 0 all TOP, 1 all 1, 2 the staircase (TOP for j <= i, 1 beyond), 3 the staircase with its rows
 * in descending order, 4 random of the levels {0, 1, TOP - 1, TOP}, 5 random over the whole range, 6 all 0 */
static void solve(int m, int kind) {
  int32_t* w = exact(4 * (size_t)m * 64, 0);
  int* slot_det = exact(4 * 64, 0);
  int* det_slot = exact(4 * (size_t)m, 0);
  const int32_t levels[4] = {0, 1, TOP - 1, TOP};
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < 64; ++j) {
      const int row = kind == 3 ? m - 1 - i : i;
      w[i * 64 + j] = kind == 0 ? TOP : kind == 1 ? 1 : kind == 2 || kind == 3 ? (j <= row ? TOP : 1) : kind == 4 ? levels[rnd() % 4u]
                      : kind == 5 ? (int32_t)(rnd() % (uint32_t)TOP) + (int32_t)(rnd() % 2u) : 0;
    }
  const int64_t total = yfi_assign_solve_host(w, m, slot_det, det_slot);
  int64_t sum = 0;
  int pairs = 0;
  for (int i = 0; i < m; ++i) {
    const int j = det_slot[i];
    CHECK(j >= -1 && j < 64);
    if (j < 0) continue;
    CHECK(slot_det[j] == i && w[i * 64 + j] > 0);
    sum += w[i * 64 + j];
    ++pairs;
  }
  for (int j = 0; j < 64; ++j) CHECK(slot_det[j] >= -1 && slot_det[j] < m && (slot_det[j] < 0 || det_slot[slot_det[j]] == j));
  CHECK(sum == total);
  if (kind == 0) CHECK(pairs == m && total == (int64_t)m * TOP);
  if (kind == 1) CHECK(pairs == m && total == m);
  if (kind == 2 || kind == 3) CHECK(pairs == m && total == (int64_t)m * TOP);       /* the diagonal */
  if (kind == 6) CHECK(pairs == 0 && total == 0);
  free(w); free(slot_det); free(det_slot);
  ++g_calls;
}

static const int32_t EDGE[8] = {INT32_MIN, INT32_MIN + 1, -1, 0, 1, 7, INT32_MAX - 1, INT32_MAX};
static const int64_t WIDE[10] = {INT64_MIN, INT64_MIN + 1, -LIMIT - 1, -LIMIT, -1, 0, 256 * 20, LIMIT, LIMIT + 1, INT64_MAX};

/* kind 0: random bytes; 1: edges drawn from EDGE (extremes, empty, inverted); 2: small boxes near the origin, which meet each other; 3:
 * all the box (12, 10, 51, 59); 4: all the box that shares the pixel (2^20 - 1, 2^20 - 1) with the slots of state kind 6 */
static void fill_records(yf_det* d, size_t count, int kind) {
  for (size_t i = 0; i < count; ++i) {
    if (kind == 0) continue;                                        /* `exact` made them random */
    if (kind == 1) { d[i].x1 = EDGE[rnd() % 8]; d[i].y1 = EDGE[rnd() % 8]; d[i].x2 = EDGE[rnd() % 8]; d[i].y2 = EDGE[rnd() % 8]; }
    else if (kind == 2) { d[i].x1 = (int32_t)(rnd() % 40u); d[i].y1 = (int32_t)(rnd() % 40u); d[i].x2 = d[i].x1 + (int32_t)(rnd() % 12u) - 1; d[i].y2 = d[i].y1 + (int32_t)(rnd() % 12u) - 1; }
    else if (kind == 3) { d[i].x1 = 12; d[i].y1 = 10; d[i].x2 = 51; d[i].y2 = 59; }
    else { d[i].x1 = (1 << 20) - 1; d[i].y1 = (1 << 20) - 1; d[i].x2 = 1 << 21; d[i].y2 = 1 << 21; }
  }
}

/* kind 0: zero; 1: random bytes; 2: random bytes with every id non-zero (a full table); 3: counters at the int32 extremes, pos and vel
 * from WIDE, issued about to wrap; 4: a full table of small boxes near the origin with pos and vel from WIDE on some edges; 5: a full
 * table at rest, every slot the box (12, 10, 51, 59): IoU 1 with records of kind 3; 6: a full table at rest, every slot the box
 * (0, 0, 2^20 - 1, 2^20 - 1): one shared pixel with records of kind 4 */
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
    if (kind == 5 || kind == 6) {
      memset(&st[s], 0, sizeof st[s]);
      st[s].issued = 64;
      for (int k = 0; k < YF_TRACK_SLOTS; ++k) {
        yf_track_motion* t = &st[s].slot[k];
        const int32_t box[4] = {kind == 5 ? 12 : 0, kind == 5 ? 10 : 0, kind == 5 ? 51 : (1 << 20) - 1, kind == 5 ? 59 : (1 << 20) - 1};
        t->base.id = (uint32_t)k + 1u; t->base.hits = 2; t->base.age = 2;
        t->base.det.x1 = box[0]; t->base.det.y1 = box[1]; t->base.det.x2 = box[2]; t->base.det.y2 = box[3];
        for (int e = 0; e < 4; ++e) t->pos[e] = 256 * (int64_t)box[e];
      }
    }
  }
}

static void run(long streams, long steps, int layout, int cap, int out_cap, yf_track_motion_params p, int assign, int state_kind, int rec_kind,
                int with_status, int full_counts) {
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
  for (long f = 0; f < n; ++f) counts[f] = full_counts ? cap : rnd() % 3u == 0 ? special[rnd() % 8] : (int32_t)(rnd() % (uint32_t)(cap + 1));
  CHECK(yf_images_track_motion_assign_host(dets, counts, streams, steps, layout, cap, &p, assign, st, out, info, oc, out_cap, status, NULL) == n);
  for (long f = 0; f < n; ++f) {
    CHECK(oc[f] >= 0 && oc[f] <= YF_TRACK_SLOTS);
    if (status) CHECK((status[f] & ~3) == 0 && ((status[f] & 1) != 0) == (counts[f] > (cap < 64 ? cap : 64)));
    if (full_counts && status) CHECK(status[f] == 0 && oc[f] == 64);                  /* the dense scenes: all 64 matched, nothing born */
    for (int r = 0; r < out_cap; ++r) {
      const yf_det* o = &out[f * out_cap + r];
      const yf_track_info* i = &info[f * out_cap + r];
      if (r < oc[f]) {
        CHECK(o->frame == (int32_t)f && i->id != 0 && i->hits >= p.base.min_hits);
        CHECK(r == 0 || i[-1].id <= i->id);                         /* ascending id */
        if (full_counts) CHECK(i->misses == 0 && i->id == (uint32_t)r + 1u);
      } else {
        CHECK((uint32_t)o->frame == 0xA5A5A5A5u && i->id == 0xA5A5A5A5u);           /* not touched */
      }
    }
  }
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
  const int rows[8] = {0, 1, 2, 3, 7, 33, 63, 64};
  for (int kind = 0; kind < 7; ++kind)
    for (int r = 0; r < 8; ++r) solve(rows[r], kind);
  for (int k = 0; k < 40; ++k) solve((int)(rnd() % 65u), 4 + k % 2);

  const yf_track_motion_params params[6] = {{{0.3, 1, 5}, 192, 128, 256, 0}, {{0.0, 1, 0}, 256, 256, 256, 1}, {{1.0, 3, 2}, 0, 0, 0, 0},
                                            {{-1.0, INT32_MAX, INT32_MAX}, 256, 0, 13, 1}, {{INFINITY, 1, 1}, 1, 255, 255, 1},
                                            {{0.5, 2, INT32_MAX}, 77, 201, 128, 0}};
  const int caps[4] = {1, 64, 70, 1200}, out_caps[3] = {1, 3, 64};
  for (int sk = 0; sk < 5; ++sk)
    for (int rk = 0; rk < 3; ++rk)
      for (int c = 0; c < 4; ++c)
        for (int pi = 0; pi < 6; ++pi) {
          const int layout = (sk + rk + c + pi) & 1;
          run(1 + (pi % 3), 1 + (c + rk) % 4, layout, caps[c], out_caps[(sk + pi) % 3], params[pi], (sk + c) % 3 != 0, sk, rk, (c + pi) & 1, 0);
        }
  run(5, 9, YF_TRACK_TIME_MAJOR, 70, 64, params[0], 1, 0, 2, 1, 0);   /* a longer clip from the empty state: tracks live, coast and die */
  run(5, 9, YF_TRACK_STREAM_MAJOR, 70, 2, params[1], 1, 0, 2, 1, 0);
  run(2, 9, YF_TRACK_TIME_MAJOR, 64, 64, params[1], 1, 4, 2, 1, 0);   /* full tables whose boxes the records meet, kept for ever */
  run(2, 9, YF_TRACK_STREAM_MAJOR, 64, 64, params[3], 1, 4, 2, 0, 0);
  /* the dense scenes, 64 x 64: all-maximum weight (IoU 1; gains (256, 0): the tracks stay where they are) and all-minimum weight (one
   * shared pixel of 2^40 + 2^42 or so: weight 1 at match_iou 0; alpha 0: the tracks stay), both layouts, three steps each */
  const yf_track_motion_params rest = {{0.3, 1, 5}, 256, 0, 256, 0}, still = {{0.0, 1, 5}, 0, 0, 256, 0};
  for (int layout = 0; layout < 2; ++layout) {
    run(2, 3, layout, 64, 64, rest, 1, 5, 3, 1, 1);
    run(2, 3, layout, 64, 64, still, 1, 6, 4, 1, 1);
    run(1, 2, layout, 64, 64, rest, 0, 5, 3, 1, 1);
  }
  run(0, 4, YF_TRACK_TIME_MAJOR, 8, 4, params[0], 1, 0, 2, 1, 0);     /* empty batches: nothing is read or written */
  run(3, 0, YF_TRACK_STREAM_MAJOR, 8, 4, params[0], 1, 1, 2, 0, 0);

  /* refused calls: the arrays are freed memory */
  void* gone = exact(64, 0);
  free(gone);
  yf_track_motion_params p = params[0], nan_iou = p, alpha = p, smooth = p;
  nan_iou.base.match_iou = NAN; alpha.alpha = 257; smooth.smooth = 2;
  const int bad_assign[5] = {-1, 2, 3, INT32_MIN, INT32_MAX};
  for (int k = 0; k < 5; ++k) CHECK(yf_images_track_motion_assign_host(gone, gone, 1, 1, 0, 4, &p, bad_assign[k], gone, gone, gone, gone, 4, NULL, NULL) == -1);
  CHECK(yf_images_track_motion_assign_host(gone, gone, 0, 0, 0, 4, &p, 2, gone, gone, gone, gone, 4, NULL, NULL) == -1);
  for (int a = 0; a < 2; ++a) {
    CHECK(yf_images_track_motion_assign_host(gone, gone, 1, 1, 0, 4, &nan_iou, a, gone, gone, gone, gone, 4, NULL, NULL) == -1);
    CHECK(yf_images_track_motion_assign_host(gone, gone, 1, 1, 0, 4, &alpha, a, gone, gone, gone, gone, 4, NULL, NULL) == -1);
    CHECK(yf_images_track_motion_assign_host(gone, gone, 1, 1, 0, 4, &smooth, a, gone, gone, gone, gone, 4, NULL, NULL) == -1);
    CHECK(yf_images_track_motion_assign_host(gone, gone, 1, 1, 0, 0, &p, a, gone, gone, gone, gone, 4, NULL, NULL) == -1);
    CHECK(yf_images_track_motion_assign_host(gone, gone, 1, 1, 0, 4, &p, a, gone, gone, gone, gone, 0, NULL, NULL) == -1);
    CHECK(yf_images_track_motion_assign_host(gone, gone, 1, 1, 2, 4, &p, a, gone, gone, gone, gone, 4, NULL, NULL) == -1);
    CHECK(yf_images_track_motion_assign_host(gone, gone, -1, 1, 0, 4, &p, a, gone, gone, gone, gone, 4, NULL, NULL) == -1);
    CHECK(yf_images_track_motion_assign_host(gone, gone, 1, 1, 0, 4, NULL, a, gone, gone, gone, gone, 4, NULL, NULL) == -1);
    CHECK(yf_images_track_motion_assign_host(NULL, gone, 1, 1, 0, 4, &p, a, gone, gone, gone, gone, 4, NULL, NULL) == -1);
    CHECK(yf_images_track_motion_assign_host(gone, gone, 1, 1, 0, 4, &p, a, (char*)gone + 4, gone, gone, gone, 4, NULL, NULL) == -1);
  }
  printf("assign: ok, %ld calls\n", g_calls);
  return 0;
}
