/* The host build at h x w (csrc/yf_calib_host.c: yf_calib_host_run_hw, yf_calib_host_compare_hw, yf_calib_host_histogram_hw, with the .yfw
 * parser) under ASan + UBSan, a program of its own: the three functions at 8x8, 16x24, 24x8 and 56x56 with three frames on two threads, every
 * buffer a heap block of exactly its size, so an access past an end -- a stage table whose offsets did not scale with the frame, an h / w
 * swap -- is a report.  Checked besides: the stage table at (56, 56) is yfc_build_stages' field for field, every stage of every size stays
 * inside its arena, the 56x56 functions give the _hw functions' bytes, the histograms conserve their elements, and refused sizes write
 * nothing.  argv[1]: a valid .yfw.  Prints "calibration at h x w: ok ..." and exits 0. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/yf_calib.h"
#include "../../stm32h7-yolo_amd/csrc/yf_calib_arith.h"

enum { N = 3, THREADS = 2, BINS = 64, ENTRIES = 3 };
static uint8_t* yfw;
static size_t yfw_bytes;

static void die(const char* what, const char* text) {
  fprintf(stderr, "%s: %s\n", what, text);
  exit(1);
}

static void* block(size_t bytes, int fill) {
  void* p = malloc(bytes ? bytes : 1);
  if (!p) die("malloc", "out of memory");
  memset(p, fill, bytes);
  return p;
}

/* every stage of the table for (h, w) reads and writes inside the arena of that size, and the logits are its last stage's output */
static void check_table(int h, int w) {
  yfc_stage st[YFC_N_STAGES];
  int32_t ids[YFC_N_RANGES];
  yfc_dims d;
  yfc_build_stages_hw(st, ids, h, w);
  yfc_dims_of(h, w, &d);
  if (d.arena_floats != 800 * (h / 8) * (w / 8) || d.frame_bytes != h * w * 3 || d.logits != (h / 8) * (w / 8) * 18) die("dims", "not the stated sizes");
  if (st[0].h != h || st[0].w != w || st[0].in_off != 0) die("table", "the first stage does not read the frame");
  for (int s = 0; s < YFC_N_STAGES; ++s) {
    const yfc_stage* g = &st[s];
    const long count = (long)g->oh * g->ow * g->cout, in_end = (long)g->in_off + (long)g->h * g->w * g->cin;
    const long out_end = (long)g->out_off + ((long)g->oh * g->ow - 1) * g->out_cstride + g->out_coff + g->cout;
    if (g->oh * g->stride != g->h || g->ow * g->stride != g->w) die("table", "a stride-2 stage does not halve exactly");
    if (g->in_off < 0 || in_end > d.arena_floats || g->out_off < 0 || out_end > d.arena_floats) die("table", "a stage leaves the arena");
    if (g->add_off >= 0 && g->add_off + count > d.arena_floats) die("table", "an ADD operand leaves the arena");
    if (s + 1 < YFC_N_STAGES && g->kind == YFC_CONV && st[s + 1].kind == YFC_CONV && g->out_coff == 0 && g->out_cstride == g->cout &&
        (st[s + 1].h != g->oh || st[s + 1].w != g->ow)) die("table", "a stage does not take its predecessor's shape");
  }
  const yfc_stage* last = &st[YFC_N_STAGES - 1];
  if (last->out_off != d.logits_off || last->oh * last->ow * last->cout != d.logits) die("table", "the logits are not the last stage's output");
}

static void run_size(int h, int w, uint64_t* checksum) {
  yfc_dims d;
  yfc_dims_of(h, w, &d);
  yfc_stage st[YFC_N_STAGES];
  int32_t ids[YFC_N_RANGES];
  yfc_build_stages_hw(st, ids, h, w);
  char err[256] = "";
  int8_t* frames = (int8_t*)block((size_t)N * d.frame_bytes, 0);
  uint32_t x = 12345u + (uint32_t)(h * 1000 + w);
  for (size_t i = 0; i < (size_t)N * d.frame_bytes; ++i) { x = x * 1664525u + 1013904223u; frames[i] = (int8_t)(x >> 24); }
  float* mm = (float*)block(sizeof(float) * 2 * YFC_N_RANGES, 0);
  int32_t* tensors = (int32_t*)block(sizeof(int32_t) * YFC_N_RANGES, 0);
  float* logits = (float*)block(sizeof(float) * (size_t)N * d.logits, 0);
  if (yf_calib_host_run_hw(yfw, yfw_bytes, h, w, frames, N, mm, tensors, logits, THREADS, err, sizeof err) != N) die("yf_calib_host_run_hw", err);
  for (int r = 0; r < YFC_N_RANGES; ++r) if (!(mm[2 * r] <= mm[2 * r + 1]) || tensors[r] != ids[r]) die("ranges", "a range is empty or misnamed");
  for (long i = 0; i < (long)N * d.logits; ++i) { uint32_t b; memcpy(&b, &logits[i], 4); *checksum = *checksum * 1099511628211ull + b; }

  /* histograms on the ranges just observed: every row holds n x the tensor's elements */
  uint64_t* counts = (uint64_t*)block(sizeof(uint64_t) * YFC_N_RANGES * BINS, 0);
  if (yf_calib_host_histogram_hw(yfw, yfw_bytes, h, w, frames, N, mm, BINS, counts, THREADS, err, sizeof err) != N) die("yf_calib_host_histogram_hw", err);
  uint64_t input = 0;
  for (int k = 0; k < BINS; ++k) input += counts[k];
  if (input != (uint64_t)N * (uint64_t)d.frame_bytes) die("conservation", "the input's counts do not sum to n x h x w x 3");
  for (int s = 0; s < YFC_N_STAGES; ++s) {
    const int slots[3] = {st[s].r_conv, st[s].r_leaky, st[s].r_add};
    for (int j = 0; j < 3; ++j) {
      if (slots[j] < 0) continue;
      uint64_t sum = 0;
      for (int k = 0; k < BINS; ++k) sum += counts[(size_t)slots[j] * BINS + k];
      if (sum != (uint64_t)N * (uint64_t)(st[s].oh * st[s].ow * st[s].cout)) die("conservation", "a tensor's counts do not sum to n x its elements");
    }
  }

  /* a comparison of the first stage's, a middle stage's and the last stage's tensor, each int8 block of exactly n x elements bytes */
  const int which[ENTRIES] = {0, 9, YFC_N_STAGES - 1};
  yf_calib_qtensor entries[ENTRIES];
  size_t out_floats = 0;
  for (int e = 0; e < ENTRIES; ++e) {
    const yfc_stage* g = &st[which[e]];
    const size_t el = (size_t)g->oh * g->ow * g->cout;
    memset(&entries[e], 0, sizeof entries[e]);
    entries[e].tensor = g->t_add >= 0 ? g->t_add : g->t_leaky >= 0 ? g->t_leaky : g->t_conv;
    entries[e].scale = 0.05f; entries[e].zero_point = -3;
    entries[e].q = block((size_t)N * el, 1);
    entries[e].frame_stride = el;
    out_floats += (size_t)N * el;
  }
  void* stats = block(YF_CALIB_FRAME_STATS_BYTES * (size_t)N * ENTRIES, 0);
  void* totals = block(YF_CALIB_TOTALS_BYTES * (size_t)ENTRIES, 0);
  float* xs = (float*)block(sizeof(float) * out_floats, 0);
  if (yf_calib_host_compare_hw(yfw, yfw_bytes, h, w, frames, N, entries, ENTRIES, stats, totals, xs, THREADS, err, sizeof err) != N)
    die("yf_calib_host_compare_hw", err);
  /* the last entry is the head: its float tensor is the logits */
  if (memcmp(xs + out_floats - (size_t)N * d.logits, logits, sizeof(float) * (size_t)N * d.logits)) die("compare", "the head's float tensor is not the logits");
  entries[1].frame_stride -= 1;
  if (yf_calib_host_compare_hw(yfw, yfw_bytes, h, w, frames, N, entries, ENTRIES, stats, totals, NULL, THREADS, err, sizeof err) > 0 ||
      !strstr(err, "entry 1: frame_stride is")) die("compare", "a stride below the tensor's elements at this size was not refused");
  entries[1].frame_stride += 1;

  if (h == 56 && w == 56) {                              /* the 56x56 functions forward here: the same bytes */
    float* mm2 = (float*)block(sizeof(float) * 2 * YFC_N_RANGES, 0);
    float* logits2 = (float*)block(sizeof(float) * (size_t)N * YFC_LOGITS, 0);
    uint64_t* counts2 = (uint64_t*)block(sizeof(uint64_t) * YFC_N_RANGES * BINS, 0);
    void* stats2 = block(YF_CALIB_FRAME_STATS_BYTES * (size_t)N * ENTRIES, 0);
    if (yf_calib_host_run(yfw, yfw_bytes, frames, N, mm2, tensors, logits2, THREADS, err, sizeof err) != N) die("yf_calib_host_run", err);
    if (yf_calib_host_histogram(yfw, yfw_bytes, frames, N, mm, BINS, counts2, THREADS, err, sizeof err) != N) die("yf_calib_host_histogram", err);
    if (yf_calib_host_compare(yfw, yfw_bytes, frames, N, entries, ENTRIES, stats2, NULL, NULL, THREADS, err, sizeof err) != N) die("yf_calib_host_compare", err);
    if (memcmp(mm, mm2, sizeof(float) * 2 * YFC_N_RANGES) || memcmp(logits, logits2, sizeof(float) * (size_t)N * YFC_LOGITS) ||
        memcmp(counts, counts2, sizeof(uint64_t) * YFC_N_RANGES * BINS) || memcmp(stats, stats2, YF_CALIB_FRAME_STATS_BYTES * (size_t)N * ENTRIES))
      die("56x56", "the 56x56 functions and the _hw functions at (56, 56) differ");
    free(mm2); free(logits2); free(counts2); free(stats2);
  }
  for (int e = 0; e < ENTRIES; ++e) free((void*)entries[e].q);
  free(stats); free(totals); free(xs); free(counts); free(logits); free(tensors); free(mm); free(frames);
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s model.yfw\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  fseek(f, 0, SEEK_END);
  const long size = ftell(f);
  fseek(f, 0, SEEK_SET);
  yfw = (uint8_t*)malloc((size_t)size);
  if (!yfw || fread(yfw, 1, (size_t)size, f) != (size_t)size) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  fclose(f);
  yfw_bytes = (size_t)size;

  /* the table at (56, 56) is the one yfc_build_stages gives, field for field; every admitted size stays inside its arena */
  yfc_stage a[YFC_N_STAGES], b[YFC_N_STAGES];
  int32_t ia[YFC_N_RANGES], ib[YFC_N_RANGES];
  memset(a, 0, sizeof a); memset(b, 0, sizeof b);
  yfc_build_stages(a, ia);
  yfc_build_stages_hw(b, ib, 56, 56);
  if (memcmp(a, b, sizeof a) || memcmp(ia, ib, sizeof ia)) die("table", "yfc_build_stages is not the builder at (56, 56)");
  if (a[0].out_off != 9408 || a[4].out_cstride != 36 || a[25].out_off != YFC_LOGITS_OFF || a[9].add_off != 10584) die("table", "the 56x56 table moved");
  int tables = 0;
  for (int h = 8; h <= YFC_MAX_SIDE; h += 8)
    for (int w = 8; w <= YFC_MAX_SIDE; w += 8, ++tables) check_table(h, w);

  const int sizes[4][2] = {{8, 8}, {16, 24}, {24, 8}, {56, 56}};
  uint64_t checksum = 14695981039346656037ull;
  for (int i = 0; i < 4; ++i) run_size(sizes[i][0], sizes[i][1], &checksum);

  /* refused sizes: named, nothing written */
  const int bad[8][2] = {{0, 8}, {8, 0}, {4, 8}, {60, 56}, {56, 60}, {168, 160}, {-8, 8}, {8, -56}};
  int8_t* frames = (int8_t*)block(YFC_FRAME_BYTES, 0);
  unsigned char* out = (unsigned char*)block(4096, 0x5a);
  long refused = 0;
  for (int i = 0; i < 8; ++i) {
    char err[256] = "", want[96];
    snprintf(want, sizeof want, "h = %d, w = %d, expected multiples of 8 from 8 to 160", bad[i][0], bad[i][1]);
    if (yf_calib_host_run_hw(yfw, yfw_bytes, bad[i][0], bad[i][1], frames, 1, (float*)out, (int32_t*)(out + 1024), (float*)(out + 2048), 2, err, sizeof err) > 0 ||
        !strstr(err, want)) die("a refused size", err);
    if (yf_calib_host_histogram_hw(yfw, yfw_bytes, bad[i][0], bad[i][1], frames, 1, (const float*)out, 16, (uint64_t*)(out + 1024), 2, err, sizeof err) > 0 ||
        !strstr(err, want)) die("a refused size", err);
    yf_calib_qtensor e;
    memset(&e, 0, sizeof e);
    e.tensor = 100; e.scale = 1.0f; e.q = frames; e.frame_stride = 882;
    if (yf_calib_host_compare_hw(yfw, yfw_bytes, bad[i][0], bad[i][1], frames, 1, &e, 1, out, out + 1024, NULL, 2, err, sizeof err) > 0 ||
        !strstr(err, want)) die("a refused size", err);
    refused += 3;
  }
  /* ... and n < 1 at an admitted size */
  const long none[2] = {0, -3};
  for (int i = 0; i < 2; ++i) {
    char err[256] = "", want[64];
    yf_calib_qtensor e;
    memset(&e, 0, sizeof e);
    e.tensor = 100; e.scale = 1.0f; e.q = frames; e.frame_stride = 18;
    snprintf(want, sizeof want, "n = %ld is below 1", none[i]);
    if (yf_calib_host_run_hw(yfw, yfw_bytes, 8, 8, frames, none[i], (float*)out, (int32_t*)(out + 1024), (float*)(out + 2048), 2, err, sizeof err) > 0 ||
        !strstr(err, want)) die("n < 1", err);
    snprintf(want, sizeof want, "n is %ld, expected at least 1", none[i]);
    if (yf_calib_host_compare_hw(yfw, yfw_bytes, 8, 8, frames, none[i], &e, 1, out, out + 1024, (float*)(out + 2048), 2, err, sizeof err) > 0 ||
        !strstr(err, want)) die("n < 1", err);
    float axes[2 * YFC_N_RANGES];
    for (int r = 0; r < YFC_N_RANGES; ++r) { axes[2 * r] = -1.0f; axes[2 * r + 1] = 1.0f; }
    if (yf_calib_host_histogram_hw(yfw, yfw_bytes, 8, 8, frames, none[i], axes, 4, (uint64_t*)out, 2, err, sizeof err) > 0 || !strstr(err, want)) die("n < 1", err);
    refused += 3;
  }
  for (int i = 0; i < 4096; ++i) if (out[i] != 0x5a) die("refusals", "a refused call wrote to its outputs");
  free(out); free(frames); free(yfw);
  printf("calibration at h x w: ok (%d stage tables inside their arenas, 4 sizes run, %ld refusals, logits checksum %016llx)\n", tables, refused,
         (unsigned long long)checksum);
  return 0;
}
