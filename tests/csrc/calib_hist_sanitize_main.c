/* The host build of the histograms (csrc/yf_calib_host.c with csrc/yf_calib_hist.h and the .yfw parser) under ASan + UBSan, a program of its
 * own: two frames at 1 and 4096 bins, axes far narrower than the data (every value in an end bin), accumulation, every refused argument,
 * and the placement of the kernel's tables (yfc_hist_windows), whose result is checked against the stage table: no window holds a float its
 * step touches or a later step reads before it is rewritten.  Every buffer is a heap
 * block of exactly its size, so an access past an end is a report.  argv[1]: a valid .yfw.  Prints "histograms: ok ..." and exits 0. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/yf_calib.h"
#include "../../stm32h7-yolo_amd/csrc/yf_calib_hist.h"

enum { N = 2 };
static uint8_t* yfw;
static size_t yfw_bytes;
static int8_t* frames;
static long refused;

static void die(const char* what, const char* text) {
  fprintf(stderr, "%s: %s\n", what, text);
  exit(1);
}

/* one call on fresh exact-size blocks; returns the counts (the caller frees them) */
static uint64_t* histogram(const float* minmax, int bins, int threads, int check_input) {
  float* mm = (float*)malloc(sizeof(float) * 2 * YFC_N_RANGES);
  uint64_t* counts = (uint64_t*)calloc((size_t)YFC_N_RANGES * (size_t)bins, sizeof(uint64_t));
  char err[256] = "";
  if (!mm || !counts) die("histogram", "out of memory");
  memcpy(mm, minmax, sizeof(float) * 2 * YFC_N_RANGES);
  if (yf_calib_host_histogram(yfw, yfw_bytes, frames, N, mm, bins, counts, threads, err, sizeof err) != N) die("a valid call was refused", err);
  free(mm);
  if (check_input) {
    uint64_t input = 0;
    for (int k = 0; k < bins; ++k) input += counts[k];
    if (input != (uint64_t)N * YFC_FRAME_BYTES) die("conservation", "the input's counts do not sum to n x 9408");
  }
  return counts;
}

static void must_refuse(const int8_t* f, long n, const float* minmax, int bins, uint64_t* counts, const char* needle) {
  char err[256] = "";
  if (yf_calib_host_histogram(yfw, yfw_bytes, f, n, minmax, bins, counts, 2, err, sizeof err) > 0 || !strstr(err, needle)) {
    fprintf(stderr, "not refused as expected (text: '%s', wanted '%s')\n", err, needle);
    exit(1);
  }
  ++refused;
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
  frames = (int8_t*)malloc((size_t)N * YFC_FRAME_BYTES);
  if (!frames) return 2;
  uint32_t x = 12345;
  for (size_t i = 0; i < (size_t)N * YFC_FRAME_BYTES; ++i) { x = x * 1664525u + 1013904223u; frames[i] = (int8_t)(x >> 24); }

  /* the ranges of these frames, then axes of them, of a sliver inside them, and of one point */
  float own[2 * YFC_N_RANGES], narrow[2 * YFC_N_RANGES], point[2 * YFC_N_RANGES];
  int32_t ids[YFC_N_RANGES];
  char err[256] = "";
  if (yf_calib_host_run(yfw, yfw_bytes, frames, N, own, ids, NULL, 2, err, sizeof err) != N) die("yf_calib_host_run", err);
  for (int r = 0; r < YFC_N_RANGES; ++r) {
    const float mid = own[2 * r] + (own[2 * r + 1] - own[2 * r]) * 0.5f;
    narrow[2 * r] = mid; narrow[2 * r + 1] = mid + (own[2 * r + 1] - own[2 * r]) * 1e-6f;
    point[2 * r] = point[2 * r + 1] = mid;
  }
  const int bin_counts[2] = {1, YFC_HIST_MAX_BINS};
  for (int b = 0; b < 2; ++b) {
    const int bins = bin_counts[b];
    uint64_t* wide = histogram(own, bins, 1, 1);
    uint64_t* thin = histogram(narrow, bins, 2, 1);
    uint64_t* dot = histogram(point, bins, 2, 1);
    for (int r = 0; r < YFC_N_RANGES; ++r) {
      const uint64_t* w = wide + (size_t)r * bins;
      const uint64_t* t = thin + (size_t)r * bins;
      const uint64_t* d = dot + (size_t)r * bins;
      uint64_t sw = 0, st = 0, sd = 0, inner = 0;
      for (int k = 0; k < bins; ++k) { sw += w[k]; st += t[k]; sd += d[k]; if (k > 0 && k < bins - 1) inner += t[k]; }
      if (sw != st || sw != sd || sw == 0) die("conservation", "the three axes count different totals");
      if (bins > 1 && (w[0] == 0 || w[bins - 1] == 0)) die("own axes", "an end bin is empty: the minimum and the maximum lie there");
      if (d[0] != sd) die("max == min", "a value left bin 0");
      if (bins > 1 && inner > sw / 100) die("narrow axes", "more than a hundredth of the values inside a millionth of the range");
    }
    /* accumulation: a second call into the same block doubles it */
    float* mm = (float*)malloc(sizeof own);
    if (!mm) return 2;
    memcpy(mm, own, sizeof own);
    uint64_t* twice = histogram(own, bins, 2, 1);
    if (yf_calib_host_histogram(yfw, yfw_bytes, frames, N, mm, bins, twice, 64, err, sizeof err) != N) die("accumulation", err);
    for (size_t i = 0; i < (size_t)YFC_N_RANGES * (size_t)bins; ++i)
      if (twice[i] != 2 * wide[i]) die("accumulation", "a second call did not add the same counts");
    free(mm); free(twice); free(wide); free(thin); free(dot);
  }

  /* the refusals: nothing is written */
  uint64_t* counts = (uint64_t*)calloc((size_t)YFC_N_RANGES * 16, sizeof(uint64_t));
  float bad[2 * YFC_N_RANGES];
  if (!counts) return 2;
  must_refuse(frames, N, own, 0, counts, "bins is 0, expected 1 to 4096");
  must_refuse(frames, N, own, YFC_HIST_MAX_BINS + 1, counts, "bins is 4097, expected 1 to 4096");
  must_refuse(frames, N, own, -7, counts, "bins is -7");
  must_refuse(frames, 0, own, 16, counts, "n is 0, expected at least 1");
  must_refuse(frames, -1, own, 16, counts, "n is -1");
  must_refuse(NULL, N, own, 16, counts, "frames is NULL");
  must_refuse(frames, N, NULL, 16, counts, "minmax is NULL");
  must_refuse(frames, N, own, 16, NULL, "counts is NULL");
  memcpy(bad, own, sizeof bad); bad[2 * 7] = __builtin_nanf("");
  must_refuse(frames, N, bad, 16, counts, "tensor 57: the range is {");
  memcpy(bad, own, sizeof bad); bad[2 * 46 + 1] = __builtin_inff();
  must_refuse(frames, N, bad, 16, counts, "tensor 100: the range is {");
  memcpy(bad, own, sizeof bad); bad[2 * 17] = 3.0f; bad[2 * 17 + 1] = -2.0f;
  must_refuse(frames, N, bad, 16, counts, "tensor 68: max -2 is below min 3");
  for (int i = 0; i < YFC_N_RANGES * 16; ++i) if (counts[i]) die("refusals", "a refused call wrote counts");
  free(counts);
  yfw[9] ^= 0x40;                                       /* conv 0's record no longer matches the graph */
  char text[256] = "";
  uint64_t one[YFC_N_RANGES];
  memset(one, 0, sizeof one);
  if (yf_calib_host_histogram(yfw, yfw_bytes, frames, N, own, 1, one, 1, text, sizeof text) > 0 || !text[0]) die("a damaged .yfw", "not refused");
  ++refused;

  /* the kernel's tables: each step's window lies inside the arena, holds 4096 bins of every tensor the step has, and touches nothing the
   * step reads or writes */
  yfc_stage stages[YFC_N_STAGES];
  int32_t off[YFC_N_STAGES + 1], floats[YFC_N_STAGES + 1], least = YFC_ARENA_FLOATS;
  int8_t* writer = (int8_t*)malloc(YFC_ARENA_FLOATS);
  uint32_t* busy = (uint32_t*)malloc(sizeof(uint32_t) * YFC_ARENA_FLOATS);
  if (!writer || !busy) return 2;
  yfc_build_stages(stages, ids);
  yfc_hist_windows(stages, off, floats, writer, busy);
  for (int step = 0; step <= YFC_N_STAGES; ++step) {
    const yfc_stage* g = step ? &stages[step - 1] : NULL;
    const int tables = g ? (g->r_conv >= 0) + (g->r_leaky >= 0) + (g->r_add >= 0) : 1;
    const int lo = off[step], hi = off[step] + floats[step];
    if (lo < 0 || hi > YFC_ARENA_FLOATS || floats[step] < tables * YFC_HIST_MAX_BINS) die("windows", "a window is outside the arena or too small");
    if (!g) { if (lo < YFC_FRAME_BYTES) die("windows", "step 0 overlaps the input"); continue; }
    const int count = g->oh * g->ow * g->cout, in_end = g->in_off + g->h * g->w * g->cin;
    if (lo < in_end && g->in_off < hi) die("windows", "a window overlaps its stage's input");
    if (g->add_off >= 0 && lo < g->add_off + count && g->add_off < hi) die("windows", "a window overlaps its stage's ADD operand");
    for (int idx = 0; idx < count; ++idx) {
      const int at = g->out_off + idx / g->cout * g->out_cstride + g->out_coff + idx % g->cout;
      if (at >= lo && at < hi) die("windows", "a window overlaps its stage's output");
    }
    if (floats[step] < least) least = floats[step];
  }
  /* ... and nothing a LATER step still reads, restated here from the stage table alone (not from yfc_hist_windows' own bookkeeping): rd[x]
   * and wr[x] hold one bit per step that reads / writes arena float x.  A float of step t's window must not be touched by step t, and
   * walking the steps after t, it must be written again before it is read. */
  uint32_t* rd = (uint32_t*)calloc(YFC_ARENA_FLOATS, sizeof(uint32_t));
  uint32_t* wr = (uint32_t*)calloc(YFC_ARENA_FLOATS, sizeof(uint32_t));
  if (!rd || !wr) return 2;
  for (int x = 0; x < YFC_FRAME_BYTES; ++x) wr[x] |= 1u;
  for (int s = 0; s < YFC_N_STAGES; ++s) {
    const yfc_stage* g = &stages[s];
    const int count = g->oh * g->ow * g->cout;
    for (int x = g->in_off; x < g->in_off + g->h * g->w * g->cin; ++x) rd[x] |= 1u << (s + 1);
    for (int x = g->add_off; g->add_off >= 0 && x < g->add_off + count; ++x) rd[x] |= 1u << (s + 1);
    for (int idx = 0; idx < count; ++idx) wr[g->out_off + idx / g->cout * g->out_cstride + g->out_coff + idx % g->cout] |= 1u << (s + 1);
  }
  long checked = 0;
  for (int step = 0; step <= YFC_N_STAGES; ++step)
    for (int x = off[step]; x < off[step] + floats[step]; ++x, ++checked) {
      if ((rd[x] | wr[x]) >> step & 1u) die("windows", "a window holds a float its own step reads or writes");
      for (int later = step + 1; later <= YFC_N_STAGES; ++later) {
        if (rd[x] >> later & 1u) die("windows", "a window holds a float that a later step reads before anything rewrites it");
        if (wr[x] >> later & 1u) break;
      }
    }
  /* the check has teeth: the arena's first float, the input, is read by the first stage, so it may not lie in step 0's window */
  if (!(rd[0] >> 1 & 1u) || !(wr[0] & 1u) || off[0] == 0) die("windows", "the liveness check does not see the input");
  free(rd); free(wr);
  free(writer); free(busy); free(frames); free(yfw);
  printf("histograms: ok (%ld refusals; the smallest window holds %d floats; %ld window floats checked against later reads)\n", refused, (int)least, checked);
  return 0;
}
