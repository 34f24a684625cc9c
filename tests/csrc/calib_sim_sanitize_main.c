/* The simulation of the host build (csrc/yf_calib_host.c: yf_calib_host_simulate_hw, yf_calib_host_simulate, csrc/yf_calib_sim.h) under
 * ASan + UBSan, a program of its own: at 8x8 and 16x24 with three frames on two threads, an all-enabled table and a refused one, every buffer a
 * heap block of exactly its size, so an access past an end -- a table entry past the 50th, a record past the n-th, a QUANTIZE entry attached to
 * a stage that has none -- is a report.  Checked besides: with every entry disabled the logits are yf_calib_host_run_hw's bytes and the record
 * is zero but for sum_sq_ref; the 56x56 function is the _hw function at (56, 56); a refusal writes nothing.
 * argv[1]: a valid .yfw.  Prints "simulation: ok ..." and exits 0. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/yf_calib.h"
#include "../../stm32h7-yolo_amd/csrc/yf_calib_sim.h"

enum { N = 3, THREADS = 2 };
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

static yf_calib_sim_entry* table_all(void) {
  yf_calib_sim_entry* t = (yf_calib_sim_entry*)block(sizeof(yf_calib_sim_entry) * YF_CALIB_SIM_ENTRIES, 0);
  for (int i = 0; i < YF_CALIB_SIM_ENTRIES; ++i) { t[i].scale = 0.02f + 0.003f * (float)(i % 7); t[i].zero_point = (i * 37) % 256 - 128; }
  t[0].scale = 1.0f / 255.0f; t[0].zero_point = -128;
  return t;
}

static long run_size(int h, int w, int64_t* clipped) {
  yfc_dims d;
  yfc_dims_of(h, w, &d);
  char err[256] = "";
  int8_t* frames = (int8_t*)block((size_t)N * d.frame_bytes, 0);
  uint32_t x = 777u + (uint32_t)(h * 1000 + w);
  for (size_t i = 0; i < (size_t)N * d.frame_bytes; ++i) { x = x * 1664525u + 1013904223u; frames[i] = (int8_t)(x >> 24); }
  float* mm = (float*)block(sizeof(float) * 2 * YFC_N_RANGES, 0);
  int32_t* tensors = (int32_t*)block(sizeof(int32_t) * YFC_N_RANGES, 0);
  float* want = (float*)block(sizeof(float) * (size_t)N * d.logits, 0);
  float* ref = (float*)block(sizeof(float) * (size_t)N * d.logits, 0);
  float* logits = (float*)block(sizeof(float) * (size_t)N * d.logits, 0);
  yfc_cmp_frame* stats = (yfc_cmp_frame*)block(YF_CALIB_FRAME_STATS_BYTES * (size_t)N, 0);
  yfc_cmp_total* totals = (yfc_cmp_total*)block(YF_CALIB_TOTALS_BYTES, 0);
  yf_calib_sim_entry* none = (yf_calib_sim_entry*)block(sizeof(yf_calib_sim_entry) * YF_CALIB_SIM_ENTRIES, 0);
  yf_calib_sim_entry* all = table_all();

  if (yf_calib_host_run_hw(yfw, yfw_bytes, h, w, frames, N, mm, tensors, want, THREADS, err, sizeof err) != N) die("yf_calib_host_run_hw", err);
  if (yf_calib_host_simulate_hw(yfw, yfw_bytes, h, w, frames, N, none, NULL, ref, NULL, NULL, THREADS, err, sizeof err) != N) die("simulate, disabled", err);
  if (memcmp(ref, want, sizeof(float) * (size_t)N * d.logits)) die("simulate, disabled", "the logits are not the float evaluation's");
  if (yf_calib_host_simulate_hw(yfw, yfw_bytes, h, w, frames, N, none, ref, logits, stats, totals, THREADS, err, sizeof err) != N) die("simulate, disabled", err);
  for (int f = 0; f < N; ++f)
    if (stats[f].sum_err != 0.0 || stats[f].sum_sq_err != 0.0 || stats[f].max_abs_err != 0.0f || stats[f].saturated != 0 || !(stats[f].sum_sq_ref > 0.0))
      die("simulate, disabled", "the record is not zero but for sum_sq_ref");
  if (totals->elements != (int64_t)N * d.logits || totals->saturated != 0) die("simulate, disabled", "totals");

  if (yf_calib_host_simulate_hw(yfw, yfw_bytes, h, w, frames, N, all, ref, logits, stats, totals, THREADS, err, sizeof err) != N) die("simulate, all enabled", err);
  if (!(totals->sum_sq_err > 0.0) || totals->saturated < 1) die("simulate, all enabled", "no error or nothing clipped on these scales");
  int64_t sum = 0;
  for (int f = 0; f < N; ++f) sum += stats[f].saturated;
  if (sum != totals->saturated) die("simulate, all enabled", "the frames' clipped counts do not sum to the total");
  *clipped += totals->saturated;
  /* logits alone: no record asked for */
  float* again = (float*)block(sizeof(float) * (size_t)N * d.logits, 0);
  if (yf_calib_host_simulate_hw(yfw, yfw_bytes, h, w, frames, N, all, NULL, again, NULL, NULL, 1, err, sizeof err) != N) die("simulate, no reference", err);
  if (memcmp(again, logits, sizeof(float) * (size_t)N * d.logits)) die("simulate, no reference", "one thread and two differ");

  /* a refused table: nothing written */
  all[17].scale = -1.0f;
  memset(logits, 0x5a, sizeof(float) * (size_t)N * d.logits);
  memset(stats, 0x5a, YF_CALIB_FRAME_STATS_BYTES * (size_t)N);
  if (yf_calib_host_simulate_hw(yfw, yfw_bytes, h, w, frames, N, all, ref, logits, stats, totals, THREADS, err, sizeof err) > 0 ||
      !strstr(err, "entry 17 (tensor 68): scale is -1")) die("a refused table", err);
  all[17].scale = 0.05f;
  if (yf_calib_host_simulate_hw(yfw, yfw_bytes, h, w, frames, N, all, ref, logits, NULL, NULL, THREADS, err, sizeof err) > 0 ||
      !strstr(err, "yf_calib_host_simulate: ref_logits given without frame_stats")) die("reference logits without records", err);
  all[3].scale = 1e-39f;
  if (yf_calib_host_simulate_hw(yfw, yfw_bytes, h, w, frames, N, all, ref, logits, stats, totals, THREADS, err, sizeof err) > 0 ||
      !strstr(err, "entry 3 (tensor 53): scale is 1e-39, whose reciprocal is not a finite float32")) die("a subnormal scale", err);
  for (size_t i = 0; i < sizeof(float) * (size_t)N * d.logits; ++i) if (((unsigned char*)logits)[i] != 0x5a) die("a refused table", "logits were written");
  for (size_t i = 0; i < YF_CALIB_FRAME_STATS_BYTES * (size_t)N; ++i) if (((unsigned char*)stats)[i] != 0x5a) die("a refused table", "records were written");

  free(again); free(all); free(none); free(totals); free(stats); free(logits); free(ref); free(want); free(tensors); free(mm); free(frames);
  return (long)N * d.logits;
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

  /* the entries' tensors and the stages the QUANTIZE entries attach to, at every admitted size */
  int32_t ids[YFC_SIM_ENTRIES];
  yfc_sim_tensors(ids);
  if (ids[46] != 100 || ids[47] != 101 || ids[48] != 102 || ids[49] != 103) die("entries", "the QUANTIZE outputs are not 101, 102, 103");
  yf_calib_sim_entry* none = (yf_calib_sim_entry*)block(sizeof(yf_calib_sim_entry) * YF_CALIB_SIM_ENTRIES, 0);
  for (int h = 8; h <= YFC_MAX_SIDE; h += 8) {
    yfc_stage st[YFC_N_STAGES];
    int32_t slots[YFC_N_RANGES];
    yfc_sim_plan plan;
    char err[256] = "";
    yfc_build_stages_hw(st, slots, h, 8);
    if (yfc_sim_validate("plan", st, none, 1, none, NULL, NULL, NULL, &plan, err, sizeof err)) die("yfc_sim_validate", err);
    int attached = 0;
    for (int s = 0; s < YFC_N_STAGES; ++s) {
      const int q = plan.stage_q[s];
      if (q < 0) continue;
      ++attached;
      if (q < YFC_N_RANGES || q >= YFC_SIM_ENTRIES) die("plan", "a stage's QUANTIZE entry is outside 47 .. 49");
      const int want = st[s].t_conv == 74 ? 47 : st[s].t_leaky == 92 ? 48 : st[s].t_conv == 58 ? 49 : -1;
      if (q != want) die("plan", "a QUANTIZE entry is attached to another stage than pool 74, the convolution ending in 92, pool 58");
    }
    if (attached != 3) die("plan", "not three stages pass through a QUANTIZE op");
  }
  free(none);

  /* yfc_sim_q itself, on scale 1 and zero point 0: ties go to the even integer, the sign of a zero is kept, from 2^23 on a value is its own
   * integer, infinities clip, a NaN passes through and is not counted */
  {
    const yfc_sim_qp one = {1.0f, 1.0f, -128.0f, 127.0f};
    const float nan = __builtin_nanf(""), inf = __builtin_inff();
    const float v[17] = {0.5f, 1.5f, 2.5f, -0.5f, -1.5f, -0.3f, 0.3f, 8388607.5f, 8388608.0f, -8388609.0f, inf, -inf, nan, 126.5f, 127.5f, -128.5f, -129.5f};
    const float want[17] = {0.0f, 2.0f, 2.0f, -0.0f, -2.0f, -0.0f, 0.0f, 127.0f, 127.0f, -128.0f, 127.0f, -128.0f, nan, 126.0f, 127.0f, -128.0f, -128.0f};
    const float rints[10] = {0.0f, 2.0f, 2.0f, -0.0f, -2.0f, -0.0f, 0.0f, 8388608.0f, 8388608.0f, -8388609.0f};
    int32_t count = 0;
    for (int i = 0; i < 17; ++i) {
      const float got = yfc_sim_q(&one, v[i], &count);
      if (i == 12 ? got == got : memcmp(&got, &want[i], 4) != 0) die("yfc_sim_q", "a value of the rounding vector came out otherwise");
    }
    if (count != 7) die("yfc_sim_q", "the clipped count of the rounding vector is not 7 (a NaN is not counted)");
    for (int i = 0; i < 10; ++i) {
      const float got = yfc_sim_rint(v[i]);
      if (memcmp(&got, &rints[i], 4) != 0) die("yfc_sim_rint", "not round half to even with the sign kept");
    }
  }

  int64_t clipped = 0;
  long logits = run_size(8, 8, &clipped) + run_size(16, 24, &clipped);

  /* the 56x56 function forwards to the _hw function */
  {
    char err[256] = "";
    int8_t* frames = (int8_t*)block(YFC_FRAME_BYTES, 3);
    yf_calib_sim_entry* all = table_all();
    float* a = (float*)block(sizeof(float) * YFC_LOGITS, 0);
    float* b = (float*)block(sizeof(float) * YFC_LOGITS, 0);
    if (yf_calib_host_simulate(yfw, yfw_bytes, frames, 1, all, NULL, a, NULL, NULL, THREADS, err, sizeof err) != 1) die("yf_calib_host_simulate", err);
    if (yf_calib_host_simulate_hw(yfw, yfw_bytes, 56, 56, frames, 1, all, NULL, b, NULL, NULL, THREADS, err, sizeof err) != 1) die("yf_calib_host_simulate_hw", err);
    if (memcmp(a, b, sizeof(float) * YFC_LOGITS)) die("56x56", "the 56x56 function and the _hw function at (56, 56) differ");
    free(a); free(b); free(all); free(frames);
  }
  free(yfw);
  printf("simulation: ok (2 sizes, %ld logits, %lld values clipped, 20 plans)\n", logits, (long long)clipped);
  return 0;
}
