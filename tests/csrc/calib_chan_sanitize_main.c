/* The channel sums of the host build (csrc/yf_calib_host.c: yf_calib_host_channel_sums_hw, yf_calib_host_channel_sums, csrc/yf_calib_chan.h)
 * under ASan + UBSan, a program of its own: at 8x8 with three frames and at 56x56 with two, on two threads, with every entry disabled and with
 * every entry enabled, every buffer a heap block of exactly its size, so an access past an end -- a row past the n-th, a channel past the
 * 544th, a chunk's lane past the stage's last pixel -- is a report.  Checked besides: the totals are the rows added in ascending order; the
 * logits are yf_calib_host_simulate_hw's bytes; one thread and two give the same bytes; the 56x56 function is the _hw function at (56, 56);
 * the layout; a refusal writes nothing.
 * argv[1]: a valid .yfw.  Prints "channel sums: ok ..." and exits 0. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/yf_calib.h"
#include "../../stm32h7-yolo_amd/csrc/yf_calib_chan.h"

enum { THREADS = 2 };
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

static long run_size(int h, int w, int n) {
  yfc_dims d;
  yfc_dims_of(h, w, &d);
  char err[256] = "";
  const size_t row_bytes = sizeof(double) * YF_CALIB_CHANNELS, logit_bytes = sizeof(float) * (size_t)n * d.logits;
  int8_t* frames = (int8_t*)block((size_t)n * d.frame_bytes, 0);
  uint32_t x = 4242u + (uint32_t)(h * 1000 + w);
  for (size_t i = 0; i < (size_t)n * d.frame_bytes; ++i) { x = x * 1664525u + 1013904223u; frames[i] = (int8_t)(x >> 24); }
  yf_calib_sim_entry* none = (yf_calib_sim_entry*)block(sizeof(yf_calib_sim_entry) * YF_CALIB_SIM_ENTRIES, 0);
  yf_calib_sim_entry* all = table_all();
  double* rows = (double*)block(row_bytes * (size_t)n, 0);
  double* sums = (double*)block(row_bytes, 0);
  double* rows1 = (double*)block(row_bytes * (size_t)n, 0);
  float* logits = (float*)block(logit_bytes, 0);
  float* want = (float*)block(logit_bytes, 0);
  double moved = 0.0;

  for (int pass = 0; pass < 2; ++pass) {
    const yf_calib_sim_entry* table = pass ? all : none;
    if (yf_calib_host_channel_sums_hw(yfw, yfw_bytes, h, w, frames, n, table, rows, sums, logits, THREADS, err, sizeof err) != n) die("channel sums", err);
    if (yf_calib_host_simulate_hw(yfw, yfw_bytes, h, w, frames, n, table, NULL, want, NULL, NULL, THREADS, err, sizeof err) != n) die("simulate", err);
    if (memcmp(logits, want, logit_bytes)) die("channel sums", "the logits are not the simulation's");
    for (int c = 0; c < YF_CALIB_CHANNELS; ++c) {
      double v = rows[c];
      for (int f = 1; f < n; ++f) v = v + rows[(size_t)f * YF_CALIB_CHANNELS + c];
      if (memcmp(&v, &sums[c], sizeof v)) die("channel sums", "a total is not its rows added in ascending order");
      if (!(v == v)) die("channel sums", "a NaN on finite weights");
    }
    /* one thread, and neither totals nor logits asked for */
    if (yf_calib_host_channel_sums_hw(yfw, yfw_bytes, h, w, frames, n, table, rows1, NULL, NULL, 1, err, sizeof err) != n) die("channel sums, one thread", err);
    if (memcmp(rows, rows1, row_bytes * (size_t)n)) die("channel sums", "one thread and two differ");
    moved += sums[YF_CALIB_CHANNELS - 1];
  }

  /* refusals: nothing written */
  memset(rows, 0x5a, row_bytes * (size_t)n);
  memset(sums, 0x5a, row_bytes);
  memset(logits, 0x5a, logit_bytes);
  all[17].scale = -1.0f;
  if (yf_calib_host_channel_sums_hw(yfw, yfw_bytes, h, w, frames, n, all, rows, sums, logits, THREADS, err, sizeof err) > 0 ||
      !strstr(err, "yf_calib_host_channel_sums: entry 17 (tensor 68): scale is -1")) die("a refused table", err);
  all[17].scale = 0.05f;
  if (yf_calib_host_channel_sums_hw(yfw, yfw_bytes, h, w, frames, 0, all, rows, sums, logits, THREADS, err, sizeof err) > 0 ||
      !strstr(err, "yf_calib_host_channel_sums: n is 0, expected at least 1")) die("n = 0", err);
  if (yf_calib_host_channel_sums_hw(yfw, yfw_bytes, h, w, NULL, n, all, rows, sums, logits, THREADS, err, sizeof err) > 0 ||
      !strstr(err, "yf_calib_host_channel_sums: frames is NULL")) die("NULL frames", err);
  if (yf_calib_host_channel_sums_hw(yfw, yfw_bytes, h, w, frames, n, NULL, rows, sums, logits, THREADS, err, sizeof err) > 0 ||
      !strstr(err, "yf_calib_host_channel_sums: table is NULL")) die("NULL table", err);
  if (yf_calib_host_channel_sums_hw(yfw, yfw_bytes, h, w, frames, n, all, NULL, sums, logits, THREADS, err, sizeof err) > 0 ||
      !strstr(err, "yf_calib_host_channel_sums: frame_sums is NULL")) die("NULL frame_sums", err);
  if (yf_calib_host_channel_sums_hw(yfw, yfw_bytes, h + 4, w, frames, n, all, rows, sums, logits, THREADS, err, sizeof err) > 0 ||
      !strstr(err, "yf_calib_host_channel_sums: the frame size is h = ")) die("a refused size", err);
  if (yf_calib_host_channel_sums_hw(yfw, yfw_bytes - 1, h, w, frames, n, all, rows, sums, logits, THREADS, err, sizeof err) > 0) die("a truncated .yfw", "admitted");
  for (size_t i = 0; i < row_bytes * (size_t)n; ++i) if (((unsigned char*)rows)[i] != 0x5a) die("a refusal", "rows were written");
  for (size_t i = 0; i < row_bytes; ++i) if (((unsigned char*)sums)[i] != 0x5a) die("a refusal", "totals were written");
  for (size_t i = 0; i < logit_bytes; ++i) if (((unsigned char*)logits)[i] != 0x5a) die("a refusal", "logits were written");
  if (!(moved == moved)) die("channel sums", "not a number");

  free(want); free(logits); free(rows1); free(sums); free(rows); free(all); free(none); free(frames);
  return (long)n * YF_CALIB_CHANNELS;
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

  /* the layout, and the scratch bounds the kernels are compiled with, at every admitted size */
  int32_t* first = (int32_t*)block(sizeof(int32_t) * YF_CALIB_N_CONVS, 0);
  int32_t* cout = (int32_t*)block(sizeof(int32_t) * YF_CALIB_N_CONVS, 0);
  int32_t* pixels = (int32_t*)block(sizeof(int32_t) * YF_CALIB_N_CONVS, 0);
  if (yf_calib_channel_layout(first, cout, pixels) != YF_CALIB_CHANNELS) die("layout", "not 544 channels");
  if (first[0] != 0 || first[23] + cout[23] != YF_CALIB_CHANNELS || cout[23] != 18 || pixels[0] != 784 || pixels[23] != 49) die("layout", "first, cout or pixels");
  if (yf_calib_channel_layout(NULL, cout, pixels) > 0) die("layout", "a NULL argument was admitted");
  for (int h = 8; h <= YFC_MAX_SIDE; h += 8)
    for (int w = 8; w <= YFC_MAX_SIDE; w += 8) {
      yfc_stage st[YFC_N_STAGES];
      int32_t slots[YFC_N_RANGES];
      yfc_build_stages_hw(st, slots, h, w);
      const int need = yfc_chan_scratch_doubles(st);
      if (need < 1 || need > YFC_CHAN_SCRATCH_MAX || (h == 56 && w == 56 && need != YFC_CHAN_SCRATCH_56) || (h == 160 && w == 160 && need != YFC_CHAN_SCRATCH_MAX))
        die("scratch", "a size needs more chunk scratch than the kernels have");
      if (yfc_chan_layout(st, first, cout, pixels) != YF_CALIB_CHANNELS) die("layout", "not 544 channels at a size");
    }
  /* the halving: 64 ones give 64; a lone value in the last lane arrives */
  {
    double s[YFC_CHAN_CHUNK];
    for (int l = 0; l < YFC_CHAN_CHUNK; ++l) s[l] = 1.0;
    if (yfc_chan_chunk_value(s) != 64.0) die("halving", "64 ones");
    for (int l = 0; l < YFC_CHAN_CHUNK; ++l) s[l] = l == YFC_CHAN_CHUNK - 1 ? 0x1p-30 : 0.0;
    if (yfc_chan_chunk_value(s) != 0x1p-30) die("halving", "the last lane");
  }
  free(pixels); free(cout); free(first);

  long values = run_size(8, 8, 3) + run_size(56, 56, 2);

  /* the 56x56 function forwards to the _hw function */
  {
    char err[256] = "";
    int8_t* frames = (int8_t*)block(YFC_FRAME_BYTES, 3);
    yf_calib_sim_entry* all = table_all();
    double* a = (double*)block(sizeof(double) * YF_CALIB_CHANNELS, 0);
    double* b = (double*)block(sizeof(double) * YF_CALIB_CHANNELS, 0);
    if (yf_calib_host_channel_sums(yfw, yfw_bytes, frames, 1, all, a, NULL, NULL, THREADS, err, sizeof err) != 1) die("yf_calib_host_channel_sums", err);
    if (yf_calib_host_channel_sums_hw(yfw, yfw_bytes, 56, 56, frames, 1, all, b, NULL, NULL, THREADS, err, sizeof err) != 1) die("yf_calib_host_channel_sums_hw", err);
    if (memcmp(a, b, sizeof(double) * YF_CALIB_CHANNELS)) die("56x56", "the 56x56 function and the _hw function at (56, 56) differ");
    free(a); free(b); free(all); free(frames);
  }
  free(yfw);
  printf("channel sums: ok (2 sizes, 2 tables, %ld sums, 400 scratch bounds)\n", values);
  return 0;
}
