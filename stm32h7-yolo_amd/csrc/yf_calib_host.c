/* Host build of the calibration arithmetic (yf_calib_arith.h, the functions the kernel calls) with the .yfw parser: libyf_calib_host.so,
 * plain C, no HIP.  Compiled with -ffp-contract=off like the kernel: the two agree bit for bit. */
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/yf_calib.h"
#include "yf_calib_arith.h"
#include "yf_yfw.h"

typedef struct {
  const yfc_stage* stages;
  const float* params;
  const int8_t* frames;
  float* logits;
  long n, first, step;
  float mm[YFC_N_RANGES][2];
  int failed;
} job;

static void observe(float mm[2], float v) {
  if (v < mm[0]) mm[0] = v;
  if (v > mm[1]) mm[1] = v;
}

static void* run_job(void* arg) {
  job* j = (job*)arg;
  float* arena = (float*)malloc(sizeof(float) * YFC_ARENA_FLOATS);
  if (!arena) { j->failed = 1; return NULL; }
  for (long f = j->first; f < j->n; f += j->step) {
    const int8_t* q = j->frames + (size_t)f * YFC_FRAME_BYTES;
    for (int i = 0; i < YFC_FRAME_BYTES; ++i) {
      arena[i] = j->params[q[i] + 128];
      observe(j->mm[0], arena[i]);
    }
    for (int s = 0; s < YFC_N_STAGES; ++s) {
      const yfc_stage* g = &j->stages[s];
      const int count = g->oh * g->ow * g->cout;
      for (int idx = 0; idx < count; ++idx) {
        float v[3] = {0.0f, 0.0f, 0.0f};
        yfc_stage_element(g, arena, j->params, idx, v);
        if (g->r_conv >= 0) observe(j->mm[g->r_conv], v[0]);
        if (g->r_leaky >= 0) observe(j->mm[g->r_leaky], v[1]);
        if (g->r_add >= 0) observe(j->mm[g->r_add], v[2]);
      }
    }
    if (j->logits) memcpy(j->logits + (size_t)f * YFC_LOGITS, arena + YFC_LOGITS_OFF, sizeof(float) * YFC_LOGITS);
  }
  free(arena);
  return NULL;
}

#define REFUSE(...) do { if (err && errlen) snprintf(err, errlen, __VA_ARGS__); return -1; } while (0)

YF_CALIB_API long yf_calib_host_run(const void* yfw, size_t bytes, const int8_t* frames, long n, float* minmax, int32_t* tensors, float* logits,
                                    int threads, char* err, size_t errlen) {
  enum { MAX_THREADS = 64, PARAM_FLOATS = YFC_INPUT_TABLE + YF_YFW_FLOATS };
  float* p = (float*)malloc(sizeof(float) * PARAM_FLOATS);
  if (!p) REFUSE("yf_calib_host_run: out of memory");
  yfc_input_table(p);
  if (yf_yfw_parse(yfw, bytes, p + YFC_INPUT_TABLE, err, errlen)) { free(p); return -1; }
  if (!frames || !minmax || !tensors || n < 1) { free(p); REFUSE("yf_calib_host_run: frames, minmax or tensors is NULL, or n = %ld is below 1", n); }
  yfc_stage stages[YFC_N_STAGES];
  yfc_build_stages(stages, tensors);
  if (threads < 1) threads = 1;
  if (threads > MAX_THREADS) threads = MAX_THREADS;
  if ((long)threads > n) threads = (int)n;
  job* jobs = (job*)malloc(sizeof(job) * (size_t)threads);
  pthread_t tid[MAX_THREADS];
  if (!jobs) { free(p); REFUSE("yf_calib_host_run: out of memory"); }
  int started = 0, failed = 0;
  for (int t = 0; t < threads; ++t) {
    job* j = &jobs[t];
    j->stages = stages; j->params = p; j->frames = frames; j->logits = logits; j->n = n; j->first = t; j->step = threads; j->failed = 0;
    for (int r = 0; r < YFC_N_RANGES; ++r) { j->mm[r][0] = __builtin_inff(); j->mm[r][1] = -__builtin_inff(); }
  }
  for (int t = 1; t < threads; ++t) {
    if (pthread_create(&tid[t], NULL, run_job, &jobs[t]) != 0) { jobs[t].failed = 1; break; }
    started = t;
  }
  run_job(&jobs[0]);
  for (int t = 1; t <= started; ++t) pthread_join(tid[t], NULL);
  for (int t = 0; t < threads; ++t) failed |= jobs[t].failed;
  for (int r = 0; r < YFC_N_RANGES && !failed; ++r) {
    float lo = __builtin_inff(), hi = -__builtin_inff();
    for (int t = 0; t < threads; ++t) {
      if (jobs[t].mm[r][0] < lo) lo = jobs[t].mm[r][0];
      if (jobs[t].mm[r][1] > hi) hi = jobs[t].mm[r][1];
    }
    minmax[2 * r] = lo + 0.0f;                          /* (a zero comes out as +0 whichever sign was met first) */
    minmax[2 * r + 1] = hi + 0.0f;
  }
  free(jobs);
  free(p);
  if (failed) REFUSE("yf_calib_host_run: could not start a thread or allocate its arena");
  return n;
}
