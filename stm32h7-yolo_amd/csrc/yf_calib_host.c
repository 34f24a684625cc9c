/* Host build of the calibration arithmetic (yf_calib_arith.h, the functions the kernel calls) with the .yfw parser: libyf_calib_host.so,
 * plain C, no HIP.  Compiled with -ffp-contract=off like the kernel: the two agree bit for bit. */
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/yf_calib.h"
#include "yf_calib_arith.h"
#include "yf_calib_compare.h"
#include "yf_calib_hist.h"
#include "yf_calib_sim.h"
#include "yf_calib_chan.h"
#include "yf_yfw.h"

enum { MAX_THREADS = 64, PARAM_FLOATS = YFC_INPUT_TABLE + YF_YFW_FLOATS };

/* what every form's job starts with: the evaluation's tables and this thread's share of the frames (first, first + step, ... below n) */
typedef struct {
  const yfc_stage* stages;
  const yfc_dims* dims;
  const float* params;
  const int8_t* frames;
  long n, first, step;
  int failed;
} job_head;

typedef struct {
  job_head h;
  float* logits;
  float mm[YFC_N_RANGES][2];
} job;

static void observe(float mm[2], float v) {
  if (v < mm[0]) mm[0] = v;
  if (v > mm[1]) mm[1] = v;
}

static void* run_job(void* arg) {
  job* j = (job*)arg;
  float* arena = (float*)malloc(sizeof(float) * (size_t)j->h.dims->arena_floats);
  if (!arena) { j->h.failed = 1; return NULL; }
  for (long f = j->h.first; f < j->h.n; f += j->h.step) {
    const int8_t* q = j->h.frames + (size_t)f * (size_t)j->h.dims->frame_bytes;
    for (int i = 0; i < j->h.dims->frame_bytes; ++i) {
      arena[i] = j->h.params[q[i] + 128];
      observe(j->mm[0], arena[i]);
    }
    for (int s = 0; s < YFC_N_STAGES; ++s) {
      const yfc_stage* g = &j->h.stages[s];
      const int count = g->oh * g->ow * g->cout;
      for (int idx = 0; idx < count; ++idx) {
        float v[3] = {0.0f, 0.0f, 0.0f};
        yfc_stage_element(g, arena, j->h.params, idx, v);
        if (g->r_conv >= 0) observe(j->mm[g->r_conv], v[0]);
        if (g->r_leaky >= 0) observe(j->mm[g->r_leaky], v[1]);
        if (g->r_add >= 0) observe(j->mm[g->r_add], v[2]);
      }
    }
    if (j->logits) memcpy(j->logits + (size_t)f * (size_t)j->h.dims->logits, arena + j->h.dims->logits_off, sizeof(float) * (size_t)j->h.dims->logits);
  }
  free(arena);
  return NULL;
}

#define REFUSE(...) do { if (err && errlen) snprintf(err, errlen, __VA_ARGS__); return -1; } while (0)

/* what an entry has in hand once its frame size and its .yfw are accepted; params is malloc'ed and the entry's to free */
typedef struct {
  float* params;
  yfc_stage stages[YFC_N_STAGES];
  int32_t tensors[YFC_N_RANGES];
  yfc_dims dims;
  int threads;                                          /* 1 .. MAX_THREADS, and no more than n */
} setup;

/* How every entry begins: the one check of a frame size, the parameters out of the .yfw, the stage table and the sizes of h x w, the thread
 * count.  0, or -1 with the text written and nothing held. */
static int prepare(const char* name, const void* yfw, size_t bytes, int h, int w, long n, int threads, setup* s, char* err, size_t errlen) {
  if (!yfc_size_ok(h, w)) REFUSE("%s: the frame size is h = %d, w = %d, expected " YFC_SIZE_RULE " each", name, h, w);
  s->params = (float*)malloc(sizeof(float) * PARAM_FLOATS);
  if (!s->params) REFUSE("%s: out of memory", name);
  yfc_input_table(s->params);
  if (yf_yfw_parse(yfw, bytes, s->params + YFC_INPUT_TABLE, err, errlen)) { free(s->params); return -1; }
  yfc_build_stages_hw(s->stages, s->tensors, h, w);
  yfc_dims_of(h, w, &s->dims);
  if (threads < 1) threads = 1;
  if (threads > MAX_THREADS) threads = MAX_THREADS;
  if (n >= 1 && (long)threads > n) threads = (int)n;
  s->threads = threads;
  return 0;
}

static job_head head_of(const setup* s, const int8_t* frames, long n) {
  const job_head h = {s->stages, &s->dims, s->params, frames, n, 0, s->threads, 0};
  return h;
}

/* jobs[0 .. threads), `size` bytes each and a job_head first, become copies of *proto with first = the thread's index; `worker` runs job 0 on
 * the caller's thread and the others on threads of their own.  Nonzero when a thread could not be started or a worker failed. */
static int fan_out(void* jobs, const void* proto, size_t size, int threads, void* (*worker)(void*)) {
#define JOB(t) ((job_head*)((char*)jobs + (size_t)(t) * size))
  pthread_t tid[MAX_THREADS];
  int started = 0, failed = 0;
  for (int t = 0; t < threads; ++t) {
    memcpy(JOB(t), proto, size);
    JOB(t)->first = t;
  }
  for (int t = 1; t < threads; ++t) {
    if (pthread_create(&tid[t], NULL, worker, JOB(t)) != 0) { JOB(t)->failed = 1; break; }
    started = t;
  }
  worker(JOB(0));
  for (int t = 1; t <= started; ++t) pthread_join(tid[t], NULL);
  for (int t = 0; t < threads; ++t) failed |= JOB(t)->failed;
  return failed;
#undef JOB
}

YF_CALIB_API long yf_calib_host_run(const void* yfw, size_t bytes, const int8_t* frames, long n, float* minmax, int32_t* tensors, float* logits,
                                    int threads, char* err, size_t errlen) {
  return yf_calib_host_run_hw(yfw, bytes, 56, 56, frames, n, minmax, tensors, logits, threads, err, errlen);
}

YF_CALIB_API long yf_calib_host_run_hw(const void* yfw, size_t bytes, int h, int w, const int8_t* frames, long n, float* minmax, int32_t* tensors,
                                       float* logits, int threads, char* err, size_t errlen) {
  setup s;
  if (prepare("yf_calib_host_run", yfw, bytes, h, w, n, threads, &s, err, errlen)) return -1;
  if (!frames || !minmax || !tensors || n < 1) { free(s.params); REFUSE("yf_calib_host_run: frames, minmax or tensors is NULL, or n = %ld is below 1", n); }
  memcpy(tensors, s.tensors, sizeof s.tensors);
  threads = s.threads;
  job* jobs = (job*)malloc(sizeof(job) * (size_t)threads);
  if (!jobs) { free(s.params); REFUSE("yf_calib_host_run: out of memory"); }
  job proto = {head_of(&s, frames, n), logits, {{0.0f}}};
  for (int r = 0; r < YFC_N_RANGES; ++r) { proto.mm[r][0] = __builtin_inff(); proto.mm[r][1] = -__builtin_inff(); }
  const int failed = fan_out(jobs, &proto, sizeof proto, threads, run_job);
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
  free(s.params);
  if (failed) REFUSE("yf_calib_host_run: could not start a thread or allocate its arena");
  return n;
}

/* ---- the comparison (yf_calib_compare.h): the evaluation again, with the lanes of the defined order as an array ---- */
typedef struct {
  job_head h;
  const yfc_cmp_plan* plan;
  const size_t* out_off;                                /* where entry e's [n][elements] block starts in tensors_out */
  yfc_cmp_frame* stats;
  float* tensors_out;
} cmp_job;

static void* run_cmp_job(void* arg) {
  cmp_job* j = (cmp_job*)arg;
  const yfc_cmp_plan* p = j->plan;
  float* arena = (float*)malloc(sizeof(float) * (size_t)j->h.dims->arena_floats);
  yfc_cmp_frame* lanes = (yfc_cmp_frame*)malloc(sizeof(yfc_cmp_frame) * 3 * YFC_CMP_LANES);
  if (!arena || !lanes) { free(arena); free(lanes); j->h.failed = 1; return NULL; }
  for (long f = j->h.first; f < j->h.n; f += j->h.step) {
    const int8_t* q = j->h.frames + (size_t)f * (size_t)j->h.dims->frame_bytes;
    for (int i = 0; i < j->h.dims->frame_bytes; ++i) arena[i] = j->h.params[q[i] + 128];
    for (int s = 0; s < YFC_N_STAGES; ++s) {
      const yfc_stage* g = &j->h.stages[s];
      const int count = g->oh * g->ow * g->cout;
      const int8_t* qt[3] = {NULL, NULL, NULL};
      float* xt[3] = {NULL, NULL, NULL};
      for (int k = 0; k < 3; ++k) {
        const int e = p->entry[s][k];
        if (e < 0) continue;
        qt[k] = p->q[e] + (size_t)f * p->frame_stride[e];
        if (j->tensors_out) xt[k] = j->tensors_out + j->out_off[e] + (size_t)f * count;
        for (int l = 0; l < YFC_CMP_LANES; ++l) yfc_cmp_zero(&lanes[k * YFC_CMP_LANES + l]);
      }
      for (int idx = 0; idx < count; ++idx) {
        float v[3] = {0.0f, 0.0f, 0.0f};
        yfc_stage_element(g, arena, j->h.params, idx, v);
        for (int k = 0; k < 3; ++k) {
          const int e = p->entry[s][k];
          if (e < 0) continue;
          yfc_cmp_add(&lanes[k * YFC_CMP_LANES + idx % YFC_CMP_LANES], qt[k][idx], p->zero_point[e], p->scale[e], v[k]);
          if (xt[k]) xt[k][idx] = v[k];
        }
      }
      for (int k = 0; k < 3; ++k)
        if (p->entry[s][k] >= 0) yfc_cmp_frame_value(&lanes[k * YFC_CMP_LANES], &j->stats[(size_t)f * p->count + p->entry[s][k]]);
    }
  }
  free(arena);
  free(lanes);
  return NULL;
}

YF_CALIB_API long yf_calib_host_compare(const void* yfw, size_t bytes, const int8_t* frames, long n, const yf_calib_qtensor* entries, int count,
                                        void* frame_stats, void* totals, float* tensors_out, int threads, char* err, size_t errlen) {
  return yf_calib_host_compare_hw(yfw, bytes, 56, 56, frames, n, entries, count, frame_stats, totals, tensors_out, threads, err, errlen);
}

YF_CALIB_API long yf_calib_host_compare_hw(const void* yfw, size_t bytes, int h, int w, const int8_t* frames, long n, const yf_calib_qtensor* entries,
                                           int count, void* frame_stats, void* totals, float* tensors_out, int threads, char* err, size_t errlen) {
  setup s;
  if (prepare("yf_calib_host_compare", yfw, bytes, h, w, n, threads, &s, err, errlen)) return -1;
  if (!frames || !frame_stats) { free(s.params); REFUSE("yf_calib_host_compare: frames or frame_stats is NULL"); }
  yfc_cmp_plan plan;
  if (yfc_cmp_validate(s.stages, entries, count, n, &plan, err, errlen)) { free(s.params); return -1; }
  size_t out_off[YFC_CMP_MAX_ENTRIES], at = 0;
  for (int e = 0; e < count; ++e) { out_off[e] = at; at += (size_t)n * (size_t)plan.elements[e]; }
  const cmp_job proto = {head_of(&s, frames, n), &plan, out_off, (yfc_cmp_frame*)frame_stats, tensors_out};
  cmp_job jobs[MAX_THREADS];
  const int failed = fan_out(jobs, &proto, sizeof proto, s.threads, run_cmp_job);
  free(s.params);
  if (failed) REFUSE("yf_calib_host_compare: could not start a thread or allocate its arena");
  if (totals)
    for (int e = 0; e < count; ++e)
      for (int field = 0; field < YFC_CMP_FIELDS; ++field)
        yfc_cmp_total_field((const yfc_cmp_frame*)frame_stats, n, count, e, plan.elements[e], field, (yfc_cmp_total*)totals + e);
  return n;
}

/* ---- the histograms (yf_calib_hist.h): the evaluation again, every value counted in its bin; a table per thread, added up at the end ---- */
typedef struct {
  job_head h;
  const yfc_hist_axes* axes;
  uint64_t* tables;                                     /* [threads][YFC_N_RANGES][bins]: every thread counts in its own */
  int bins;
} hist_job;

static void* run_hist_job(void* arg) {
  hist_job* j = (hist_job*)arg;
  const yfc_hist_axes* a = j->axes;
  const int bins = j->bins;
  uint64_t* counts = j->tables + (size_t)j->h.first * YFC_N_RANGES * (size_t)bins;     /* (first: the thread's index) */
  float* arena = (float*)malloc(sizeof(float) * (size_t)j->h.dims->arena_floats);
  if (!arena) { j->h.failed = 1; return NULL; }
  for (long f = j->h.first; f < j->h.n; f += j->h.step) {
    const int8_t* q = j->h.frames + (size_t)f * (size_t)j->h.dims->frame_bytes;
    for (int i = 0; i < j->h.dims->frame_bytes; ++i) {
      arena[i] = j->h.params[q[i] + 128];
      counts[yfc_hist_bin(arena[i], a->lo[0], a->inv[0], bins)] += 1;
    }
    for (int s = 0; s < YFC_N_STAGES; ++s) {
      const yfc_stage* g = &j->h.stages[s];
      const int count = g->oh * g->ow * g->cout;
      const int slots[3] = {g->r_conv, g->r_leaky, g->r_add};
      for (int idx = 0; idx < count; ++idx) {
        float v[3] = {0.0f, 0.0f, 0.0f};
        yfc_stage_element(g, arena, j->h.params, idx, v);
        for (int k = 0; k < 3; ++k)
          if (slots[k] >= 0) counts[(size_t)slots[k] * bins + yfc_hist_bin(v[k], a->lo[slots[k]], a->inv[slots[k]], bins)] += 1;
      }
    }
  }
  free(arena);
  return NULL;
}

YF_CALIB_API long yf_calib_host_histogram(const void* yfw, size_t bytes, const int8_t* frames, long n, const float* minmax, int bins,
                                          uint64_t* counts, int threads, char* err, size_t errlen) {
  return yf_calib_host_histogram_hw(yfw, bytes, 56, 56, frames, n, minmax, bins, counts, threads, err, errlen);
}

YF_CALIB_API long yf_calib_host_histogram_hw(const void* yfw, size_t bytes, int h, int w, const int8_t* frames, long n, const float* minmax, int bins,
                                             uint64_t* counts, int threads, char* err, size_t errlen) {
  setup s;
  if (prepare("yf_calib_host_histogram", yfw, bytes, h, w, n, threads, &s, err, errlen)) return -1;
  yfc_hist_axes axes;
  if (yfc_hist_validate(frames, n, minmax, bins, counts, &axes, err, errlen)) { free(s.params); return -1; }
  const size_t entries = (size_t)YFC_N_RANGES * (size_t)bins;
  uint64_t* tables = (uint64_t*)calloc((size_t)s.threads * entries, sizeof(uint64_t));
  if (!tables) { free(s.params); REFUSE("yf_calib_host_histogram: out of memory"); }
  const hist_job proto = {head_of(&s, frames, n), &axes, tables, bins};
  hist_job jobs[MAX_THREADS];
  const int failed = fan_out(jobs, &proto, sizeof proto, s.threads, run_hist_job);
  for (int t = 0; t < s.threads && !failed; ++t)
    for (size_t i = 0; i < entries; ++i) counts[i] += tables[(size_t)t * entries + i];
  free(tables);
  free(s.params);
  if (failed) REFUSE("yf_calib_host_histogram: could not start a thread or allocate its arena");
  return n;
}

/* ---- the simulation (yf_calib_sim.h): the evaluation with the enabled tensors on their int8 grids, and the head's record against reference logits ---- */
typedef struct {
  job_head h;
  const yfc_sim_plan* plan;
  const float* ref;
  float* logits;
  yfc_cmp_frame* stats;
} sim_job;

static void* run_sim_job(void* arg) {
  sim_job* j = (sim_job*)arg;
  const yfc_sim_plan* p = j->plan;
  const size_t logits = (size_t)j->h.dims->logits;
  float* arena = (float*)malloc(sizeof(float) * (size_t)j->h.dims->arena_floats);
  yfc_cmp_frame* lanes = (yfc_cmp_frame*)malloc(sizeof(yfc_cmp_frame) * YFC_CMP_LANES);
  if (!arena || !lanes) { free(arena); free(lanes); j->h.failed = 1; return NULL; }
  for (long f = j->h.first; f < j->h.n; f += j->h.step) {
    const int8_t* q = j->h.frames + (size_t)f * (size_t)j->h.dims->frame_bytes;
    int32_t clipped = 0;
    for (int i = 0; i < j->h.dims->frame_bytes; ++i) arena[i] = yfc_sim_input(p, j->h.params[q[i] + 128], &clipped);
    for (int s = 0; s < YFC_N_STAGES; ++s) {
      const yfc_stage* g = &j->h.stages[s];
      const int count = g->oh * g->ow * g->cout;
      for (int idx = 0; idx < count; ++idx) yfc_stage_element_sim(g, s, arena, j->h.params, idx, p, &clipped);
    }
    const float* y = arena + j->h.dims->logits_off;
    if (j->logits) memcpy(j->logits + (size_t)f * logits, y, sizeof(float) * logits);
    if (j->ref) {
      const float* x = j->ref + (size_t)f * logits;
      for (int l = 0; l < YFC_CMP_LANES; ++l) yfc_cmp_zero(&lanes[l]);
      for (size_t i = 0; i < logits; ++i) yfc_sim_cmp_add(&lanes[i % YFC_CMP_LANES], y[i], x[i]);
      yfc_cmp_frame_value(lanes, &j->stats[f]);
      j->stats[f].saturated = clipped;
    }
  }
  free(arena);
  free(lanes);
  return NULL;
}

YF_CALIB_API long yf_calib_host_simulate(const void* yfw, size_t bytes, const int8_t* frames, long n, const yf_calib_sim_entry* table,
                                         const float* ref_logits, float* logits, void* frame_stats, void* totals, int threads, char* err,
                                         size_t errlen) {
  return yf_calib_host_simulate_hw(yfw, bytes, 56, 56, frames, n, table, ref_logits, logits, frame_stats, totals, threads, err, errlen);
}

YF_CALIB_API long yf_calib_host_simulate_hw(const void* yfw, size_t bytes, int h, int w, const int8_t* frames, long n,
                                            const yf_calib_sim_entry* table, const float* ref_logits, float* logits, void* frame_stats,
                                            void* totals, int threads, char* err, size_t errlen) {
  setup s;
  if (prepare("yf_calib_host_simulate", yfw, bytes, h, w, n, threads, &s, err, errlen)) return -1;
  yfc_sim_plan plan;
  if (yfc_sim_validate("yf_calib_host_simulate", s.stages, frames, n, table, ref_logits, frame_stats, totals, &plan, err, errlen)) { free(s.params); return -1; }
  const sim_job proto = {head_of(&s, frames, n), &plan, ref_logits, logits, ref_logits ? (yfc_cmp_frame*)frame_stats : NULL};
  sim_job jobs[MAX_THREADS];
  const int failed = fan_out(jobs, &proto, sizeof proto, s.threads, run_sim_job);
  free(s.params);
  if (failed) REFUSE("yf_calib_host_simulate: could not start a thread or allocate its arena");
  if (ref_logits && totals)
    for (int field = 0; field < YFC_CMP_FIELDS; ++field)
      yfc_cmp_total_field((const yfc_cmp_frame*)frame_stats, n, 1, 0, s.dims.logits, field, (yfc_cmp_total*)totals);
  return n;
}

/* ---- the channel sums (yf_calib_chan.h): the simulation again, the raw value of every convolution kept for the stage and added per channel in
 * the defined order ---- */
typedef struct {
  job_head h;
  const yfc_chan_plan* plan;
  double* frame_sums;
  float* logits;
} chan_job;

static void* run_chan_job(void* arg) {
  chan_job* j = (chan_job*)arg;
  const yfc_sim_plan* p = &j->plan->sim;
  const size_t logits = (size_t)j->h.dims->logits;
  float* arena = (float*)malloc(sizeof(float) * (size_t)j->h.dims->arena_floats);
  float* raw = (float*)malloc(sizeof(float) * (size_t)j->h.dims->arena_floats);      /* (no stage has more elements than the arena has floats) */
  if (!arena || !raw) { free(arena); free(raw); j->h.failed = 1; return NULL; }
  for (long f = j->h.first; f < j->h.n; f += j->h.step) {
    const int8_t* q = j->h.frames + (size_t)f * (size_t)j->h.dims->frame_bytes;
    double* row = j->frame_sums + (size_t)f * YFC_CHANNELS;
    int32_t clipped = 0;
    for (int i = 0; i < j->h.dims->frame_bytes; ++i) arena[i] = yfc_sim_input(p, j->h.params[q[i] + 128], &clipped);
    for (int s = 0; s < YFC_N_STAGES; ++s) {
      const yfc_stage* g = &j->h.stages[s];
      const int pixels = g->oh * g->ow, count = pixels * g->cout;
      for (int idx = 0; idx < count; ++idx) {
        raw[idx] = yfc_stage_element_sim_raw(g, arena, j->h.params, idx);
        yfc_stage_element_sim_finish(g, s, arena, idx, raw[idx], p, &clipped);
      }
      if (g->kind != YFC_CONV) continue;
      for (int co = 0; co < g->cout; ++co) row[j->plan->first[s] + co] = yfc_chan_frame_value(raw, pixels, g->cout, co);
    }
    if (j->logits) memcpy(j->logits + (size_t)f * logits, arena + j->h.dims->logits_off, sizeof(float) * logits);
  }
  free(arena);
  free(raw);
  return NULL;
}

YF_CALIB_API long yf_calib_host_channel_sums(const void* yfw, size_t bytes, const int8_t* frames, long n, const yf_calib_sim_entry* table,
                                             double* frame_sums, double* sums, float* logits, int threads, char* err, size_t errlen) {
  return yf_calib_host_channel_sums_hw(yfw, bytes, 56, 56, frames, n, table, frame_sums, sums, logits, threads, err, errlen);
}

YF_CALIB_API long yf_calib_host_channel_sums_hw(const void* yfw, size_t bytes, int h, int w, const int8_t* frames, long n,
                                                const yf_calib_sim_entry* table, double* frame_sums, double* sums, float* logits, int threads,
                                                char* err, size_t errlen) {
  setup s;
  if (prepare("yf_calib_host_channel_sums", yfw, bytes, h, w, n, threads, &s, err, errlen)) return -1;
  yfc_chan_plan plan;
  if (yfc_chan_validate("yf_calib_host_channel_sums", s.stages, frames, n, table, frame_sums, &plan, err, errlen)) { free(s.params); return -1; }
  const chan_job proto = {head_of(&s, frames, n), &plan, frame_sums, logits};
  chan_job jobs[MAX_THREADS];
  const int failed = fan_out(jobs, &proto, sizeof proto, s.threads, run_chan_job);
  free(s.params);
  if (failed) REFUSE("yf_calib_host_channel_sums: could not start a thread or allocate its arena");
  if (sums)
    for (int c = 0; c < YFC_CHANNELS; ++c) sums[c] = yfc_chan_total(frame_sums, n, c);
  return n;
}

YF_CALIB_API int yf_calib_channel_layout(int32_t first[YF_CALIB_N_CONVS], int32_t cout[YF_CALIB_N_CONVS], int32_t pixels56[YF_CALIB_N_CONVS]) {
  yfc_stage stages[YFC_N_STAGES];
  int32_t range_tensors[YFC_N_RANGES];
  if (!first || !cout || !pixels56) return -1;
  yfc_build_stages(stages, range_tensors);
  return yfc_chan_layout(stages, first, cout, pixels56);
}
