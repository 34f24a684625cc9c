/* Per-channel sums of the raw output of every convolution, in the float32 evaluation of yf_calib_arith.h or in the simulated one of
 * yf_calib_sim.h, stated once for the kernel (yf_calib.hip) and the host build (yf_calib_host.c): the same C, compiled twice, with
 * -ffp-contract=off like its neighbours.  Plain C and HIP C++.  ("Channel-sum arithmetic")
 *
 * What empirical bias correction needs: the mean, per output channel of each convolution, of the quantised network's pre-activation output
 * against the float network's (calib.correct_biases folds the difference into the convolution's bias).
 *
 * THE VALUE SUMMED.  For the stage of convolution k (index in file order) the value is y = acc + bias: the float32 value
 * yfc_stage_element_sim holds before the stage's r_conv entry quantises it (yfc_stage_element_sim_raw returns it).  Pools have no bias and
 * contribute nothing.  With every entry of the table disabled this is the float evaluation's convolution output; with entries enabled the
 * simulated network's pre-requantisation output.
 * THE CHANNEL INDEX.  Convolutions in file order, channel co within each: first[k] + co, first[k] = the sum of cout over the earlier
 * convolutions; YFC_CHANNELS = 544 in all (checked against gen/yf_graph_gen.h by yfc_chan_layout).
 * THE ORDER IS PART OF THE DEFINITION.  Per frame and channel, with P = oh * ow pixels, p = oy * ow + ox:
 *   pixels are taken in chunks of 64 consecutive p;
 *   in a chunk lane l holds (double)y of pixel 64 * chunk + l, or +0.0 when that pixel does not exist;
 *   s[l] = s[l] + s[l + h] for l < h, h = 32, 16, 8, 4, 2, 1 (the halving of yf_calib_compare.h); the chunk's value is s[0];
 *   the frame's value for the channel is chunk 0, then + chunk 1, ... in ascending chunk order.
 * Over frames: frame 0's value, then + frame 1, ... in ascending order (yfc_chan_total: one thread per channel on the device), whatever
 * the grid was and whichever workgroup saw which frame.  A NaN or an infinity goes through as IEEE has it.
 * (On the device a chunk is a wave's task, the halving a shuffle; yfc_chan_chunk_value is the host's form.) */
#ifndef YF_CALIB_CHAN_H
#define YF_CALIB_CHAN_H
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/yf_calib.h"
#include "yf_calib_arith.h"
#include "yf_calib_sim.h"
#include "gen/yf_graph_gen.h"

enum { YFC_CHANNELS = YF_CALIB_CHANNELS, YFC_CHAN_CHUNK = 64,
       /* the doubles of one half of the chunk scratch [cout][chunks]: the largest stage is the 18-channel convolution of the first phase,
        * 784 pixels = 13 chunks at 56x56 and 6400 pixels = 100 chunks at 160x160 (yfc_chan_scratch_doubles computes it for a stage table) */
       YFC_CHAN_SCRATCH_56 = 18 * 13, YFC_CHAN_SCRATCH_MAX = 18 * 100,
       YFC_CHAN_OP_CONV_2D = 3, YFC_CHAN_OP_DEPTHWISE_CONV_2D = 4 };

/* The derived simulation table and, per stage, the first channel of its convolution (-1: a pool): travels as a kernel argument, so a launch
 * refers to nothing of the caller's. */
typedef struct {
  yfc_sim_plan sim;
  int16_t first[YFC_N_STAGES];
} yfc_chan_plan;

YFC_FN int yfc_chan_chunks(int pixels) { return (pixels + YFC_CHAN_CHUNK - 1) / YFC_CHAN_CHUNK; }

/* the totals: d_sums[c] from d_frame_sums[n][YFC_CHANNELS], the frames in ascending order */
YFC_FN double yfc_chan_total(const double* frame_sums, long n, int c) {
  double v = frame_sums[c];
  for (long f = 1; f < n; ++f) v = v + frame_sums[(size_t)f * YFC_CHANNELS + c];
  return v;
}

/* ---- host only ---- */
/* the halving of one chunk: s[0 .. 63], lanes without a pixel at +0.0; s is overwritten */
static inline double yfc_chan_chunk_value(double s[YFC_CHAN_CHUNK]) {
  for (int h = YFC_CHAN_CHUNK / 2; h; h >>= 1)
    for (int l = 0; l < h; ++l) s[l] = s[l] + s[l + h];
  return s[0];
}

/* One frame's value for channel co of a stage from the stage's raw values raw[p * cout + co], p < pixels. */
static inline double yfc_chan_frame_value(const float* raw, int pixels, int cout, int co) {
  double total = 0.0;
  for (int chunk = 0; chunk * YFC_CHAN_CHUNK < pixels; ++chunk) {
    double s[YFC_CHAN_CHUNK];
    for (int l = 0; l < YFC_CHAN_CHUNK; ++l) {
      const int p = chunk * YFC_CHAN_CHUNK + l;
      s[l] = p < pixels ? (double)raw[(size_t)p * cout + co] : 0.0;
    }
    const double v = yfc_chan_chunk_value(s);
    total = chunk ? total + v : v;
  }
  return total;
}

/* first[k], cout[k] and the pixels per frame of convolution k for a stage table; returns the number of channels, or -1 when the
 * convolutions do not appear in file order or differ from the graph's (gen/yf_graph_gen.h: the CONV_2D and DEPTHWISE_CONV_2D ops in op
 * order, the last dimension of their outputs). */
static inline int yfc_chan_layout(const yfc_stage stages[YFC_N_STAGES], int32_t first[YFC_N_CONVS], int32_t cout[YFC_N_CONVS],
                                  int32_t pixels[YFC_N_CONVS]) {
  int at = 0, k = 0, op = 0;
  for (int s = 0; s < YFC_N_STAGES; ++s) {
    const yfc_stage* g = &stages[s];
    if (g->kind != YFC_CONV) continue;
    if (g->conv != k || k >= YFC_N_CONVS) return -1;
    while (op < YF_GRAPH_N_OPS && yf_graph_ops[op].opcode != YFC_CHAN_OP_CONV_2D && yf_graph_ops[op].opcode != YFC_CHAN_OP_DEPTHWISE_CONV_2D) ++op;
    if (op >= YF_GRAPH_N_OPS || yf_graph_tensors[yf_graph_ops[op].out].shape[3] != g->cout) return -1;
    ++op;
    first[k] = at; cout[k] = g->cout; pixels[k] = g->oh * g->ow;
    at += g->cout;
    ++k;
  }
  return k == YFC_N_CONVS ? at : -1;
}

/* the doubles one half of the chunk scratch needs for a stage table: the largest cout * chunks of its convolutions */
static inline int yfc_chan_scratch_doubles(const yfc_stage stages[YFC_N_STAGES]) {
  int most = 0;
  for (int s = 0; s < YFC_N_STAGES; ++s) {
    const int need = stages[s].kind == YFC_CONV ? stages[s].cout * yfc_chan_chunks(stages[s].oh * stages[s].ow) : 0;
    most = need > most ? need : most;
  }
  return most;
}

/* The one check of a channel-sums call's arguments, for both builds: 0 and the plan, or 1 and a text that starts with `name` and names what
 * was refused.  n, frames, table and the table's entries go through yfc_sim_validate, so the texts are the simulation's. */
static inline int yfc_chan_validate(const char* name, const yfc_stage stages[YFC_N_STAGES], const void* frames, long n, const yf_calib_sim_entry* table,
                                    const void* frame_sums, yfc_chan_plan* plan, char* err, size_t errlen) {
  int32_t first[YFC_N_CONVS], cout[YFC_N_CONVS], pixels[YFC_N_CONVS];
  if (yfc_sim_validate(name, stages, frames, n, table, NULL, NULL, NULL, &plan->sim, err, errlen)) return 1;
  if (!frame_sums) {
    if (err && errlen) snprintf(err, errlen, "%s: frame_sums is NULL, expected room for %ld x %d doubles", name, n, (int)YFC_CHANNELS);
    return 1;
  }
  if (yfc_chan_layout(stages, first, cout, pixels) != YFC_CHANNELS) {
    if (err && errlen) snprintf(err, errlen, "%s: the stage table's convolutions do not give the graph's %d channels", name, (int)YFC_CHANNELS);
    return 1;
  }
  for (int s = 0; s < YFC_N_STAGES; ++s) plan->first[s] = stages[s].kind == YFC_CONV ? (int16_t)first[stages[s].conv] : (int16_t)-1;
  return 0;
}

#endif /* YF_CALIB_CHAN_H */
