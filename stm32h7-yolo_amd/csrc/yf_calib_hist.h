/* Histograms of the 47 tensors calibration observes, stated once for the kernel (yf_calib.hip) and the host build (yf_calib_host.c): the same
 * C, compiled twice, with -ffp-contract=off like yf_calib_arith.h.  Plain C and HIP C++.  ("Histogram arithmetic")
 *
 * Every range slot (YFC_RANGE_TENSORS: the slot order and tensor ids of yf_calib_ranges) gets an AXIS built on the host from one
 * {min, max} pair in float32 (yfc_hist_validate):
 *   lo  = min
 *   inv = (float)bins / (max - min)       one float32 subtraction, one float32 division
 *   inv = 0 when max <= min or when the quotient is not finite
 * and a value's bin is yfc_hist_bin: one float32 subtraction, one float32 multiplication, a truncation.  What follows from that is the
 * library's choice:
 *   - a value outside [min, max] lands in an end bin (below: bin 0, above: bin bins - 1; -inf and +inf with them);
 *   - v == max lands in the last bin (t == bins exactly), so bin k holds edge[k] <= v < edge[k + 1] and the last bin is closed above;
 *   - a NaN lands in bin 0 (both comparisons are false);
 *   - with max == min every value lands in bin 0.
 * Counts are uint64_t and integer addition is exact: a histogram does not depend on which workgroup or thread saw which frame or in which
 * order the adds arrived.  The device and the host build agree EXACTLY. */
#ifndef YF_CALIB_HIST_H
#define YF_CALIB_HIST_H
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "yf_calib_arith.h"

enum { YFC_HIST_MAX_BINS = 4096 };

/* the 47 axes: small enough to travel as a kernel argument, so a launch refers to nothing of the caller's and to nothing a later call rewrites */
typedef struct { float lo[YFC_N_RANGES], inv[YFC_N_RANGES]; } yfc_hist_axes;

YFC_FN int yfc_hist_bin(float v, float lo, float inv, int bins) {
  const float t = (v - lo) * inv;
  return t >= (float)bins ? bins - 1 : t > 0.0f ? (int)t : 0;
}

/* ---- host only ----
 * The one check of a histogram call's arguments, for both builds: 0 and the axes, or 1 and a text that names what was refused. */
static inline int yfc_hist_validate(const void* frames, long n, const float* minmax, int bins, const void* counts, yfc_hist_axes* axes,
                                    char* err, size_t errlen) {
#define YFC_HIST_REFUSE(...) do { if (err && errlen) snprintf(err, errlen, __VA_ARGS__); return 1; } while (0)
  static const int32_t ids[YFC_N_RANGES] = { YFC_RANGE_TENSORS };
  const float top = 0x1.fffffep+127f;
  if (n < 1) YFC_HIST_REFUSE("histogram: n is %ld, expected at least 1", n);
  if (bins < 1 || bins > YFC_HIST_MAX_BINS) YFC_HIST_REFUSE("histogram: bins is %d, expected 1 to %d", bins, YFC_HIST_MAX_BINS);
  if (!frames || !minmax || !counts) YFC_HIST_REFUSE("histogram: %s is NULL", !frames ? "frames" : !minmax ? "minmax" : "counts");
  for (int r = 0; r < YFC_N_RANGES; ++r) {
    const float lo = minmax[2 * r], hi = minmax[2 * r + 1];
    if (!(lo >= -top && lo <= top && hi >= -top && hi <= top))
      YFC_HIST_REFUSE("histogram: tensor %d: the range is {%g, %g}, expected two finite float32", (int)ids[r], (double)lo, (double)hi);
    if (hi < lo) YFC_HIST_REFUSE("histogram: tensor %d: max %g is below min %g", (int)ids[r], (double)hi, (double)lo);
    const float width = hi - lo;
    const float q = (float)bins / width;
    axes->lo[r] = lo;
    axes->inv[r] = (hi <= lo || !(q >= -top && q <= top)) ? 0.0f : q;
  }
  return 0;
#undef YFC_HIST_REFUSE
}

/* Where the kernel keeps a stage's tables: for step 0 (the input's conversion) and step 1 + s (stage s), the largest run of arena floats
 * that the step neither reads nor writes and that holds no value a later step still reads -- the arena is full only while T57 is
 * written; every step leaves a dead run behind it.  Derived from the stage table, float by float: writer[x] is the step that last wrote
 * x; a float is busy from the step after its writer up to each step that reads it, and during the step that writes it. */
static inline void yfc_hist_windows(const yfc_stage stages[YFC_N_STAGES], int32_t off[YFC_N_STAGES + 1], int32_t floats[YFC_N_STAGES + 1],
                                    int8_t* writer /* [YFC_ARENA_FLOATS] */, uint32_t* busy /* [YFC_ARENA_FLOATS], bit = step */) {
  memset(busy, 0, sizeof(uint32_t) * YFC_ARENA_FLOATS);
  memset(writer, -1, YFC_ARENA_FLOATS);
  for (int x = 0; x < YFC_FRAME_BYTES; ++x) { writer[x] = 0; busy[x] |= 1u; }
  for (int s = 0; s < YFC_N_STAGES; ++s) {
    const yfc_stage* g = &stages[s];
    const int step = s + 1, count = g->oh * g->ow * g->cout;
    for (int pass = 0; pass < 2; ++pass) {
      const int from = pass ? g->add_off : g->in_off, len = pass ? count : g->h * g->w * g->cin;
      if (from < 0) continue;
      for (int x = from; x < from + len; ++x)
        for (int t = writer[x] < 0 ? step : writer[x] + 1; t <= step; ++t) busy[x] |= 1u << t;
    }
    for (int idx = 0; idx < count; ++idx) {
      const int x = g->out_off + idx / g->cout * g->out_cstride + g->out_coff + idx % g->cout;
      writer[x] = (int8_t)step;
      busy[x] |= 1u << step;
    }
  }
  for (int step = 0; step <= YFC_N_STAGES; ++step) {
    int best = 0, best_at = 0, run = 0;
    for (int x = 0; x < YFC_ARENA_FLOATS; ++x) {
      run = (busy[x] >> step & 1u) ? 0 : run + 1;
      if (run > best) { best = run; best_at = x + 1 - run; }
    }
    off[step] = best_at;
    floats[step] = best;
  }
}

#endif /* YF_CALIB_HIST_H */
