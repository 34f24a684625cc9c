/* Simulated quantisation inside the float32 evaluation of yf_calib_arith.h, stated once for the kernel (yf_calib.hip) and the host build
 * (yf_calib_host.c): the same C, compiled twice, with -ffp-contract=off like yf_calib_arith.h.  Plain C and HIP C++.
 * ("Simulation arithmetic")
 *
 * The evaluation runs as yfc_stage_element runs it, in float32, but a tensor whose ENTRY is enabled is put on its int8 grid where it is
 * produced: what one tensor's quantisation costs the logits is then the difference to the evaluation with every entry disabled.  This is
 * float arithmetic on the int8 grid; the engine's fixed-point requantisation, its LeakyReLU tables and its rounding variants are not
 * reproduced.
 *
 * THE TABLE has YFC_SIM_ENTRIES = 50 entries {scale, zero_point}: entries 0 .. 46 are the 47 range slots in the order of yf_calib_ranges
 * (YFC_RANGE_TENSORS), entries 47 .. 49 the outputs of the graph's three QUANTIZE ops in ascending tensor id (101, 102, 103: read from
 * gen/yf_graph_gen.h by yfc_sim_quantize_ops).  scale == 0: the tensor stays float.
 * Per enabled entry, on the host, once (yfc_sim_validate):
 *   inv = (float)(1.0 / (double)scale)     lo = (float)(-128 - zero_point)     hi = (float)(127 - zero_point)
 * Per value v (yfc_sim_q), every line one float32 operation, the comparisons written as in yf_calib_compare.h:
 *   t = v * inv
 *   r = rint(t)                            round half to even
 *   c = r < lo ? lo : (r > hi ? hi : r)
 *   clipped += (r < lo) | (r > hi)
 *   result = c * scale
 * A NaN passes through (both comparisons are false) and is not counted.
 * WHERE: the input by entry 0 when it is loaded into the arena; in a stage v[0] (the convolution's or pool's output) by the stage's r_conv
 * entry before the LeakyReLU reads it, v[1] by r_leaky before the ADD reads it, v[2] by r_add; and the value the stage stores once more by
 * the QUANTIZE entry when the graph passes that stage's output through a QUANTIZE op (pool 58, pool 74 and the convolution ending in tensor
 * 92).  A disabled entry is skipped, not multiplied by one: with every entry disabled the logits are yfc_stage_element's bit for bit.
 *
 * THE RECORD of a frame against reference logits is a yfc_cmp_frame over the frame's logits: e = simulated - reference, x = reference, the
 * sums of yfc_cmp_add without the int8 step (yfc_sim_cmp_add), in the lane, group and frame order yf_calib_compare.h defines (logit i belongs
 * to lane i mod 1024).  `saturated` is the frame's `clipped` count over all enabled entries: an integer, its order is free.  Totals over the
 * frames: yfc_cmp_total_field with one entry. */
#ifndef YF_CALIB_SIM_H
#define YF_CALIB_SIM_H
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../../include/yf_calib.h"
#include "yf_calib_arith.h"
#include "yf_calib_compare.h"
#include "gen/yf_graph_gen.h"

/* YFC_SIM_OP_QUANTIZE: the tflite builtin code of QUANTIZE as gen/yf_graph_gen.h carries it (the header has the codes as numbers only;
 * model_file.OPCODE is the Python side's list, and tests/test_calib_sim_host.py checks the entries this gives against the graph read there) */
enum { YFC_SIM_ENTRIES = YF_CALIB_SIM_ENTRIES, YFC_SIM_QUANTIZE_OPS = YFC_SIM_ENTRIES - YFC_N_RANGES, YFC_SIM_OP_QUANTIZE = 114 };

/* one entry as the evaluation reads it; scale == 0: disabled */
typedef struct { float scale, inv, lo, hi; } yfc_sim_qp;

/* The derived table and, per stage, the QUANTIZE entry its stored value passes through (or -1): small enough to travel as a kernel argument,
 * so a launch refers to nothing of the caller's and to nothing a later call rewrites. */
typedef struct {
  yfc_sim_qp e[YFC_SIM_ENTRIES];
  int8_t stage_q[YFC_N_STAGES];
} yfc_sim_plan;

#if defined(__cplusplus)
static_assert(sizeof(yfc_sim_qp) == 16 && sizeof(yf_calib_sim_entry) == 8 && YFC_SIM_QUANTIZE_OPS == 3, "table layouts");
#else
_Static_assert(sizeof(yfc_sim_qp) == 16 && sizeof(yf_calib_sim_entry) == 8 && YFC_SIM_QUANTIZE_OPS == 3, "table layouts");
#endif

/* rint in float32, round half to even.  The device has the instruction; the host form needs no libm: below 2^23 adding and subtracting 2^23
 * rounds to an integer in the default rounding mode (no contraction, no reassociation: -ffp-contract=off and no fast-math), the sign is put
 * back so that -0.3 gives -0 as rintf does, and from 2^23 on every float32 is an integer already (infinities and NaN pass). */
YFC_FN float yfc_sim_rint(float t) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_rintf(t);
#else
  const float a = __builtin_fabsf(t);
  if (!(a < 0x1p23f)) return t;
  const float r = (a + 0x1p23f) - 0x1p23f;
  return __builtin_copysignf(r, t);
#endif
}

YFC_FN float yfc_sim_q(const yfc_sim_qp* p, float v, int32_t* clipped) {
  const float t = v * p->inv;
  const float r = yfc_sim_rint(t);
  const float c = r < p->lo ? p->lo : (r > p->hi ? p->hi : r);
  *clipped += (r < p->lo) | (r > p->hi);
  return c * p->scale;
}

/* the input's value as the arena receives it */
YFC_FN float yfc_sim_input(const yfc_sim_plan* p, float v, int32_t* clipped) {
  return p->e[0].scale != 0.0f ? yfc_sim_q(&p->e[0], v, clipped) : v;
}

/* yfc_cmp_add without the int8 step: y the simulated logit, x the reference */
YFC_FN void yfc_sim_cmp_add(yfc_cmp_frame* a, float y, float x) {
  const float e = y - x;
  const double de = (double)e, dx = (double)x;
  const float ae = __builtin_fabsf(e);
  a->sum_err = a->sum_err + de;
  a->sum_sq_err = a->sum_sq_err + de * de;
  a->sum_sq_ref = a->sum_sq_ref + dx * dx;
  a->max_abs_err = ae > a->max_abs_err ? ae : a->max_abs_err;
}

/* One output element of stage `si` (s = &stages[si]) with the plan's quantisation: yfc_stage_element, and the four points above.  A COPY of
 * yfc_stage_element (yf_calib_arith.h), kept apart so that the bits of the existing kernels stay frozen: whoever edits one edits the other; the
 * all-disabled tests (equal to host_run / observe bit for bit) are what keeps the two in step.
 * In two parts, so that the channel sums (yf_calib_chan.h) can read the value between them: yfc_stage_element_sim_raw ends with the raw
 * value -- a convolution's y = acc + bias, a pool's maximum, before the stage's r_conv entry quantises it --, yfc_stage_element_sim_finish
 * is everything after and stores the element.  yfc_stage_element_sim is the two in a row. */
YFC_FN float yfc_stage_element_sim_raw(const yfc_stage* s, const float* arena, const float* params, int idx) {
  const int co = idx % s->cout, px = idx / s->cout;
  const int ox = px % s->ow, oy = px / s->ow;
  const int k = s->k, h = s->h, w = s->w, cin = s->cin;
  const float* x = arena + s->in_off;
  const int y0 = oy * s->stride - s->pad, x0 = ox * s->stride - s->pad;
  float y;
  if (s->kind == YFC_POOL) {
    y = -__builtin_inff();
    for (int fy = 0; fy < k; ++fy) {
      const int iy = y0 + fy;
      if (iy < 0 || iy >= h) continue;
      for (int fx = 0; fx < k; ++fx) {
        const int ix = x0 + fx;
        if (ix < 0 || ix >= w) continue;
        const float t = x[(iy * w + ix) * cin + co];
        y = t > y ? t : y;
      }
    }
  } else {
    const float* wt = params + s->w_off;
    float acc = 0.0f;
    for (int fy = 0; fy < k; ++fy) {
      const int iy = y0 + fy;
      if (iy < 0 || iy >= h) continue;
      for (int fx = 0; fx < k; ++fx) {
        const int ix = x0 + fx;
        if (ix < 0 || ix >= w) continue;
        if (s->dw) {
          acc = acc + x[(iy * w + ix) * cin + co] * wt[(fy * k + fx) * s->cout + co];
        } else {
          const float* xp = x + (iy * w + ix) * cin;
          const float* wp = wt + ((co * k + fy) * k + fx) * cin;
          for (int ci = 0; ci < cin; ++ci) acc = acc + xp[ci] * wp[ci];
        }
      }
    }
    y = acc + params[s->b_off + co];
  }
  return y;
}

YFC_FN void yfc_stage_element_sim_finish(const yfc_stage* s, int si, float* arena, int idx, float y, const yfc_sim_plan* p, int32_t* clipped) {
  const int co = idx % s->cout, px = idx / s->cout;
  if (p->e[s->r_conv].scale != 0.0f) y = yfc_sim_q(&p->e[s->r_conv], y, clipped);
  if (s->kind != YFC_POOL) {
    if (s->leaky) {
      y = y >= 0.0f ? y : y * YFC_LEAKY_ALPHA;
      if (p->e[s->r_leaky].scale != 0.0f) y = yfc_sim_q(&p->e[s->r_leaky], y, clipped);
    }
    if (s->add_off >= 0) {
      y = arena[s->add_off + idx] + y;
      if (p->e[s->r_add].scale != 0.0f) y = yfc_sim_q(&p->e[s->r_add], y, clipped);
    }
  }
  const int q = p->stage_q[si];
  if (q >= 0 && p->e[q].scale != 0.0f) y = yfc_sim_q(&p->e[q], y, clipped);
  arena[s->out_off + px * s->out_cstride + s->out_coff + co] = y;
}

YFC_FN void yfc_stage_element_sim(const yfc_stage* s, int si, float* arena, const float* params, int idx, const yfc_sim_plan* p, int32_t* clipped) {
  yfc_stage_element_sim_finish(s, si, arena, idx, yfc_stage_element_sim_raw(s, arena, params, idx), p, clipped);
}

/* ---- host only ----
 * The graph's QUANTIZE ops in ascending output tensor id: out[i] the tensor entry YFC_N_RANGES + i stands for, in[i] the tensor it copies.
 * Returns their number. */
static inline int yfc_sim_quantize_ops(int32_t out[YFC_SIM_QUANTIZE_OPS], int32_t in[YFC_SIM_QUANTIZE_OPS]) {
  int count = 0;
  for (int o = 0; o < YF_GRAPH_N_OPS; ++o) {
    if (yf_graph_ops[o].opcode != YFC_SIM_OP_QUANTIZE) continue;
    if (count < YFC_SIM_QUANTIZE_OPS) {
      int at = count;
      for (; at > 0 && out[at - 1] > yf_graph_ops[o].out; --at) { out[at] = out[at - 1]; in[at] = in[at - 1]; }
      out[at] = yf_graph_ops[o].out;
      in[at] = yf_graph_ops[o].ins[0];
    }
    ++count;
  }
  return count;
}

/* the tensor id of every entry */
static inline void yfc_sim_tensors(int32_t ids[YFC_SIM_ENTRIES]) {
  static const int32_t slots[YFC_N_RANGES] = { YFC_RANGE_TENSORS };
  int32_t in[YFC_SIM_QUANTIZE_OPS];
  for (int i = 0; i < YFC_N_RANGES; ++i) ids[i] = slots[i];
  for (int i = YFC_N_RANGES; i < YFC_SIM_ENTRIES; ++i) ids[i] = -1;
  (void)yfc_sim_quantize_ops(ids + YFC_N_RANGES, in);
}

/* The one check of a simulate call's arguments, for both builds: 0 and the plan, or 1 and a text that starts with `name` (the entry that was
 * called) and names what was refused (a table entry with its tensor id).  A scale whose reciprocal is not a finite float32 (a subnormal
 * one) is refused with the others: inv = inf would turn every zero activation into a NaN. */
static inline int yfc_sim_validate(const char* name, const yfc_stage stages[YFC_N_STAGES], const void* frames, long n, const yf_calib_sim_entry* table,
                                   const void* ref_logits, const void* frame_stats, const void* totals, yfc_sim_plan* plan, char* err,
                                   size_t errlen) {
#define YFC_SIM_REFUSE(fmt, ...) do { if (err && errlen) snprintf(err, errlen, "%s: " fmt, name, ##__VA_ARGS__); return 1; } while (0)
  const float top = 0x1.fffffep+127f;
  int32_t ids[YFC_SIM_ENTRIES], q_out[YFC_SIM_QUANTIZE_OPS], q_in[YFC_SIM_QUANTIZE_OPS];
  if (n < 1) YFC_SIM_REFUSE("n is %ld, expected at least 1", n);
  if (!frames || !table) YFC_SIM_REFUSE("%s is NULL", !frames ? "frames" : "table");
  if (!ref_logits && (frame_stats || totals))
    YFC_SIM_REFUSE("%s given without ref_logits, expected NULL: there is nothing to compare with", frame_stats ? "frame_stats" : "totals");
  if (ref_logits && !frame_stats) YFC_SIM_REFUSE("ref_logits given without frame_stats, expected room for %ld records: the comparison has nowhere to go", n);
  if (yfc_sim_quantize_ops(q_out, q_in) != YFC_SIM_QUANTIZE_OPS)
    YFC_SIM_REFUSE("the graph has %d QUANTIZE ops, expected %d", yfc_sim_quantize_ops(q_out, q_in), YFC_SIM_QUANTIZE_OPS);
  yfc_sim_tensors(ids);
  memset(plan, 0, sizeof *plan);
  for (int i = 0; i < YFC_SIM_ENTRIES; ++i) {
    const float scale = table[i].scale;
    const int32_t zp = table[i].zero_point;
    if (scale == 0.0f) continue;                           /* (a NaN is not 0) */
    if (!(scale > 0.0f && scale <= top))
      YFC_SIM_REFUSE("entry %d (tensor %d): scale is %g, expected 0 (the tensor stays float) or a finite positive float32", i, (int)ids[i],
                     (double)scale);
    if (zp < -128 || zp > 127) YFC_SIM_REFUSE("entry %d (tensor %d): zero_point is %d, expected -128 to 127", i, (int)ids[i], (int)zp);
    const float inv = (float)(1.0 / (double)scale);
    if (!(inv <= top))
      YFC_SIM_REFUSE("entry %d (tensor %d): scale is %g, whose reciprocal is not a finite float32; expected at least %g", i, (int)ids[i], (double)scale,
                     1.0 / (double)top);
    plan->e[i].scale = scale;
    plan->e[i].inv = inv;
    plan->e[i].lo = (float)(-128 - zp);
    plan->e[i].hi = (float)(127 - zp);
  }
  for (int s = 0; s < YFC_N_STAGES; ++s) {                 /* the tensor a stage stores: its last */
    const int32_t t = stages[s].t_add >= 0 ? stages[s].t_add : stages[s].t_leaky >= 0 ? stages[s].t_leaky : stages[s].t_conv;
    plan->stage_q[s] = -1;
    for (int i = 0; i < YFC_SIM_QUANTIZE_OPS; ++i)
      if (q_in[i] == t) plan->stage_q[s] = (int8_t)(YFC_N_RANGES + i);
  }
  return 0;
#undef YFC_SIM_REFUSE
}

#endif /* YF_CALIB_SIM_H */
