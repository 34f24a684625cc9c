/* Per-tensor quantisation error of an int8 run of the network against the float32 evaluation of yf_calib_arith.h, stated once for the kernel
 * (yf_calib.hip) and the host build (yf_calib_host.c): the same C, compiled twice, with -ffp-contract=off like yf_calib_arith.h.
 *
 * An ENTRY names one tensor t of the 46 the 26 stages produce (YFC_RANGE_TENSORS without the input) with the int8 values some run gave it:
 * E = oh * ow * cout bytes per frame, unpadded NHWC (element i = (oy * ow + ox) * cout + co, the idx of yfc_stage_element), frame f's at
 * q + f * frame_stride, and the scale and zero point that relate them to real values.  x_i is the float32 value the evaluation gives the
 * element: v[0], v[1] or v[2] of yfc_stage_element, by which of the stage's t_conv, t_leaky, t_add is t.  ("Comparison arithmetic")
 *
 * Per element (yfc_cmp_add):
 *   d = (float)(q - zp) * scale        integer subtraction, exact conversion, one float32 multiply
 *   e = d - x                          one float32 subtraction
 *   sum_err    += (double)e            three double sums; the two products are exact in double (24-bit factors)
 *   sum_sq_err += (double)e * (double)e
 *   sum_sq_ref += (double)x * (double)x
 *   max_abs_err = |e| > max_abs_err ? |e| : max_abs_err        (a NaN never replaces it; starts at +0)
 *   saturated  += q == -128 || q == 127
 * Per frame, THE ORDER IS PART OF THE DEFINITION: element i belongs to lane i mod 1024; a lane adds its terms in ascending i into doubles that
 * start at +0.0; the 1024 lanes are 16 groups of 64 consecutive lanes; in a group s[l] = s[l] + s[l + h] for l < h, h = 32, 16, 8, 4, 2, 1, the
 * group's value is s[0]; the frame's value is g0, then + g1, ... + g15.  (On the device a lane is a thread, a group a wave, the halving a
 * shuffle; yfc_cmp_frame_value is the host's form.)  Maxima and counts are exact: their order is free.
 * Over frames: frame 0's value, then + frame 1, ... in ascending order (yfc_cmp_total_field: one thread per entry and field on the device),
 * whatever the grid was and whichever workgroup saw which frame. */
#ifndef YF_CALIB_COMPARE_H
#define YF_CALIB_COMPARE_H
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../../include/yf_calib.h"
#include "yf_calib_arith.h"

enum { YFC_CMP_LANES = 1024, YFC_CMP_GROUP = 64, YFC_CMP_GROUPS = YFC_CMP_LANES / YFC_CMP_GROUP, YFC_CMP_MAX_ENTRIES = YFC_N_RANGES - 1,
       YFC_CMP_FIELDS = 6 };

/* one frame of one entry: d_frame_stats[f][entry] */
typedef struct { double sum_err, sum_sq_err, sum_sq_ref; float max_abs_err; int32_t saturated; } yfc_cmp_frame;
/* one entry over all frames: d_totals[entry] */
typedef struct { double sum_err, sum_sq_err, sum_sq_ref; float max_abs_err; uint32_t reserved; int64_t saturated, elements; } yfc_cmp_total;

#if defined(__cplusplus)
static_assert(sizeof(yfc_cmp_frame) == 32 && sizeof(yfc_cmp_total) == 48, "record layouts");
#else
_Static_assert(sizeof(yfc_cmp_frame) == 32 && sizeof(yfc_cmp_total) == 48, "record layouts");
#endif

/* What the evaluation reads of the entries, checked and sorted by stage (yfc_cmp_validate): small enough to travel as a kernel argument, so
 * a launch keeps no reference to the caller's entries or to anything a later call rewrites. */
typedef struct {
  const int8_t* q[YFC_CMP_MAX_ENTRIES];
  uint64_t frame_stride[YFC_CMP_MAX_ENTRIES];
  float scale[YFC_CMP_MAX_ENTRIES];
  int32_t zero_point[YFC_CMP_MAX_ENTRIES];
  int32_t elements[YFC_CMP_MAX_ENTRIES];
  int32_t count;
  int8_t entry[YFC_N_STAGES][3];                 /* the entry that lists the stage's t_conv / t_leaky / t_add, or -1 */
} yfc_cmp_plan;

YFC_FN void yfc_cmp_zero(yfc_cmp_frame* a) {
  a->sum_err = 0.0; a->sum_sq_err = 0.0; a->sum_sq_ref = 0.0; a->max_abs_err = 0.0f; a->saturated = 0;
}

YFC_FN void yfc_cmp_add(yfc_cmp_frame* a, int q, int zero_point, float scale, float x) {
  const float d = (float)(q - zero_point) * scale;
  const float e = d - x;
  const double de = (double)e, dx = (double)x;
  const float ae = __builtin_fabsf(e);
  a->sum_err = a->sum_err + de;
  a->sum_sq_err = a->sum_sq_err + de * de;
  a->sum_sq_ref = a->sum_sq_ref + dx * dx;
  a->max_abs_err = ae > a->max_abs_err ? ae : a->max_abs_err;
  a->saturated += (q == -128) | (q == 127);
}

/* a = a + b field by field: how the 16 group values become the frame's, in ascending group order */
YFC_FN void yfc_cmp_join(yfc_cmp_frame* a, const yfc_cmp_frame* b) {
  a->sum_err = a->sum_err + b->sum_err;
  a->sum_sq_err = a->sum_sq_err + b->sum_sq_err;
  a->sum_sq_ref = a->sum_sq_ref + b->sum_sq_ref;
  a->max_abs_err = b->max_abs_err > a->max_abs_err ? b->max_abs_err : a->max_abs_err;
  a->saturated += b->saturated;
}

/* Field `field` (0 sum_err, 1 sum_sq_err, 2 sum_sq_ref, 3 max_abs_err, 4 saturated, 5 elements) of entry `entry`'s total over frames 0 .. n - 1
 * of stats[n][count], in ascending frame order. */
YFC_FN void yfc_cmp_total_field(const yfc_cmp_frame* stats, long n, int count, int entry, int elements, int field, yfc_cmp_total* out) {
  const yfc_cmp_frame* r = stats + entry;
  if (field < 3) {
    double s = field == 0 ? r->sum_err : field == 1 ? r->sum_sq_err : r->sum_sq_ref;
    for (long f = 1; f < n; ++f) {
      const yfc_cmp_frame* p = r + (size_t)f * count;
      s = s + (field == 0 ? p->sum_err : field == 1 ? p->sum_sq_err : p->sum_sq_ref);
    }
    if (field == 0) out->sum_err = s; else if (field == 1) out->sum_sq_err = s; else out->sum_sq_ref = s;
  } else if (field == 3) {
    float m = 0.0f;
    for (long f = 0; f < n; ++f) { const float t = r[(size_t)f * count].max_abs_err; m = t > m ? t : m; }
    out->max_abs_err = m;
    out->reserved = 0;
  } else if (field == 4) {
    int64_t c = 0;
    for (long f = 0; f < n; ++f) c += r[(size_t)f * count].saturated;
    out->saturated = c;
  } else {
    out->elements = (int64_t)elements * n;
  }
}

/* ---- host only (yfc_build_stages is, too) ----
 * The host's form of the per-frame order: lane[1024] accumulators (lane l holds elements l, l + 1024, ...) -> the frame's record.
 * lane[] is used up. */
static inline void yfc_cmp_frame_value(yfc_cmp_frame* lane, yfc_cmp_frame* out) {
  for (int g = 0; g < YFC_CMP_GROUPS; ++g) {
    yfc_cmp_frame* s = lane + g * YFC_CMP_GROUP;
    for (int h = YFC_CMP_GROUP / 2; h; h >>= 1)
      for (int l = 0; l < h; ++l) yfc_cmp_join(&s[l], &s[l + h]);
  }
  *out = lane[0];
  for (int g = 1; g < YFC_CMP_GROUPS; ++g) yfc_cmp_join(out, &lane[g * YFC_CMP_GROUP]);
}

/* The one check of a compare call's arguments, for both builds: 0 and the plan, or 1 and a text that names the entry, the field, the value
 * found and the value expected. */
static inline int yfc_cmp_validate(const yfc_stage stages[YFC_N_STAGES], const yf_calib_qtensor* entries, int count, long n, yfc_cmp_plan* plan,
                                   char* err, size_t errlen) {
#define YFC_CMP_REFUSE(...) do { if (err && errlen) snprintf(err, errlen, __VA_ARGS__); return 1; } while (0)
  if (n < 1) YFC_CMP_REFUSE("compare: n is %ld, expected at least 1", n);
  if (count < 1 || count > YFC_CMP_MAX_ENTRIES) YFC_CMP_REFUSE("compare: count is %d, expected 1 to %d", count, YFC_CMP_MAX_ENTRIES);
  if (!entries) YFC_CMP_REFUSE("compare: entries is NULL, expected %d entries", count);
  memset(plan, 0, sizeof *plan);
  memset(plan->entry, -1, sizeof plan->entry);
  plan->count = count;
  for (int i = 0; i < count; ++i) {
    const yf_calib_qtensor* e = &entries[i];
    int stage = -1, which = -1;
    for (int s = 0; s < YFC_N_STAGES && e->tensor > 0; ++s) {
      const int32_t t[3] = {stages[s].t_conv, stages[s].t_leaky, stages[s].t_add};
      for (int j = 0; j < 3; ++j) if (t[j] == e->tensor) { stage = s; which = j; }
    }
    if (stage < 0)
      YFC_CMP_REFUSE("entry %d: tensor is %d, expected one of the %d tensors the stages produce (51 to 100; no PAD, QUANTIZE or CONCATENATION output)",
                     i, (int)e->tensor, YFC_CMP_MAX_ENTRIES);
    if (plan->entry[stage][which] >= 0)
      YFC_CMP_REFUSE("entry %d: tensor is %d, which entry %d lists already; expected every tensor once", i, (int)e->tensor, plan->entry[stage][which]);
    if (!(e->scale > 0.0f && e->scale <= 0x1.fffffep+127f))
      YFC_CMP_REFUSE("entry %d: scale is %g, expected a finite positive float32", i, (double)e->scale);
    if (e->zero_point < -128 || e->zero_point > 127) YFC_CMP_REFUSE("entry %d: zero_point is %d, expected -128 to 127", i, (int)e->zero_point);
    if (!e->q) YFC_CMP_REFUSE("entry %d: q is NULL, expected the int8 values of tensor %d", i, (int)e->tensor);
    const int elements = stages[stage].oh * stages[stage].ow * stages[stage].cout;
    if (e->frame_stride < (size_t)elements)
      YFC_CMP_REFUSE("entry %d: frame_stride is %zu, expected at least the %d elements of tensor %d", i, e->frame_stride, elements, (int)e->tensor);
    plan->entry[stage][which] = (int8_t)i;
    plan->q[i] = (const int8_t*)e->q;
    plan->frame_stride[i] = e->frame_stride;
    plan->scale[i] = e->scale;
    plan->zero_point[i] = e->zero_point;
    plan->elements[i] = elements;
  }
  return 0;
#undef YFC_CMP_REFUSE
}
#endif /* YF_CALIB_COMPARE_H */
