/* The float32 evaluation of the network that calibration observes, stated once for the kernel (yf_calib.hip) and the host build
 * (yf_calib_host.c, libyf_calib_host.so): the same C, compiled twice.  Plain C and HIP C++.
 *
 * The converter's calibrator runs optimised float kernels whose summation order is not published, so there is no literal arithmetic to
 * reproduce; this header DEFINES one ("Calibration arithmetic"):
 *   input       x = T[q + 128], T[p] = (float)((double)p / 255.0): tflite_quantize.py:55-58 (the table is built on the host, yfc_input_table)
 *   CONV_2D, DEPTHWISE_CONV_2D
 *               acc = 0; for fy, fx, ci ascending: acc = acc + x * w, product and sum rounded separately; taps in the padding are skipped;
 *               y = acc + bias.  Padding as in the int8 graph: one row and column before the first (the explicit PAD in front of the
 *               stride-2 convolutions, SAME of the 3x3 stride-1 ones, which also pads one behind the last)
 *   LEAKY_RELU  x >= 0 ? x : x * 0.1f (0x3dcccccd)
 *   MAX_POOL_2D the maximum over the in-bounds window
 *   ADD         a + b
 *   PAD, QUANTIZE, CONCATENATION move values: a pool and the convolution beside it write into the concatenated buffer directly.
 * NO CONTRACTION: every translation unit that includes this header is compiled with -ffp-contract=off (csrc/Makefile: the hipcc line through
 * CALIBFLAGS, whose default would be `fast`, and the gcc lines), so `acc + x * w` is v_mul_f32 + v_add_f32 / mulss + addss and never an fma.
 * Nothing here relies on intrinsics for that.
 *
 * Activations live in one arena of YFC_ARENA_FLOATS floats per frame in flight (LDS on the device: 156.8 KB of the CU's 160 KB); the
 * offsets below reuse the space of tensors that are dead.  At another frame size the same layout scales with the frame (yfc_build_stages_hw
 * below; the arena is then global memory on the device).  A stage is one convolution with the LeakyReLU and / or ADD that follows it, or
 * one pool; each output element is computed by yfc_stage_element from the arena and written back to it. */
#ifndef YF_CALIB_ARITH_H
#define YF_CALIB_ARITH_H
#include <stdint.h>

#if defined(__HIPCC__)
#define YFC_FN __host__ __device__ static inline
#else
#define YFC_FN static inline
#endif

enum { YFC_N_CONVS = 24, YFC_N_STAGES = 26, YFC_N_RANGES = 47, YFC_ARENA_FLOATS = 39200, YFC_FRAME_BYTES = 56 * 56 * 3, YFC_LOGITS = 7 * 7 * 18,
       YFC_INPUT_TABLE = 256, YFC_LOGITS_OFF = 18032 };
enum { YFC_CONV = 0, YFC_POOL = 1 };
#define YFC_LEAKY_ALPHA 0x1.99999ap-4f             /* 0x3dcccccd, the alpha of every LEAKY_RELU of the graph */

typedef struct {
  int32_t kind, conv, dw, k, stride, pad, leaky;   /* conv: index in file order; pad: rows / columns before the first */
  int32_t h, w, cin, oh, ow, cout;
  int32_t in_off, out_off, out_cstride, out_coff;  /* arena floats; the output pixel's channels start at out_off + pixel * out_cstride + out_coff */
  int32_t add_off;                                 /* the other ADD operand (same shape as the output), or -1 */
  int32_t w_off, b_off;                            /* floats into the parameter block: [T 256][conv 0 weights][conv 0 bias][conv 1 ...] */
  int32_t t_conv, t_leaky, t_add;                  /* the tensors (tflite ids) the stage observes: conv or pool output, ...; -1: none */
  int32_t r_conv, r_leaky, r_add;                  /* ... and their slots in the range table */
} yfc_stage;

/* The 26 stages.  {kind, conv, dw, k, stride, leaky,  h, w, cin, cout,  in_off, out_off, out_cstride, out_coff, add_off,  t_conv, t_leaky, t_add}
 * Arena (floats):  28x28 phase: input 0, T52 9408, T54 15680, T55 21952, T57 25088 (ends at 39200)
 *                  14x14 phase: cat71 0 (36 ch: pool_8 | T70), T61 7056, T62 10584, T64 11760, T66 18816, T68 25872, T73 27048
 *                  7x7 phase:   cat93 0 (48 ch: pool_25 | T92), T77 2352, T78 3528, T80 3920, T82 5880, T84 7840, T86 8232, T88 10192, T90 12152,
 *                               T95 12544, T97 14504, T99 16464, logits 18032 */
#define YFC_STAGE_ROWS \
  {YFC_CONV,  0, 0, 3, 2, 1,  56, 56,  3,  8,      0,  9408,  8,  0, -1,   51, 52, -1}, \
  {YFC_CONV,  1, 1, 3, 1, 1,  28, 28,  8,  8,   9408, 15680,  8,  0, -1,   53, 54, -1}, \
  {YFC_CONV,  2, 0, 1, 1, 0,  28, 28,  8,  4,  15680, 21952,  4,  0, -1,   55, -1, -1}, \
  {YFC_CONV,  3, 0, 1, 1, 1,  28, 28,  4, 18,  21952, 25088, 18,  0, -1,   56, 57, -1}, \
  {YFC_POOL, -1, 0, 8, 2, 0,  28, 28, 18, 18,  25088,     0, 36,  0, -1,   58, -1, -1}, \
  {YFC_CONV,  4, 1, 3, 2, 1,  28, 28, 18, 18,  25088,  7056, 18,  0, -1,   60, 61, -1}, \
  {YFC_CONV,  5, 0, 1, 1, 0,  14, 14, 18,  6,   7056, 10584,  6,  0, -1,   62, -1, -1}, \
  {YFC_CONV,  6, 0, 1, 1, 1,  14, 14,  6, 36,  10584, 11760, 36,  0, -1,   63, 64, -1}, \
  {YFC_CONV,  7, 1, 3, 1, 1,  14, 14, 36, 36,  11760, 18816, 36,  0, -1,   65, 66, -1}, \
  {YFC_CONV,  8, 0, 1, 1, 0,  14, 14, 36,  6,  18816, 25872,  6,  0, 10584, 67, -1, 68}, \
  {YFC_CONV,  9, 0, 1, 1, 1,  14, 14,  6, 18,  25872,     0, 36, 18, -1,   69, 70, -1}, \
  {YFC_CONV, 10, 0, 1, 1, 1,  14, 14, 36, 24,      0, 27048, 24,  0, -1,   72, 73, -1}, \
  {YFC_POOL, -1, 0, 4, 2, 0,  14, 14, 24, 24,  27048,     0, 48,  0, -1,   74, -1, -1}, \
  {YFC_CONV, 11, 1, 3, 2, 1,  14, 14, 24, 24,  27048,  2352, 24,  0, -1,   76, 77, -1}, \
  {YFC_CONV, 12, 0, 1, 1, 0,   7,  7, 24,  8,   2352,  3528,  8,  0, -1,   78, -1, -1}, \
  {YFC_CONV, 13, 0, 1, 1, 1,   7,  7,  8, 40,   3528,  3920, 40,  0, -1,   79, 80, -1}, \
  {YFC_CONV, 14, 1, 3, 1, 1,   7,  7, 40, 40,   3920,  5880, 40,  0, -1,   81, 82, -1}, \
  {YFC_CONV, 15, 0, 1, 1, 0,   7,  7, 40,  8,   5880,  7840,  8,  0,  3528, 83, -1, 84}, \
  {YFC_CONV, 16, 0, 1, 1, 1,   7,  7,  8, 40,   7840,  8232, 40,  0, -1,   85, 86, -1}, \
  {YFC_CONV, 17, 1, 3, 1, 1,   7,  7, 40, 40,   8232, 10192, 40,  0, -1,   87, 88, -1}, \
  {YFC_CONV, 18, 0, 1, 1, 0,   7,  7, 40,  8,  10192, 12152,  8,  0,  7840, 89, -1, 90}, \
  {YFC_CONV, 19, 0, 1, 1, 1,   7,  7,  8, 24,  12152,     0, 48, 24, -1,   91, 92, -1}, \
  {YFC_CONV, 20, 0, 1, 1, 1,   7,  7, 48, 40,      0, 12544, 40,  0, -1,   94, 95, -1}, \
  {YFC_CONV, 21, 1, 3, 1, 1,   7,  7, 40, 40,  12544, 14504, 40,  0, -1,   96, 97, -1}, \
  {YFC_CONV, 22, 0, 1, 1, 1,   7,  7, 40, 32,  14504, 16464, 32,  0, -1,   98, 99, -1}, \
  {YFC_CONV, 23, 0, 1, 1, 0,   7,  7, 32, 18,  16464, 18032, 18,  0, -1,  100, -1, -1},

/* The tensors whose extremes are observed, in slot order: the input, then every CONV_2D, DEPTHWISE_CONV_2D, LEAKY_RELU and ADD output in op
 * order (45 tensors with a quantisation of their own), and the two MAX_POOL_2D outputs 58 and 74.  The pools keep their input's parameters,
 * but a CONCATENATION output's range is the union of its inputs' ranges, and the minimum of a max-pool is not the minimum of its input. */
#define YFC_RANGE_TENSORS \
  0, 51, 52, 53, 54, 55, 56, 57, 58, 60, 61, 62, 63, 64, 65, 66, 67, 68, 69, 70, 72, 73, 74, 76, 77, 78, 79, 80, 81, 82, 83, 84, 85, 86, 87, 88, 89, 90, \
  91, 92, 94, 95, 96, 97, 98, 99, 100

/* The evaluation at another frame size.  Admitted: h and w each a multiple of 8 from 8 to YFC_MAX_SIDE, so the three stride-2 stages halve
 * exactly, nothing is larger than what the engine runs, and the arena stays bounded.  With cells = (h / 8) * (w / 8) -- 49 at 56x56 --
 * every tensor has cells / 49 times its 56x56 elements and every arena offset above is a multiple of 49, so the layout at h x w is the
 * 56x56 layout with every offset divided by 49 and multiplied by cells: the liveness argument carries over unchanged, because every tensor
 * scales by the same factor.  The arena is 800 * cells floats (320 000 floats = 1.28 MB at 160x160: global memory on the device). */
enum { YFC_MAX_SIDE = 160, YFC_SIDE_STEP = 8, YFC_BASE_CELLS = 49, YFC_ARENA_PER_CELL = YFC_ARENA_FLOATS / 49, YFC_LOGITS_PER_CELL = 18,
       YFC_N_SIDES = YFC_MAX_SIDE / YFC_SIDE_STEP };
#define YFC_SIZE_RULE "multiples of 8 from 8 to 160"

typedef struct {
  int32_t h, w, cells;
  int32_t frame_bytes;                             /* int8 [h][w][3] */
  int32_t logits, logits_off;                      /* float [h / 8][w / 8][18] and where the last stage leaves them in the arena */
  int32_t arena_floats;
} yfc_dims;

static inline int yfc_size_ok(long h, long w) {
  return h >= YFC_SIDE_STEP && h <= YFC_MAX_SIDE && h % YFC_SIDE_STEP == 0 && w >= YFC_SIDE_STEP && w <= YFC_MAX_SIDE && w % YFC_SIDE_STEP == 0;
}

/* (h, w) must be admitted */
static inline void yfc_dims_of(int h, int w, yfc_dims* d) {
  d->h = h; d->w = w;
  d->cells = (h / YFC_SIDE_STEP) * (w / YFC_SIDE_STEP);
  d->frame_bytes = h * w * 3;
  d->logits = d->cells * YFC_LOGITS_PER_CELL;
  d->logits_off = YFC_LOGITS_OFF / YFC_BASE_CELLS * d->cells;
  d->arena_floats = YFC_ARENA_PER_CELL * d->cells;
}

/* The stage table for a frame of h x w (admitted, see yfc_size_ok) with the derived fields filled in (host only; the kernel reads the copy
 * the library uploads). */
static inline void yfc_build_stages_hw(yfc_stage out[YFC_N_STAGES], int32_t range_tensors[YFC_N_RANGES], int h, int w) {
  static const int32_t rows[YFC_N_STAGES][18] = { YFC_STAGE_ROWS };
  static const int32_t slots[YFC_N_RANGES] = { YFC_RANGE_TENSORS };
  const int32_t h8 = h / YFC_SIDE_STEP, w8 = w / YFC_SIDE_STEP, cells = h8 * w8;
  int32_t w_off[YFC_N_CONVS], b_off[YFC_N_CONVS], at = YFC_INPUT_TABLE;
  for (int s = 0; s < YFC_N_STAGES; ++s) {                 /* (the convolutions appear in file order) */
    const int32_t* r = rows[s];
    if (r[0] != YFC_CONV) continue;
    w_off[r[1]] = at;
    at += r[2] ? r[3] * r[3] * r[9] : r[9] * r[3] * r[3] * r[8];
    b_off[r[1]] = at;
    at += r[9];
  }
  for (int i = 0; i < YFC_N_RANGES; ++i) range_tensors[i] = slots[i];
  for (int s = 0; s < YFC_N_STAGES; ++s) {
    const int32_t* r = rows[s];
    yfc_stage* g = &out[s];
    g->kind = r[0]; g->conv = r[1]; g->dw = r[2]; g->k = r[3]; g->stride = r[4]; g->leaky = r[5];
    g->h = r[6] / 7 * h8; g->w = r[7] / 7 * w8; g->cin = r[8]; g->cout = r[9];       /* the rows' sides are 56, 28, 14, 7 */
    g->in_off = r[10] / YFC_BASE_CELLS * cells; g->out_off = r[11] / YFC_BASE_CELLS * cells;
    g->out_cstride = r[12]; g->out_coff = r[13]; g->add_off = r[14] < 0 ? -1 : r[14] / YFC_BASE_CELLS * cells;
    g->t_conv = r[15]; g->t_leaky = r[16]; g->t_add = r[17];
    /* one row / column of padding before the first at 3x3 (PAD + VALID at stride 2, SAME at stride 1); a pool's SAME padding: (k - 2) / 2 */
    g->pad = g->kind == YFC_POOL ? (g->k - 2) / 2 : (g->k - 1) / 2;
    g->oh = (g->h + g->stride - 1) / g->stride;
    g->ow = (g->w + g->stride - 1) / g->stride;
    g->w_off = g->kind == YFC_CONV ? w_off[g->conv] : 0;
    g->b_off = g->kind == YFC_CONV ? b_off[g->conv] : 0;
    g->r_conv = g->r_leaky = g->r_add = -1;
    for (int i = 0; i < YFC_N_RANGES; ++i) {
      if (slots[i] == g->t_conv) g->r_conv = i;
      if (slots[i] == g->t_leaky) g->r_leaky = i;
      if (slots[i] == g->t_add) g->r_add = i;
    }
  }
}

/* ... and at 56x56, where h8 * w8 = 49 and every row stands as written */
static inline void yfc_build_stages(yfc_stage out[YFC_N_STAGES], int32_t range_tensors[YFC_N_RANGES]) {
  yfc_build_stages_hw(out, range_tensors, 56, 56);
}

/* T[p] = float32(p / 255.0), the division in double: what `img.astype(np.float32) / 255.0` ... astype(np.float32) gives a pixel */
static inline void yfc_input_table(float T[YFC_INPUT_TABLE]) {
  for (int p = 0; p < YFC_INPUT_TABLE; ++p) T[p] = (float)((double)p / 255.0);
}

/* One output element of a stage: idx = (oy * ow + ox) * cout + co.  v[0] the convolution's (or pool's) value, v[1] after the LeakyReLU,
 * v[2] after the ADD -- each meaningful only where the stage has that tensor.  The value the stage ends with is stored.
 * (yf_calib_sim.h holds a twin, yfc_stage_element_sim, with the simulated quantisation inserted: an edit here belongs there too.) */
YFC_FN void yfc_stage_element(const yfc_stage* s, float* arena, const float* params, int idx, float v[3]) {
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
    v[0] = y;
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
    v[0] = y;
    if (s->leaky) {
      y = y >= 0.0f ? y : y * YFC_LEAKY_ALPHA;
      v[1] = y;
    }
    if (s->add_off >= 0) {
      y = arena[s->add_off + idx] + y;
      v[2] = y;
    }
  }
  arena[s->out_off + px * s->out_cstride + s->out_coff + co] = y;
}

#endif /* YF_CALIB_ARITH_H */
