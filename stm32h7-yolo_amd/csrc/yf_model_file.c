/* Parser of a .yfm model image for yf_network_init_model (plain C, no HIP, no allocation: it can be built and exercised alone, and
 * tests/csrc/model_file_sanitize_main.c does so under ASan + UBSan).
 *
 * The bytes are UNTRUSTED.  Every record is read with memcpy at an offset that was checked against the image size first; every offset a record
 * carries is checked against the data section in 64-bit arithmetic before it is used.  The image must then BE this network: the kernels are
 * built for one graph, only its quantisation and weights vary, so gen/yf_graph_gen.h (tools/gen_model.py) states the
 * graph and everything is compared with it.  What the table builder (yf_host_prep.c) assumes without reading it is checked here as well:
 *   - PAD ops 0, 9, 26: the builder takes the convolution's input parameters from the tensor BEFORE the PAD and fills halos with its zero point,
 *     so the PAD's output must carry its input's scale and zero point;
 *   - MAX_POOL_2D ops 8, 25: the pooling code moves bytes, and the QUANTIZE LUTs Q21 / Q45 are built from the pool's OUTPUT tensors 58 / 74;
 *   - CONCATENATION ops 22, 46: the concatenated buffer is read with the output's parameters;
 *   - filters are symmetric (zero point 0) and a bias is in units of s_in * s_w[c] with zero point 0: the accumulator adds it unscaled.
 * The input must be quantised as the frame producers write it (pixel - 128: the prepare kernels, the camera staging, libyf_images). */
#include "yf_model_file.h"
#include "gen/yf_graph_gen.h"
#include "yf_exp_f32.h"
#include <stdio.h>
#include <string.h>

enum { HDR = 24, TREC = 44, OREC = 52 };
enum { OP_ADD = 0, OP_CONCAT = 2, OP_CONV = 3, OP_DWCONV = 4, OP_MAXPOOL = 17, OP_PAD = 34, OP_LEAKY = 98, OP_QUANTIZE = 114 };
#define NO_DATA 0xFFFFFFFFu

typedef struct { int32_t shape[4]; uint32_t type; int32_t zp; uint32_t ns, soff; int32_t qdim; uint32_t doff, dbytes; } trec;

static uint32_t rd_u32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }
static int32_t rd_i32(const uint8_t* p) { int32_t v; memcpy(&v, p, 4); return v; }

#define REFUSE(...) do { if (err && errlen) snprintf(err, errlen, __VA_ARGS__); return 1; } while (0)

static int same_quant(const yf_model_file* o, int a, int b) { return o->scale_bits[a] == o->scale_bits[b] && o->zero_point[a] == o->zero_point[b]; }

int yf_model_file_parse(const void* yfm, size_t bytes, yf_model_file* out, char* err, size_t errlen) {
  if (!yfm || !out) REFUSE("model file: NULL argument");
  const uint8_t* b = (const uint8_t*)yfm;
  if (bytes < HDR) REFUSE("model file: %zu bytes, shorter than the 24-byte header", bytes);
  if (memcmp(b, "YFM1", 4) != 0) REFUSE("model file: magic is %02x %02x %02x %02x, expected 'YFM1'", b[0], b[1], b[2], b[3]);
  const uint32_t nt = rd_u32(b + 4), no = rd_u32(b + 8), tin = rd_u32(b + 12), tout = rd_u32(b + 16), nd = rd_u32(b + 20);
  if (nt != YF_N_TENSORS) REFUSE("model file: %u tensors, expected %d", nt, YF_N_TENSORS);
  if (no != YF_GRAPH_N_OPS) REFUSE("model file: %u ops, expected %d", no, YF_GRAPH_N_OPS);
  if (tin != YF_GRAPH_INPUT) REFUSE("model file: input tensor is %u, expected %d", tin, YF_GRAPH_INPUT);
  if (tout != YF_GRAPH_OUTPUT) REFUSE("model file: output tensor is %u, expected %d", tout, YF_GRAPH_OUTPUT);
  const uint64_t need = (uint64_t)HDR + (uint64_t)TREC * nt + (uint64_t)OREC * no + nd;
  if ((uint64_t)bytes != need) REFUSE("model file: %zu bytes, the header's counts and data size give %llu", bytes, (unsigned long long)need);
  const uint8_t* trecs = b + HDR;
  const uint8_t* orecs = trecs + (size_t)TREC * nt;
  const uint8_t* data = orecs + (size_t)OREC * no;

  memset(out, 0, sizeof *out);
  trec T[YF_N_TENSORS];
  for (int i = 0; i < YF_N_TENSORS; ++i) {
    const uint8_t* p = trecs + (size_t)TREC * i;
    trec* t = &T[i];
    for (int k = 0; k < 4; ++k) t->shape[k] = rd_i32(p + 4 * k);
    t->type = rd_u32(p + 16); t->zp = rd_i32(p + 20); t->ns = rd_u32(p + 24); t->soff = rd_u32(p + 28);
    t->qdim = rd_i32(p + 32); t->doff = rd_u32(p + 36); t->dbytes = rd_u32(p + 40);
    const yf_graph_tensor* g = &yf_graph_tensors[i];
    if (t->type > 1) REFUSE("tensor %d: type is %u, expected 0 (int8) or 1 (int32)", i, t->type);
    if (t->type != g->type) REFUSE("tensor %d: type is %u, expected %d", i, t->type, g->type);
    for (int k = 0; k < 4; ++k)
      if (t->shape[k] != g->shape[k]) REFUSE("tensor %d: shape[%d] is %d, expected %d", i, k, t->shape[k], g->shape[k]);
    if (t->qdim < 0 || t->qdim > 3) REFUSE("tensor %d: quantized_dimension is %d, expected 0..3", i, t->qdim);
    if (t->ns != 0 && t->ns != 1 && (int64_t)t->ns != (int64_t)t->shape[t->qdim])
      REFUSE("tensor %d: n_scales is %u, expected 1 or %d (the channels of dimension %d)", i, t->ns, t->shape[t->qdim], t->qdim);
    if (t->ns != g->n_scales) REFUSE("tensor %d: n_scales is %u, expected %d", i, t->ns, g->n_scales);
    if (t->ns > 1 && t->qdim != g->qdim) REFUSE("tensor %d: quantized_dimension is %d, expected %d", i, t->qdim, g->qdim);
    if (t->ns && (uint64_t)t->soff + 4ull * t->ns > nd)
      REFUSE("tensor %d: scales at soff %u (%u of them) end past the data section of %u bytes", i, t->soff, t->ns, nd);
    if (g->is_const) {
      if (t->doff == NO_DATA) REFUSE("tensor %d: has no data, expected a constant", i);
      const uint64_t want = (uint64_t)g->shape[0] * g->shape[1] * g->shape[2] * g->shape[3] * (g->type ? 4u : 1u);
      if (t->dbytes != want) REFUSE("tensor %d: dbytes is %u, expected %llu", i, t->dbytes, (unsigned long long)want);
      if ((uint64_t)t->doff + t->dbytes > nd) REFUSE("tensor %d: data at doff %u (dbytes %u) ends past the data section of %u bytes", i, t->doff, t->dbytes, nd);
    } else if (t->doff != NO_DATA) {
      REFUSE("tensor %d: doff is %u, expected 0xFFFFFFFF (an activation carries no data)", i, t->doff);
    }
    for (uint32_t k = 0; k < t->ns; ++k) {
      const uint32_t sb = rd_u32(data + t->soff + 4 * (size_t)k);
      if (sb == 0 || sb >= 0x7F800000u) REFUSE("tensor %d: scale[%u] has bits 0x%08x, expected a positive finite float32", i, k, sb);
    }
    if (t->ns == 1) {                                   /* an activation: per-tensor parameters */
      if (t->zp < -128 || t->zp > 127) REFUSE("tensor %d: zero point is %d, expected -128..127", i, t->zp);
      out->scale_bits[i] = rd_u32(data + t->soff);
      out->zero_point[i] = (int16_t)t->zp;
    } else if (t->zp != 0) {
      REFUSE("tensor %d: zero point is %d, expected 0 (filters and biases are symmetric)", i, t->zp);
    }
  }

  /* ---- the graph: SURVEY.md Appendix A, op by op ---- */
  static const char* const op_field[] = {"opcode", "inputs[0]", "inputs[1]", "inputs[2]", "output", "padding", "stride_w", "stride_h", "filter_w",
                                         "filter_h", "depth_multiplier", "axis"};
  for (int i = 0; i < YF_GRAPH_N_OPS; ++i) {
    const uint8_t* p = orecs + (size_t)OREC * i;
    const yf_graph_op* g = &yf_graph_ops[i];
    const int64_t want[12] = {g->opcode, g->ins[0], g->ins[1], g->ins[2], g->out, g->padding, g->stride_w, g->stride_h, g->filter_w, g->filter_h,
                              g->depth_multiplier, g->axis};
    for (int k = 0; k < 12; ++k) {
      const int64_t have = k == 0 ? (int64_t)rd_u32(p) : (int64_t)rd_i32(p + 4 * k);
      if (have != want[k]) REFUSE("op %d: %s is %lld, expected %lld", i, op_field[k], (long long)have, (long long)want[k]);
    }
    const uint32_t alpha = rd_u32(p + 48);
    if (alpha != g->alpha_bits) REFUSE("op %d: alpha has bits 0x%08x, expected 0x%08x", i, alpha, g->alpha_bits);
  }
  {
    const trec* t = &T[YF_GRAPH_PAD_TENSOR];            /* dbytes was checked against the expected shape */
    for (size_t k = 0; k < sizeof yf_graph_paddings / 4; ++k) {
      const int32_t v = rd_i32(data + t->doff + 4 * k);
      if (v != yf_graph_paddings[k]) REFUSE("tensor %d: paddings[%zu] is %d, expected %d", YF_GRAPH_PAD_TENSOR, k, v, yf_graph_paddings[k]);
    }
  }

  /* ---- the quantisation the frame producers assume ---- */
  if (out->scale_bits[YF_GRAPH_INPUT] != YF_MODEL_INPUT_SCALE_BITS)
    REFUSE("tensor %d (input): scale has bits 0x%08x, expected 0x%08x (frames are pixel - 128 in units of 1/255)", YF_GRAPH_INPUT,
           out->scale_bits[YF_GRAPH_INPUT], YF_MODEL_INPUT_SCALE_BITS);
  if (out->zero_point[YF_GRAPH_INPUT] != YF_MODEL_INPUT_ZERO_POINT)
    REFUSE("tensor %d (input): zero point is %d, expected %d (frames are pixel - 128)", YF_GRAPH_INPUT, out->zero_point[YF_GRAPH_INPUT],
           YF_MODEL_INPUT_ZERO_POINT);

  /* ---- the converter's constraints the table builder relies on ---- */
  for (int i = 0; i < YF_GRAPH_N_OPS; ++i) {
    const yf_graph_op* g = &yf_graph_ops[i];
    if (g->opcode == OP_PAD || g->opcode == OP_MAXPOOL) {
      if (!same_quant(out, g->ins[0], g->out))
        REFUSE("op %d (%s): output tensor %d has scale bits 0x%08x, zero point %d, expected its input's (tensor %d): 0x%08x, %d", i,
               g->opcode == OP_PAD ? "PAD" : "MAX_POOL_2D", g->out, out->scale_bits[g->out], out->zero_point[g->out], g->ins[0],
               out->scale_bits[g->ins[0]], out->zero_point[g->ins[0]]);
    } else if (g->opcode == OP_CONCAT) {
      for (int k = 0; k < 2; ++k)
        if (!same_quant(out, g->ins[k], g->out))
          REFUSE("op %d (CONCATENATION): input tensor %d has scale bits 0x%08x, zero point %d, expected the output's (tensor %d): 0x%08x, %d", i,
                 g->ins[k], out->scale_bits[g->ins[k]], out->zero_point[g->ins[k]], g->out, out->scale_bits[g->out], out->zero_point[g->out]);
    }
  }

  /* ---- convolutions: filter scales, and weights and biases into the ST layout ---- */
  for (int c = 0; c < YF_N_CONVS; ++c) {
    const yf_conv_desc* d = &yf_convs[c];
    const yf_graph_op* g = &yf_graph_ops[d->tfl_op];
    const int tw = g->ins[1], tb = g->ins[2];
    const trec* w = &T[tw];
    const trec* bs = &T[tb];
    if ((int)w->ns != d->cout || (int)bs->ns != d->cout || d->cout > YF_MODEL_MAX_COUT)       /* (the graph tables say so: defensive) */
      REFUSE("op %d: filter / bias carry %u / %u scales, expected %d", d->tfl_op, w->ns, bs->ns, d->cout);
    if ((size_t)d->w_off + w->dbytes > YF_WEIGHTS_BLOB_BYTES || (size_t)d->b_off + bs->dbytes > YF_WEIGHTS_BLOB_BYTES || bs->dbytes != 4u * d->cout)
      REFUSE("op %d: filter (%u bytes) or bias (%u bytes) does not fit its place in the weight layout", d->tfl_op, w->dbytes, bs->dbytes);
    float s_in;
    memcpy(&s_in, &out->scale_bits[g->ins[0]], 4);
    for (int ch = 0; ch < d->cout; ++ch) {
      const uint32_t wb = rd_u32(data + w->soff + 4 * (size_t)ch), bb = rd_u32(data + bs->soff + 4 * (size_t)ch);
      float s_w;
      memcpy(&s_w, &wb, 4);
      const volatile float p32 = s_in * s_w;                       /* the product as float32 arithmetic gives it ... */
      const float p64 = (float)((double)s_in * (double)s_w);       /* ... or rounded once from the double product (the converter's) */
      const float pa = p32;
      uint32_t a, e;
      memcpy(&a, &pa, 4); memcpy(&e, &p64, 4);
      if (bb != a && bb != e)
        REFUSE("op %d: bias scale[%d] has bits 0x%08x, expected 0x%08x (s_in * s_w[%d])", d->tfl_op, ch, bb, e, ch);
      out->wscale_bits[c][ch] = wb;
    }
    out->wscale[c].bits = out->wscale_bits[c];
    out->wscale[c].count = d->cout;
    memcpy(out->weights + d->w_off, data + w->doff, w->dbytes);
    memcpy(out->weights + d->b_off, data + bs->doff, bs->dbytes);
  }
  out->model.scale_bits = out->scale_bits;
  out->model.zero_point = out->zero_point;
  out->model.n_tensors = YF_N_TENSORS;
  out->model.wscale = out->wscale;
  out->model.n_convs = YF_N_CONVS;
  out->out_scale_bits = out->scale_bits[YF_GRAPH_OUTPUT];
  out->out_zero_point = out->zero_point[YF_GRAPH_OUTPUT];
  return 0;
}

void yf_model_decode_tables(uint32_t out_scale_bits, int32_t out_zero_point, uint32_t sig_bits[256], uint32_t exp_bits[256]) {
  float s;
  memcpy(&s, &out_scale_bits, 4);
  for (int q = -128; q < 128; ++q) {
    const volatile float d = (float)(q - out_zero_point);          /* exact: |q - zp| <= 255 */
    const volatile float x = d * s;
    const float sig = yfi_sigmoid_f32(x), ex = yfi_exp_f32(x);
    memcpy(&sig_bits[q + 128], &sig, 4);
    memcpy(&exp_bits[q + 128], &ex, 4);
  }
}
