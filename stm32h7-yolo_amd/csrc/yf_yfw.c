/* Parser of a .yfw float model (yf_yfw.h).  The bytes are UNTRUSTED: every record is read with memcpy at an offset that was checked against
 * the size first, in 64-bit arithmetic.  The file must then BE this network: the convolutions of gen/yf_graph_gen.h in order, each with the
 * graph's depthwise flag, channels, kernel and stride, and every weight and bias finite.  tests/csrc/yfw_sanitize_main.c runs it alone under
 * ASan + UBSan. */
#include "yf_yfw.h"
#include "gen/yf_graph_gen.h"
#include <stdio.h>
#include <string.h>

enum { HDR = 8, CREC = 24, OP_CONV = 3, OP_DWCONV = 4 };

static uint32_t rd_u32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }

#define REFUSE(...) do { if (err && errlen) snprintf(err, errlen, __VA_ARGS__); return 1; } while (0)

int yf_yfw_parse(const void* yfw, size_t bytes, float* out, char* err, size_t errlen) {
  if (!yfw || !out) REFUSE("float model: NULL argument");
  const uint8_t* b = (const uint8_t*)yfw;
  if (bytes < HDR) REFUSE("float model: %zu bytes, shorter than the 8-byte header", bytes);
  if (memcmp(b, "YFW1", 4) != 0) REFUSE("float model: magic is %02x %02x %02x %02x, expected 'YFW1'", b[0], b[1], b[2], b[3]);
  const uint32_t n = rd_u32(b + 4);
  if (n != YF_YFW_N_CONVS) REFUSE("float model: %u convs, expected %d", n, YF_YFW_N_CONVS);
  uint64_t at = HDR;
  size_t filled = 0;
  int conv = 0;
  for (int i = 0; i < YF_GRAPH_N_OPS; ++i) {
    const yf_graph_op* g = &yf_graph_ops[i];
    if (g->opcode != OP_CONV && g->opcode != OP_DWCONV) continue;
    const int32_t* fs = yf_graph_tensors[g->ins[1]].shape;
    const int dw = g->opcode == OP_DWCONV;
    const uint32_t cout = (uint32_t)(dw ? fs[3] : fs[0]), cin = (uint32_t)fs[3], k = (uint32_t)fs[1];
    const uint32_t want[6] = {(uint32_t)dw, cin, cout, k, (uint32_t)g->stride_w, (uint32_t)(fs[0] * fs[1] * fs[2] * fs[3])};
    static const char* const field[6] = {"depthwise", "cin", "cout", "k", "stride", "n_weights"};
    if (at + CREC > (uint64_t)bytes)
      REFUSE("conv %d: its record at byte %llu ends past the %zu bytes of the file", conv, (unsigned long long)at, bytes);
    for (int f = 0; f < 6; ++f) {
      const uint32_t have = rd_u32(b + at + 4 * (size_t)f);
      if (have != want[f]) REFUSE("conv %d: %s is %u, expected %u", conv, field[f], have, want[f]);
    }
    at += CREC;
    const uint64_t floats = (uint64_t)want[5] + cout;
    if (at + 4 * floats > (uint64_t)bytes)
      REFUSE("conv %d: %u weights and %u biases at byte %llu end past the %zu bytes of the file", conv, want[5], cout, (unsigned long long)at, bytes);
    if (filled + floats > YF_YFW_FLOATS) REFUSE("conv %d: more weights and biases than the graph has", conv);          /* (defensive) */
    for (uint64_t j = 0; j < floats; ++j) {
      const uint32_t bits = rd_u32(b + at + 4 * (size_t)j);
      if ((bits & 0x7F800000u) == 0x7F800000u) {
        if (j < want[5]) REFUSE("conv %d: weight %llu has bits 0x%08x, expected a finite float32", conv, (unsigned long long)j, bits);
        REFUSE("conv %d: bias %llu has bits 0x%08x, expected a finite float32", conv, (unsigned long long)(j - want[5]), bits);
      }
      memcpy(&out[filled + j], &bits, 4);
    }
    filled += (size_t)floats;
    at += 4 * floats;
    ++conv;
  }
  if (conv != YF_YFW_N_CONVS || filled != YF_YFW_FLOATS) REFUSE("float model: the graph gives %d convs and %zu floats", conv, filled);   /* (defensive) */
  if (at != (uint64_t)bytes) REFUSE("float model: %zu bytes, the convs' counts give %llu", bytes, (unsigned long long)at);
  return 0;
}
