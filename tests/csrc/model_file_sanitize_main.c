/* AddressSanitizer + UndefinedBehaviorSanitizer run of the model-file parser (csrc/yf_model_file.c) ALONE: it faces untrusted bytes.
 * Built and run by tests/test_model_file_host.py:  prog <model.yfm>
 * Every image is handed over in a heap block of exactly its size, so a read past the end is a report.  Fed: the shipped image (accepted), every
 * truncation of it, the corruptions the Python test names (each must be refused with a text), and every 32-bit field of the header and of every
 * tensor and op record set to a handful of extreme values (refused or accepted, never a report).  Prints "model file: ok <refused> <accepted>". */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../stm32h7-yolo_amd/csrc/yf_model_file.h"

enum { HDR = 24, TREC = 44, OREC = 52, NT = 104, NO = 54 };
static long n_refused, n_accepted;
static yf_model_file g_mf;

/* parse a private copy of exactly `n` bytes; returns the parser's result, text in `err` */
static int feed(const uint8_t* img, size_t n, char* err, size_t errlen) {
  uint8_t* copy = malloc(n ? n : 1);
  if (!copy) exit(20);
  memcpy(copy, img, n);
  err[0] = 0;
  const int rc = yf_model_file_parse(copy, n, &g_mf, err, errlen);
  free(copy);
  if (rc) { ++n_refused; if (!err[0]) { fprintf(stderr, "refused without a text\n"); exit(21); } }
  else ++n_accepted;
  return rc;
}

static void put32(uint8_t* p, uint32_t v) { memcpy(p, &v, 4); }
static uint32_t get32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }

/* one field changed: must be refused, and the text must contain `want` */
static void must_refuse(const uint8_t* img, size_t n, size_t at, uint32_t v, const char* want) {
  uint8_t* m = malloc(n);
  char err[400];
  memcpy(m, img, n);
  put32(m + at, v);
  if (feed(m, n, err, sizeof err) == 0 || !strstr(err, want)) { fprintf(stderr, "offset %zu <- %u: expected a refusal with '%s', got '%s'\n", at, v, want, err); exit(22); }
  free(m);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  fseek(f, 0, SEEK_END);
  const long len = ftell(f);
  fseek(f, 0, SEEK_SET);
  uint8_t* img = malloc((size_t)len);
  if (!img || fread(img, 1, (size_t)len, f) != (size_t)len) return 4;
  fclose(f);
  char err[400];

  if (feed(img, (size_t)len, err, sizeof err) != 0) { fprintf(stderr, "shipped image refused: %s\n", err); return 5; }
  uint32_t sig[256], ex[256];
  yf_model_decode_tables(g_mf.out_scale_bits, g_mf.out_zero_point, sig, ex);
  yf_model_decode_tables(0x3e000000u, 127, sig, ex);
  yf_model_decode_tables(0x7f7fffffu, -128, sig, ex);          /* overflow to inf, underflow to 0: no undefined conversion */
  if (yf_model_file_parse(NULL, 10, &g_mf, err, sizeof err) == 0 || yf_model_file_parse(img, (size_t)len, NULL, err, sizeof err) == 0) return 6;
  if (yf_model_file_parse(img, 3, &g_mf, NULL, 0) == 0) return 7;                     /* no text wanted */

  for (long n = 0; n < len; n += (n < 8192 ? 1 : 61))                                  /* truncations: every length through the records, then a spread */
    if (feed(img, (size_t)n, err, sizeof err) == 0) { fprintf(stderr, "truncation to %ld bytes accepted\n", n); return 8; }

  const size_t ops = HDR + (size_t)TREC * NT, nd = get32(img + 20);
  must_refuse(img, (size_t)len, 0, 0x324d4659u, "magic");                               /* 'YFM2' */
  must_refuse(img, (size_t)len, HDR + TREC * 9 + 36, (uint32_t)nd - 10, "ends past the data section");   /* doff of the first filter */
  must_refuse(img, (size_t)len, HDR + TREC * 9 + 24, 3, "n_scales is 3, expected 1 or 8");
  must_refuse(img, (size_t)len, ops + OREC * 2, 114, "op 2: opcode is 114, expected 98");
  must_refuse(img, (size_t)len, ops + OREC * 10 + 24, 1, "op 10: stride_w is 1, expected 2");
  must_refuse(img, (size_t)len, ops + OREC * 18 + 8, 66, "op 18: inputs[1] is 66, expected 67");
  must_refuse(img, (size_t)len, ops + OREC * 2 + 48, 0x3e4ccccdu, "op 2: alpha has bits 0x3e4ccccd, expected 0x3dcccccd");
  must_refuse(img, (size_t)len, HDR + 20, (uint32_t)-127, "tensor 0 (input): zero point is -127, expected -128");
  must_refuse(img, (size_t)len, HDR + TREC * 58 + 20, get32(img + HDR + TREC * 58 + 20) + 1, "op 8 (MAX_POOL_2D): output tensor 58");

  static const uint32_t extreme[] = {0xFFFFFFFFu, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFF0u, 1u, 0u};
  uint8_t* m = malloc((size_t)len);
  for (size_t at = 4; at < ops + (size_t)OREC * NO; at += 4)
    for (size_t k = 0; k < sizeof extreme / sizeof extreme[0]; ++k) {
      memcpy(m, img, (size_t)len);
      put32(m + at, extreme[k]);
      (void)feed(m, (size_t)len, err, sizeof err);
    }
  free(m);
  free(img);
  printf("model file: ok %ld %ld\n", n_refused, n_accepted);
  return 0;
}
