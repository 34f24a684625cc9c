/* The .yfw parser (csrc/yf_yfw.c) alone under ASan + UBSan: the malformed images of tests/test_calib_host.py and many more, each in a heap
 * block of exactly its size, so that a read past the end is a report.  argv[1]: a valid .yfw.  Prints "float model: ok ..." and exits 0 when the
 * valid image is admitted, every other one is refused with a text, and the sanitizers had nothing to say. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../stm32h7-yolo_amd/csrc/yf_yfw.h"

static float out[YF_YFW_FLOATS];
static long refused;

static int parse_exact(const uint8_t* img, size_t n, char* err, size_t errlen) {
  if (!img) { err[0] = 0; return yf_yfw_parse(NULL, 0, out, err, errlen); }
  uint8_t* block = (uint8_t*)malloc(n ? n : 1);
  if (!block) { fprintf(stderr, "out of memory\n"); exit(2); }
  memcpy(block, img, n);
  err[0] = 0;
  const int rc = yf_yfw_parse(block, n, out, err, errlen);
  free(block);
  return rc;
}

static void must_refuse(const uint8_t* img, size_t n, const char* what, const char* needle) {
  char err[256];
  if (parse_exact(img, n, err, sizeof err) == 0 || !err[0] || (needle && !strstr(err, needle))) {
    fprintf(stderr, "%s: not refused as expected (text: '%s', wanted '%s')\n", what, err, needle ? needle : "any");
    exit(1);
  }
  ++refused;
}

static void put_u32(uint8_t* p, uint32_t v) { memcpy(p, &v, 4); }
static uint32_t get_u32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s model.yfw\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  fseek(f, 0, SEEK_END);
  const long size = ftell(f);
  fseek(f, 0, SEEK_SET);
  uint8_t* good = (uint8_t*)malloc((size_t)size + 8);
  uint8_t* bad = (uint8_t*)malloc((size_t)size + 8);
  if (!good || !bad || fread(good, 1, (size_t)size, f) != (size_t)size) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  fclose(f);
  const size_t n = (size_t)size;
  char err[256];
  if (parse_exact(good, n, err, sizeof err) != 0) { fprintf(stderr, "the valid image was refused: %s\n", err); return 1; }

  /* every truncation of the first two records, then one in 61 */
  for (size_t k = 0; k < n; k += (k < 400 ? 1 : 61)) must_refuse(good, k, "truncation", NULL);
  must_refuse(good, n - 1, "truncation by one byte", "end past");
  memcpy(bad, good, n); memset(bad + n, 0, 4);
  must_refuse(bad, n + 4, "trailing bytes", "the convs' counts give");
  memcpy(bad, good, n); bad[3] = '2';
  must_refuse(bad, n, "magic", "magic is 59 46 57 32, expected 'YFW1'");
  memcpy(bad, good, n); put_u32(bad + 4, 23);
  must_refuse(bad, n, "23 convs", "23 convs, expected 24");

  /* every field of every record: extreme values, and the neighbour's value (a swapped cin / cout) */
  static const uint32_t extreme[] = {0u, 1u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu, 0x3FFFFFFFu, 0x40000000u};
  size_t at = 8;
  for (int c = 0; c < YF_YFW_N_CONVS; ++c) {
    const uint32_t cout = get_u32(good + at + 8), nw = get_u32(good + at + 20);
    for (int fld = 0; fld < 6; ++fld) {
      const uint32_t have = get_u32(good + at + 4 * (size_t)fld);
      for (size_t e = 0; e < sizeof extreme / sizeof extreme[0]; ++e) {
        if (extreme[e] == have) continue;
        memcpy(bad, good, n); put_u32(bad + at + 4 * (size_t)fld, extreme[e]);
        snprintf(err, sizeof err, "conv %d:", c);
        must_refuse(bad, n, "a record field at an extreme", err);
      }
    }
    const uint32_t cin = get_u32(good + at + 4);
    if (cin != cout) {
      memcpy(bad, good, n); put_u32(bad + at + 4, cout); put_u32(bad + at + 8, cin);
      snprintf(err, sizeof err, "conv %d: cin is %u, expected %u", c, cout, cin);
      must_refuse(bad, n, "swapped cin and cout", err);
    }
    /* a NaN in the first and the last weight, an infinity in the first and the last bias */
    const size_t w0 = at + 24, b0 = w0 + 4 * (size_t)nw;
    const size_t spots[4] = {w0, b0 - 4, b0, b0 + 4 * ((size_t)cout - 1)};
    const uint32_t specials[4] = {0x7FC00000u, 0xFFC00001u, 0x7F800000u, 0xFF800000u};
    for (int k = 0; k < 4; ++k) {
      memcpy(bad, good, n); put_u32(bad + spots[k], specials[k]);
      snprintf(err, sizeof err, "conv %d: %s", c, k < 2 ? "weight" : "bias");
      must_refuse(bad, n, "a weight or bias that is not finite", err);
    }
    at = b0 + 4 * (size_t)cout;
  }
  if (at != n) { fprintf(stderr, "the walk over the records ended at %zu of %zu bytes\n", at, n); return 1; }
  must_refuse(NULL, 0, "NULL image", "NULL");
  free(good);
  free(bad);
  printf("float model: ok, the valid image admitted and %ld malformed images refused\n", refused);
  return 0;
}
