/* E(x), the float32 nearest to e^x, and the sigmoid built on it -- shared by the companion library's float32 decode (yf_images_float.h: device
 * kernels and a host build) and by the network library's host layer, which builds the decode tables of a model file's output quantisation from
 * it (yf_model_file.c, yf_model_decode_tables).  Listed among the sources of BOTH libraries (Makefile IMAGES_SRCS, flags.mk HOST_SRCS): a change
 * here changes both ids.
 *
 * E is obtained by evaluating in float64 and rounding once -- THE LIBRARY'S CHOICE, in both uses.  numpy's own float32 exp, which the reference's
 * scripts call, is not that: it differs from it by up to 2 ulp on a large share of arguments, and which ones depends on the numpy build and the
 * CPU, so the scripts' literal answer is not one answer (yf_images_float.h has the figures for the float decode).  For the int8 decode the
 * shipped tables (gen/yf_decode_tables_gen.h: one numpy's answer for the shipped output quantisation) stay the contract; the tables of any OTHER
 * output quantisation, which no reference run ever produced, are built from E: x = fl32(fl32(q - zp) * s), sigmoid = 1.0f / (1.0f + E(-x)),
 * exp = E(x).  Built that way for the shipped quantisation they would differ from the shipped tables in 124 of 512 entries
 * (tests/test_model_file_host.py prints the figure).
 * E is written from IEEE basic operations only, so every build agrees by construction; compile without contraction (-ffp-contract=off; the
 * pragmas below say so again for clang). */
#ifndef YF_EXP_F32_H
#define YF_EXP_F32_H
#include <stdint.h>
#include <string.h>
#ifndef YFI_HD
#ifdef __HIPCC__
#define YFI_HD __host__ __device__ __forceinline__
#else
#define YFI_HD static inline
#endif
#endif

YFI_HD float yfi_f32_of_bits(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}

YFI_HD double yfi_f64_of_bits(uint64_t u) {
  double d;
  memcpy(&d, &u, 8);
  return d;
}

/* E(x): the float32 nearest to the float64 value of e^x */
YFI_HD float yfi_exp_f32(float xf) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  if (xf != xf) return xf;
  if (xf > 89.0f) return yfi_f32_of_bits(0x7F800000u);          /* e^89 > 2^128: +inf (and +inf itself) */
  if (xf < -104.0f) return 0.0f;                               /* e^-104 < 2^-150: 0 (and -inf itself) */
  const double x = (double)xf;
  /* k = the integer nearest to x / ln 2 (|k| <= 151); r = x - k ln 2 in two parts, |r| <= 0.3466 + rounding.  LN2_HI has 32 significant
   * bits, so k * LN2_HI is exact */
  const double t = x * 1.44269504088896338700e+00;
  const int k = (int)(t + (t < 0.0 ? -0.5 : 0.5));
  const double kd = (double)k;
  const double r = (x - kd * 6.93147180369123816490e-01) - kd * 1.90821492927058770002e-10;
  /* e^r = sum r^j / j!, j <= 13: the first term left out is below 5e-18 */
  double p = 1.0 / 6227020800.0;
  p = p * r + 1.0 / 479001600.0;
  p = p * r + 1.0 / 39916800.0;
  p = p * r + 1.0 / 3628800.0;
  p = p * r + 1.0 / 362880.0;
  p = p * r + 1.0 / 40320.0;
  p = p * r + 1.0 / 5040.0;
  p = p * r + 1.0 / 720.0;
  p = p * r + 1.0 / 120.0;
  p = p * r + 1.0 / 24.0;
  p = p * r + 1.0 / 6.0;
  p = p * r + 0.5;
  p = p * r + 1.0;
  p = p * r + 1.0;
  double y = p * yfi_f64_of_bits((uint64_t)(k + 1023) << 52);  /* 2^k, a normal double: exact scaling */
  /* below 2^-126 the float32 is subnormal, a multiple of 2^-149: round y to one here (adding 1.5 x 2^-97 leaves a double whose last
   * place is 2^-149, ties to even), so that the conversion below is exact whatever the converting instruction does with subnormals */
  if (y < 0x1p-126) y = (y + 0x1.8p-97) - 0x1.8p-97;
  return (float)y;
}

YFI_HD float yfi_sigmoid_f32(float x) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  return 1.0f / (1.0f + yfi_exp_f32(-x));
}

#endif
