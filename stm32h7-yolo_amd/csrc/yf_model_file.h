/* A .yfm model image (layout: stm32h7-yolo_amd/model_file.py; tools/gen_model.py writes one from a .tflite, the oracle reads the same bytes)
 * -> what yf_network_init_model needs: the quantisation of every tensor (yf_model, yf_host_prep.h), the weights and biases in the 11304-byte ST
 * layout, and the output tensor's parameters for the decode tables.  Plain C, no HIP: see yf_model_file.c. */
#ifndef YF_MODEL_FILE_H
#define YF_MODEL_FILE_H
#include <stddef.h>
#include <stdint.h>
#include "yf_host_prep.h"
#include "gen/yf_model_gen.h"
#ifdef __cplusplus
extern "C" {
#endif

#define YF_MODEL_INPUT_SCALE_BITS 0x3b808081u   /* 1/255 as the converter stores it: the frame producers write pixel - 128 */
#define YF_MODEL_INPUT_ZERO_POINT (-128)
#define YF_MODEL_MAX_COUT 40

typedef struct {
  yf_model model;                                      /* points into the arrays below: a yf_model_file must not be copied */
  uint32_t scale_bits[YF_N_TENSORS];
  int16_t  zero_point[YF_N_TENSORS];
  yf_wscale wscale[YF_N_CONVS];
  uint32_t wscale_bits[YF_N_CONVS][YF_MODEL_MAX_COUT];
  uint8_t  weights[YF_WEIGHTS_BLOB_BYTES];             /* the model's weights and biases at the offsets of yf_convs[] (zero between them) */
  uint32_t out_scale_bits;                             /* the output tensor's parameters: the decode tables are a function of these two */
  int32_t  out_zero_point;
} yf_model_file;

/* Parse and check `bytes` bytes at `yfm` (untrusted).  0 = accepted and *out filled; otherwise nothing in *out is meaningful and `err` (if given)
 * names the FIRST thing that is wrong: for a graph mismatch the op index, the field, the value found and the value expected.  Checked: magic,
 * counts and sizes; every scale / data range inside the data section; the number of scales (1 or the channels of the quantised dimension);
 * tensor types, shapes and which tensors are constants; the 54 ops of the network in order with their wiring, kernel sizes, strides, paddings and
 * the LeakyReLU alpha; the input quantisation (YF_MODEL_INPUT_*); and the converter's constraints the table builder relies on -- a PAD or
 * MAX_POOL_2D output carries its input's parameters, CONCATENATION inputs carry the output's, filter and bias zero points are 0, a bias scale is
 * s_in * s_w[c]. */
int yf_model_file_parse(const void* yfm, size_t bytes, yf_model_file* out, char* err, size_t errlen);

/* The shipped output quantisation, for which the shipped decode tables (gen/yf_decode_tables_gen.h) stay the contract */
#define YF_MODEL_SHIPPED_OUT_SCALE_BITS 0x3e11987eu
#define YF_MODEL_SHIPPED_OUT_ZERO_POINT (-15)
/* The decode tables of any other output quantisation, index q + 128 for q = -128..127, one IEEE float32 operation per numpy operation of
 * yoloface/tflite/tflite_prediction.py:42,53-55:  x = fl32(fl32(q - zp) * s),  sig = 1.0f / (1.0f + E(-x)),  exp = E(x),  E = yfi_exp_f32
 * (yf_exp_f32.h), the correctly rounded float32 exponential: the library's choice, as that header says. */
void yf_model_decode_tables(uint32_t out_scale_bits, int32_t out_zero_point, uint32_t sig_bits[256], uint32_t exp_bits[256]);

#ifdef __cplusplus
}
#endif
#endif
