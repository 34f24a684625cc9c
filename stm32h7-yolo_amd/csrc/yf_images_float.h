/* The float side of the image path: fp16 frames for the fp16 network (yf_network_fp16_run_device) and the decode of its float32 logits,
 * shared by the device kernels (yf_images.hip: prepare_f16_kernel, decode_f32_kernel) and a host build (yf_images_host.c,
 * libyf_images_host.so, which tests/test_images_float_host.py checks against numpy without a GPU).  Restated from the reference's float
 * caller, yoloface/tensorflow/h5_predition.py:29-73 (yoloface/pytorch/onnx_prediction.py:24-59 has the same front half).
 *
 * Frames.  frame[y][x][c] = fp16(R[y][x][rgb(c)] / 255.), R = cv2.resize(image, (56, 56)) as yf_images_taps.h computes it.  The script
 * divides in float64, the model casts to float32, the fp16 network to fp16; for the 256 bytes the routes float64 -> float32 -> fp16,
 * float32 division -> fp16 and float64 -> fp16 give the same 256 halves, so the conversion is a table: yfi_f16_of_u8, a float32 division
 * and a round-to-nearest-even to 11 bits in integer arithmetic.
 *
 * Decode of float32 logits t[row][col][a * 6 + k], h5_predition.py:51-72: one IEEE float32 operation per numpy operation, in the script's
 * order, no contraction (-ffp-contract=off; the pragmas below say so again for clang).
 *   sigmoid(x) = 1.0f / (1.0f + E(-x))
 *   E(x) = the float32 nearest to e^x, obtained by evaluating in float64 and rounding once -- THE LIBRARY'S CHOICE.  numpy's own float32
 *          exp is not that: it differs from it by up to 2 ulp on a large share of arguments, and which ones depends on the numpy build
 *          and the CPU (numpy documents no tighter bound), so the script's literal answer is not one answer.  E is written from IEEE
 *          basic operations only (Cody-Waite reduction by ln 2 in two parts, a degree-13 Taylor polynomial in float64 Horner form,
 *          scaling by a power of two built from its bits, one rounding to float32), so the host build and the kernel agree by
 *          construction, not by the luck of two math libraries.  The whole float32 domain: overflow to +inf, gradual underflow to
 *          subnormals and 0, E(-inf) = 0, E(+inf) = +inf, NaN -> NaN.
 *          Against the script run literally (numpy's float32 exp and sigmoid) on the logits of the 27 real frames of
 *          tests/golden/real_frames_56.bin at the 27 reference sizes: the same 47 candidates fire and 0 of the 188 edges differ
 *          (tests/test_images_float_host.py prints the figure; another numpy build may move an edge by 1).
 *   candidate i = (anchor * 7 + row) * 7 + col, i < 147, as reshape(7, 7, 3, 6).transpose(2, 0, 1, 3) orders them;
 *   conf = sigmoid(t_conf), kept iff conf > 0.7f (a NaN is not kept); cx = (sigmoid(tx) + col) * 8, cy = (sigmoid(ty) + row) * 8
 *   (grid[..., 0] is the column: np.meshgrid's default indexing); w = E(tw) * aw, h = E(th) * ah, anchors (9, 14), (12, 17), (22, 21);
 *   the edges, the scales and float32 -> int32 as YF_DECODE_PY: yfi_d160_box of yf_images_decode160.h.
 * The record is a yf_det as every other decode writes it; q_conf = 0: this network has no int8 logit. */
#ifndef YF_IMAGES_FLOAT_H
#define YF_IMAGES_FLOAT_H
#include <stdint.h>
#include <string.h>
#include "../../include/yf_images.h"
#include "yf_images_decode160.h"
#include "yf_exp_f32.h"                    /* E and the sigmoid built on it: yfi_exp_f32, yfi_sigmoid_f32 */

#define YFI_F32_CAND 147                   /* 3 anchors x 7 x 7 */
#define YFI_F32_LOGITS (7 * 7 * 18)        /* float32 values per frame */

/* the fp16 bits of v / 255., v in [0, 255] */
YFI_HD uint16_t yfi_f16_of_u8(int v) {
  const float f = (float)v / 255.0f;
  uint32_t u;
  memcpy(&u, &f, 4);
  if (u == 0) return 0;
  /* 1/255 <= f <= 1: a normal half.  Exponent rebias 127 -> 15, 23 -> 10 mantissa bits, ties to even; a carry runs into the exponent */
  uint32_t h = (((u >> 23) - 112u) << 10) | ((u & 0x7FFFFFu) >> 13);
  const uint32_t rem = u & 0x1FFFu;
  if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) ++h;
  return (uint16_t)h;
}

/* index in a frame's logits of candidate i's six values (x, y, w, h, conf, class) */
YFI_HD int yfi_f32_offset(int i) {
  const int a = i / 49;
  return (i - a * 49) * 18 + a * 6;
}

/* One record from candidate i (p = its six logits) of frame `frame`; conf = yfi_sigmoid_f32(p[4]), which the caller has computed to
 * decide that the candidate fires (conf > 0.7f). */
YFI_HD yf_det yfi_f32_candidate(const float* p, int i, int32_t frame, float conf, float w_scale, float h_scale) {
  const int a = i / 49, cell = i - a * 49;
  const int row = cell / 7, col = cell - row * 7;
  yf_det d;
  d.frame = frame; d.anchor = (uint8_t)a; d.row = (uint8_t)row; d.col = (uint8_t)col;
  d.q_conf = 0; d.conf = conf;
  yfi_d160_box(yfi_sigmoid_f32(p[0]), yfi_sigmoid_f32(p[1]), yfi_exp_f32(p[2]), yfi_exp_f32(p[3]), a, row, col, w_scale, h_scale, &d);
  return d;
}

#endif
