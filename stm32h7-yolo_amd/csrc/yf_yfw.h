/* Parser of a .yfw float model (what tools/gen_fp16_model.py writes and model_file.write_yfw packs), for the calibration library: plain C, no HIP,
 * no allocation.  Layout (little endian): 'YFW1', u32 n_conv, then per convolution in graph order
 *   u32 depthwise, cin, cout, k, stride, n_weights ; f32 weights (dense OHWI, depthwise HWC) ; f32 bias[cout]. */
#ifndef YF_YFW_H
#define YF_YFW_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { YF_YFW_N_CONVS = 24, YF_YFW_N_WEIGHTS = 9126, YF_YFW_N_BIASES = 544, YF_YFW_FLOATS = 9126 + 544 };

/* Checks the untrusted bytes against the graph (gen/yf_graph_gen.h) and copies every convolution's weights, then its bias, to `out`
 * (YF_YFW_FLOATS floats, file order).  Returns 0, or 1 with a text in err that names the convolution, the field, the value found and the
 * value expected. */
int yf_yfw_parse(const void* yfw, size_t bytes, float* out, char* err, size_t errlen);

#ifdef __cplusplus
}
#endif
#endif /* YF_YFW_H */
