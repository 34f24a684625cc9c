/* libyf_calib.so: calibration of a FLOAT model of the network on the GPU -- the float32 evaluation of the 54-op graph over a batch of the
 * network's int8 frames, with the running minimum and maximum of every tensor that needs a quantisation range of its own.  With the
 * ranges, stm32h7-yolo_amd/ptq.py (quantize_model) turns the float weights into a .yfm image that yf_network_init_model admits:
 *
 *     retrained float weights -> .yfw -> yf_calib_create / yf_calib_observe_device / yf_calib_ranges -> ptq.quantize_model -> .yfm
 *
 * The library needs no network handle and shares no source with libyf_network.so.  The arithmetic is the one csrc/yf_calib_arith.h defines
 * (float32, one IEEE operation per stated operation, fixed summation order); libyf_calib_host.so is the same arithmetic compiled for the
 * host, and tests/test_calib_gpu.py requires the two to agree bit for bit.
 *
 * Calls on one handle are ordered by the caller: the launches of yf_calib_observe_device accumulate into the handle's device-side ranges in
 * stream order, so two calls on different streams need an event between them (or yf_calib_ranges, which synchronises the device). */
#ifndef YF_CALIB_H
#define YF_CALIB_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(_WIN32)
#define YF_CALIB_API
#else
#define YF_CALIB_API __attribute__((visibility("default")))
#endif

#define YF_CALIB_N_RANGES 47          /* the input, the output of every CONV_2D, DEPTHWISE_CONV_2D, LEAKY_RELU and ADD (45 tensors with a
                                         quantisation of their own) and of the two MAX_POOL_2D: a CONCATENATION's range is the union of its
                                         inputs' ranges, and the minimum of a max-pool is not its input's */
#define YF_CALIB_FRAME_BYTES 9408     /* int8 [56][56][3] */
#define YF_CALIB_LOGITS 882           /* float [7][7][18] */

typedef struct yf_calib yf_calib;

/* A calibration of the float model in `yfw` (.yfw bytes, untrusted: parsed and checked against the graph, every weight and bias finite) on
 * GPU `device`.  NULL on failure; yf_calib_last_error_text() then names the convolution, the field, the value found and the value expected. */
YF_CALIB_API yf_calib* yf_calib_create(const void* yfw, size_t bytes, int device);

/* Evaluates d_frames int8 [n][56][56][3] (device memory) and folds every tensor's extremes into the handle's ranges; writes the float32
 * logits float [n][7][7][18] to d_logits unless it is NULL.  Asynchronous on `stream` (a hipStream_t; NULL: the default stream).
 * Returns n, or a value <= 0 after a failure (n < 1 included). */
YF_CALIB_API long yf_calib_observe_device(yf_calib* c, const void* d_frames, long n, void* d_logits, void* stream);

/* Synchronises the device and returns the ranges so far: minmax[YF_CALIB_N_RANGES][2] = {minimum, maximum} and the tflite tensor id of each
 * row.  Returns YF_CALIB_N_RANGES, or <= 0: before any frame was observed there are no ranges. */
YF_CALIB_API int yf_calib_ranges(yf_calib* c, float* minmax, int32_t* tensors);

/* Forgets every frame observed so far.  Returns 0 or a negative value. */
YF_CALIB_API int yf_calib_reset(yf_calib* c);

/* The number of frames submitted since creation or the last reset. */
YF_CALIB_API long yf_calib_frames_observed(const yf_calib* c);

YF_CALIB_API void yf_calib_destroy(yf_calib* c);

/* The text of the last failure on the calling thread. */
YF_CALIB_API const char* yf_calib_last_error_text(void);

/* sha256 (16 hex digits) over the library's sources and flags, as csrc/Makefile computed it (calib.py recomputes it). */
YF_CALIB_API const char* yf_calib_build_id(void);

/* ---- libyf_calib_host.so only: the same evaluation on host arrays, on `threads` threads.  minmax / tensors as yf_calib_ranges fills them
 * (the ranges of these n frames alone), logits float [n][7][7][18] or NULL.  Returns n, or <= 0 with a text in err. */
YF_CALIB_API long yf_calib_host_run(const void* yfw, size_t bytes, const int8_t* frames, long n, float* minmax, int32_t* tensors,
                                    float* logits, int threads, char* err, size_t errlen);

#ifdef __cplusplus
}
#endif
#endif /* YF_CALIB_H */
