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
 * stream order, so two calls on different streams need an event between them (or yf_calib_ranges, which synchronises the device).
 *
 * Two forms of every evaluation.  The entries without _hw take the network's 56x56 frames and keep a frame's activations in the CU's LDS.
 * The _hw entries take frames of h x w, h and w each a multiple of 8 from 8 to YF_CALIB_MAX_SIDE (160x160 is the engine's other size), and
 * keep the activations in a slab of global memory the handle owns, one slab per workgroup in flight; they compute the same arithmetic, and
 * at (56, 56) the same bits.  The handle orders the launches that share its slabs itself (see yf_calib_observe_hw_device). */
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

#define YF_CALIB_MAX_SIDE 160          /* the _hw entries: h and w are multiples of 8 from 8 to this */
#define YF_CALIB_ARENA_FLOATS_PER_CELL 800   /* a slab of the _hw entries: this many floats per cell, cells = (h / 8) * (w / 8) */

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

/* ---- Quantisation error per tensor: an int8 run of the network against the float32 evaluation of the same frames (csrc/yf_calib_compare.h,
 * DESIGN.md "Comparison arithmetic").  An entry names one of the 46 tensors the evaluation produces (the tensors of yf_calib_ranges without
 * the input) and where some int8 run left its values: unpadded NHWC bytes, frame f's at q + f * frame_stride, with the scale and zero point
 * that give them a real value.  yf_network_run_device_dump writes such tensors (yf_network_dump_offset), and the heads are tensor 100. */
typedef struct {
  int32_t tensor, zero_point;
  float scale;
  uint32_t reserved;
  const void* q;        /* frame 0's first byte of this tensor */
  size_t frame_stride;
} yf_calib_qtensor;

#define YF_CALIB_FRAME_STATS_BYTES 32 /* {double sum_err, sum_sq_err, sum_sq_ref; float max_abs_err; int32_t saturated}: error = dequantised - float */
#define YF_CALIB_TOTALS_BYTES 48      /* {double sum_err, sum_sq_err, sum_sq_ref; float max_abs_err; uint32_t reserved; int64_t saturated, elements} */

/* Evaluates d_frames int8 [n][56][56][3] and compares every listed tensor with its int8 values (device memory): one record per frame and
 * entry to d_frame_stats [n][count], and, unless d_totals is NULL, the sums over the frames in ascending order to d_totals [count].
 * Asynchronous on `stream`; `entries` is host memory and is not referenced after the call returns.  Touches neither the handle's ranges nor
 * yf_calib_frames_observed.  Returns n, or a value <= 0 after a failure: yf_calib_last_error_text() then names the entry index, the field,
 * the value found and the value expected (a tensor outside the 46 or listed twice, a scale that is not finite and positive, a zero point
 * outside -128..127, a NULL q, frame_stride below the tensor's elements, count outside 1..46, n < 1). */
YF_CALIB_API long yf_calib_compare_device(yf_calib* c, const void* d_frames, long n, const yf_calib_qtensor* entries, int count,
                                          void* d_frame_stats, void* d_totals, void* stream);

/* ---- Histograms of the 47 tensors over calibration frames, for clipped ranges (csrc/yf_calib_hist.h, DESIGN.md "Histogram arithmetic";
 * ptq.clip_ranges chooses a range from them by percentile or by least modelled error).  A second pass over the frames: the same float32
 * evaluation as yf_calib_observe_device, with every value of the input and of every convolution, LeakyReLU, ADD and pool output counted in
 * one of `bins` equal bins of its tensor's axis.  Row r of minmax (host memory, float [YF_CALIB_N_RANGES][2], the slot order and tensor ids
 * of yf_calib_ranges, whose output it usually is) gives tensor r's axis: a value outside {min, max} is counted in an end bin, v == max in
 * the last bin, a NaN in bin 0.  minmax is read during the call only: the axes travel to the kernel as a launch argument, by value.
 * d_counts uint64 [YF_CALIB_N_RANGES][bins] (device memory, 8-byte aligned) is ADDED to: the caller zeroes it once and may call again with
 * more frames, on the same axes.  Asynchronous on `stream`; allocates nothing and does not synchronise the host.  Touches neither the
 * handle's ranges nor yf_calib_frames_observed.  Counts are integers: the result equals the host build's exactly, whatever the grid.
 * Returns n, or a value <= 0 with nothing launched: yf_calib_last_error_text() then names what was refused (a NULL handle, d_frames, minmax
 * or d_counts, n < 1, bins outside 1..YF_CALIB_HIST_MAX_BINS, or the tensor id of a row that is not finite or has max < min). */
#define YF_CALIB_HIST_MAX_BINS 4096
YF_CALIB_API long yf_calib_histogram_device(yf_calib* c, const void* d_frames, long n, const float* minmax, int bins, uint64_t* d_counts,
                                            void* stream);

/* ---- Frames of h x w: the general form of the three evaluations above.  Argument lists and contracts are those of the 56x56 entries, with
 * d_frames int8 [n][h][w][3], d_logits float [n][h / 8][w / 8][18], and, in a compare entry, a tensor of elements * cells / 49 elements
 * (cells = (h / 8) * (w / 8)), which frame_stride is checked against.  These entries always run the general kernels, at (56, 56) too, where
 * their results equal the 56x56 entries' bit for bit.  Ranges and yf_calib_frames_observed accumulate across sizes and across both forms: a
 * range is the extremes of everything observed.  A refused size names h, w and the rule in yf_calib_last_error_text(), with nothing launched.
 *
 * SCRATCH.  A frame's activations live in a slab of YF_CALIB_ARENA_FLOATS_PER_CELL * cells floats of global memory (1.28 MB at 160x160),
 * one slab per workgroup of the launch: yf_calib_workgroups(c, h, w) slabs, a number fixed at yf_calib_create from an occupancy query.  The
 * handle owns the slabs and grows them when a call needs more than it has: THAT call synchronises the device and allocates -- the one place
 * where a general call may do either; a later call at the same or a smaller size does neither.
 * ORDER.  The slabs are shared by every general launch of the handle, so the library orders them: it records an event behind each general
 * launch and makes the next general launch's stream wait for it (on the same stream the wait is already satisfied).  Two _hw calls on different streams
 * therefore need nothing from the caller for the slabs' sake; what the caller still orders is what it always did -- the handle's ranges
 * between observing calls (above), and its own buffers.  Calls on one handle come from one thread at a time. */
YF_CALIB_API long yf_calib_observe_hw_device(yf_calib* c, int h, int w, const void* d_frames, long n, void* d_logits, void* stream);
YF_CALIB_API long yf_calib_compare_hw_device(yf_calib* c, int h, int w, const void* d_frames, long n, const yf_calib_qtensor* entries, int count,
                                             void* d_frame_stats, void* d_totals, void* stream);
YF_CALIB_API long yf_calib_histogram_hw_device(yf_calib* c, int h, int w, const void* d_frames, long n, const float* minmax, int bins,
                                               uint64_t* d_counts, void* stream);

/* The number of workgroups a general launch at (h, w) uses when n is at least that: the slab count.  A launch's scratch is this times
 * YF_CALIB_ARENA_FLOATS_PER_CELL * cells * 4 bytes.  <= 0 for a NULL handle or a refused size (yf_calib_last_error_text()). */
YF_CALIB_API int yf_calib_workgroups(const yf_calib* c, int h, int w);

/* The bytes of scratch the handle holds now (0 before the first general call). */
YF_CALIB_API size_t yf_calib_scratch_bytes(const yf_calib* c);

/* ---- Simulated quantisation: what ONE tensor's quantisation costs the logits (csrc/yf_calib_sim.h, DESIGN.md "Simulation arithmetic";
 * TFLite's quantisation debugger in its per-layer mode).  The float32 evaluation again, with every tensor whose entry is enabled put on its
 * int8 grid where it is produced: v -> clamp(rint(v / scale), -128 - zero_point, 127 - zero_point) * scale, in float32.  The table has
 * YF_CALIB_SIM_ENTRIES entries: 0 .. 46 are the range slots in the order of yf_calib_ranges (the input, every convolution, LeakyReLU, ADD
 * and pool output), 47 .. 49 the outputs of the graph's three QUANTIZE ops in ascending tensor id (101, 102, 103).  scale == 0: the tensor
 * stays float, and with every entry disabled the logits are yf_calib_observe_device's bit for bit.
 * d_frames int8 [n][56][56][3]; `table` is host memory, read during the call only (it travels to the kernel by value); d_logits float
 * [n][7][7][18] receives the simulated logits unless it is NULL.  With d_ref_logits (float [n][7][7][18], usually the logits of a call with
 * every entry disabled) the call also writes one record per frame to d_frame_stats [n] (YF_CALIB_FRAME_STATS_BYTES each: error = simulated -
 * reference over the frame's logits, `saturated` = the values of the frame that were clipped, over all enabled entries) and, unless d_totals
 * is NULL, their sums in ascending frame order to d_totals [1] (YF_CALIB_TOTALS_BYTES).  Without d_ref_logits both must be NULL.
 * Asynchronous on `stream`; touches neither the handle's ranges nor yf_calib_frames_observed.  Returns n, or a value <= 0 with nothing
 * launched: yf_calib_last_error_text() then names the entry point and what was refused (a NULL handle, frames or table; n < 1; frame_stats
 * or totals without ref_logits; ref_logits without frame_stats; a table entry, with its tensor id, whose scale is negative, NaN or infinite
 * or so small that its reciprocal is not a finite float32, or whose zero point is outside -128..127). */
#define YF_CALIB_SIM_ENTRIES 50
typedef struct { float scale; int32_t zero_point; } yf_calib_sim_entry;
YF_CALIB_API long yf_calib_simulate_device(yf_calib* c, const void* d_frames, long n, const yf_calib_sim_entry* table, const void* d_ref_logits,
                                           void* d_logits, void* d_frame_stats, void* d_totals, void* stream);
/* ... and at h x w: the general form, with the scratch and the ordering of the _hw entries above; at (56, 56) the same bits. */
YF_CALIB_API long yf_calib_simulate_hw_device(yf_calib* c, int h, int w, const void* d_frames, long n, const yf_calib_sim_entry* table,
                                              const void* d_ref_logits, void* d_logits, void* d_frame_stats, void* d_totals, void* stream);

/* ---- Per-channel sums of every convolution's raw output, for bias correction (csrc/yf_calib_chan.h, DESIGN.md "Channel-sum arithmetic";
 * calib.correct_biases folds the difference of the simulated and the float means into the biases).  The evaluation of
 * yf_calib_simulate_device again, under the same table: for every convolution, in file order, and every output channel of it the sum over
 * the frame's pixels of y = acc + bias, the float32 value BEFORE the convolution's own entry quantises it, added in double in the defined
 * order (chunks of 64 consecutive pixels, the halving of the comparison, the chunks in ascending order).  With every entry disabled these
 * are the sums of the float evaluation.  Channel first[k] + co belongs to channel co of convolution k (yf_calib_channel_layout);
 * YF_CALIB_CHANNELS in all.  Pools contribute nothing.
 * d_frames int8 [n][56][56][3]; `table` is host memory, read during the call only (it travels to the kernel by value); d_frame_sums double
 * [n][YF_CALIB_CHANNELS] (device memory, the caller's: 4352 bytes per frame) is OVERWRITTEN with one row per frame; d_sums double
 * [YF_CALIB_CHANNELS] receives the rows added in ascending frame order unless it is NULL; d_logits float [n][7][7][18] receives the logits
 * unless it is NULL: yf_calib_simulate_device's bits for the same table.  The result does not depend on the grid: device and host build agree
 * bit for bit.  Asynchronous on `stream`; allocates nothing and does not synchronise the host; touches neither the handle's ranges nor
 * yf_calib_frames_observed.  Returns n, or a value <= 0 with nothing launched: yf_calib_last_error_text() then names the entry point and what
 * was refused (a NULL handle, frames, table or frame_sums; n < 1; a table entry, in yf_calib_simulate_device's words). */
#define YF_CALIB_CHANNELS 544
#define YF_CALIB_N_CONVS 24
YF_CALIB_API long yf_calib_channel_sums_device(yf_calib* c, const void* d_frames, long n, const yf_calib_sim_entry* table, double* d_frame_sums,
                                               double* d_sums, void* d_logits, void* stream);
/* ... and at h x w: the general form, with the scratch and the ordering of the _hw entries above; at (56, 56) the same bits. */
YF_CALIB_API long yf_calib_channel_sums_hw_device(yf_calib* c, int h, int w, const void* d_frames, long n, const yf_calib_sim_entry* table,
                                                  double* d_frame_sums, double* d_sums, void* d_logits, void* stream);
/* The channels' layout (both libraries): first[k] and cout[k] of convolution k, and pixels56[k] = the pixels per frame of its output at 56x56
 * (at h x w: pixels56 * (h / 8) * (w / 8) / 49).  Returns YF_CALIB_CHANNELS, or <= 0 if an argument is NULL. */
YF_CALIB_API int yf_calib_channel_layout(int32_t first[YF_CALIB_N_CONVS], int32_t cout[YF_CALIB_N_CONVS], int32_t pixels56[YF_CALIB_N_CONVS]);

/* ---- libyf_calib_host.so only: the same evaluation on host arrays, on `threads` threads.  minmax / tensors as yf_calib_ranges fills them
 * (the ranges of these n frames alone), logits float [n][7][7][18] or NULL.  Returns n, or <= 0 with a text in err. */
YF_CALIB_API long yf_calib_host_run(const void* yfw, size_t bytes, const int8_t* frames, long n, float* minmax, int32_t* tensors,
                                    float* logits, int threads, char* err, size_t errlen);

/* ... and the same comparison: q of every entry is a host pointer, frame_stats [n][count] and totals [count] (or NULL) host arrays.  If
 * tensors_out is not NULL it receives the float32 tensors of the listed entries, [n][elements] per entry, concatenated in entry order. */
YF_CALIB_API long yf_calib_host_compare(const void* yfw, size_t bytes, const int8_t* frames, long n, const yf_calib_qtensor* entries, int count,
                                        void* frame_stats, void* totals, float* tensors_out, int threads, char* err, size_t errlen);

/* ... and the same histograms: counts uint64 [YF_CALIB_N_RANGES][bins] (host memory) is added to.  The arguments are checked as
 * yf_calib_histogram_device checks them. */
YF_CALIB_API long yf_calib_host_histogram(const void* yfw, size_t bytes, const int8_t* frames, long n, const float* minmax, int bins,
                                          uint64_t* counts, int threads, char* err, size_t errlen);

/* ... and the three at h x w (the three above are these at (56, 56)): frames int8 [n][h][w][3], logits float [n][h / 8][w / 8][18], a compare
 * entry's tensor elements * cells / 49 elements.  A refused size is named in err, and nothing is written to the outputs. */
YF_CALIB_API long yf_calib_host_run_hw(const void* yfw, size_t bytes, int h, int w, const int8_t* frames, long n, float* minmax, int32_t* tensors,
                                       float* logits, int threads, char* err, size_t errlen);
YF_CALIB_API long yf_calib_host_compare_hw(const void* yfw, size_t bytes, int h, int w, const int8_t* frames, long n, const yf_calib_qtensor* entries,
                                           int count, void* frame_stats, void* totals, float* tensors_out, int threads, char* err, size_t errlen);
YF_CALIB_API long yf_calib_host_histogram_hw(const void* yfw, size_t bytes, int h, int w, const int8_t* frames, long n, const float* minmax, int bins,
                                             uint64_t* counts, int threads, char* err, size_t errlen);

/* ... and the simulation (yf_calib_simulate_device's arguments as host arrays), at 56x56 and at h x w: bit for bit what the device gives. */
YF_CALIB_API long yf_calib_host_simulate(const void* yfw, size_t bytes, const int8_t* frames, long n, const yf_calib_sim_entry* table,
                                         const float* ref_logits, float* logits, void* frame_stats, void* totals, int threads, char* err,
                                         size_t errlen);
YF_CALIB_API long yf_calib_host_simulate_hw(const void* yfw, size_t bytes, int h, int w, const int8_t* frames, long n,
                                            const yf_calib_sim_entry* table, const float* ref_logits, float* logits, void* frame_stats,
                                            void* totals, int threads, char* err, size_t errlen);

/* ... and the channel sums (yf_calib_channel_sums_device's arguments as host arrays), at 56x56 and at h x w: bit for bit what the device gives. */
YF_CALIB_API long yf_calib_host_channel_sums(const void* yfw, size_t bytes, const int8_t* frames, long n, const yf_calib_sim_entry* table,
                                             double* frame_sums, double* sums, float* logits, int threads, char* err, size_t errlen);
YF_CALIB_API long yf_calib_host_channel_sums_hw(const void* yfw, size_t bytes, int h, int w, const int8_t* frames, long n,
                                                const yf_calib_sim_entry* table, double* frame_sums, double* sums, float* logits, int threads,
                                                char* err, size_t errlen);

#ifdef __cplusplus
}
#endif
#endif /* YF_CALIB_H */
