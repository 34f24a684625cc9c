/* C-ABI of libyf_images.so -- decoded images of any size (packed BGR / RGB / BGRA / RGBA, or NV12 / NV21 decoder surfaces converted as
 * cv2.cvtColor does) to the network's int8 frames, resized as OpenCV's cv2.resize does (INTER_LINEAR, 11-bit fixed-point weights), and on
 * to detection records in each image's own pixels.
 *
 * This is the front half of the reference's Python caller (yoloface/tflite/tflite_prediction.py:29-37,56-61): imread (BGR), BGR -> RGB,
 * cv2.resize(img, (56, 56)), minus 128, int8; after the network, boxes scaled by W/56. and H/56.  The resize is bit-exact against
 * ptq.resize_linear_u8, a restatement of OpenCV 4's imgproc/resize.cpp that has not been pinned against a real cv2 (none is available
 * where this library is built), just as the oracle is not pinned against TFLite.
 *
 * The library links against libyf_network.so and reaches the network only through its public C-ABI (include/yf_network.h).
 *
 * Pointers prefixed d_ are device memory.  Every call is asynchronous on `stream` (a hipStream_t, NULL = default stream) on the calling
 * thread's current device (the run_* calls: the network's device), does no host synchronisation and no allocation, and can be captured in
 * a graph -- except that a decode of int8 heads whose 2 KB decode tables are not on the device yet uploads them first (synchronously; the rule
 * is at yf_images_set_decode_tables below): always the first such decode on a device, later ones only when the tables changed.
 * Return values follow include/yf_network.h: n on success, <= 0 on error; yf_images_last_error_text() says why (per thread).
 * d_frames must be 16-byte aligned. */
#ifndef YF_IMAGES_H
#define YF_IMAGES_H
#include <stddef.h>
#include <stdint.h>
#include "yf_network.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One image of a ragged batch: its first pixel at byte `offset` of the pixel buffer, rows `row_stride` bytes apart.  24 bytes. */
typedef struct yf_image {
  uint64_t offset;
  int32_t  height, width;
  int64_t  row_stride;
} yf_image;

/* Pixel formats (bytes per pixel 3, 3, 4, 4); the alpha byte is never read.  Frames come out in RGB order whatever the format. */
enum { YF_PIX_BGR8 = 0 /* cv2.imread */, YF_PIX_RGB8 = 1, YF_PIX_BGRA8 = 2, YF_PIX_RGBA8 = 3 };
/* 4:2:0 semi-planar surfaces, what hardware video and JPEG decoders write: a plane of Y bytes and, at half resolution both ways, a plane
 * of chroma byte pairs (NV12: U, V; NV21: V, U).  Only the yf_images_prepare_yuv_* entries below take them; every other entry refuses
 * them and says so.  Out of scope: packed 4:2:2 (YUYV, UYVY), three-plane I420, BT.709, full-range variants, odd-sided surfaces. */
enum { YF_PIX_NV12 = 4, YF_PIX_NV21 = 5 };

#define YF_IMAGES_MAX_SIDE 16384   /* 1 <= height, width <= this */

/* frame[y][x][c] = (int8)(R[y][x][rgb(c)] - 128), R = cv2.resize(image, (out_hw, out_hw)).  out_hw = 56 (the network's input) or 160
 * (frames for yf_network_run_device_hw; boxes at 160: the *160* entries below).  d_frames int8[n][out_hw][out_hw][3]. */

/* Uniform batch: n images of height x width, image i at d_pixels + i * frame_stride, rows row_stride bytes apart (a video, an [n,H,W,C]
 * tensor, or crops of one: row_stride >= width * C, frame_stride >= 0).  Every argument is checked before any launch; an image that
 * would reach outside [0, pixels_bytes) is an error. */
YF_API long yf_images_prepare_device(const void* d_pixels, size_t pixels_bytes, int format, int height, int width,
                                     long row_stride, long frame_stride, long n, int out_hw, void* d_frames, void* stream);
/* Ragged batch: one descriptor per image (d_images, device memory).  The kernel checks each descriptor (1 <= h, w <= 16384,
 * row_stride >= w * C, offset + (h - 1) * row_stride + w * C <= pixels_bytes): d_status[i] = 0 for a valid image, 1 for an invalid one,
 * which is never read and whose frame is written as all -128.  No load touches a byte outside an image's own extent. */
YF_API long yf_images_prepare_ragged_device(const void* d_pixels, size_t pixels_bytes, int format, const yf_image* d_images, long n,
                                            int out_hw, void* d_frames, int32_t* d_status, void* stream);
/* ---- NV12 / NV21 surfaces -> the same frames.  frame = the frame of cv2.cvtColor(yuv, cv2.COLOR_YUV2BGR_NV12 / _NV21) under the BGR
 * path above, bit for bit: each of the four source pixels an output pixel samples is converted first (integer BT.601 limited range, the
 * constants and the clamp of OpenCV 4's color_yuv.simd.hpp, stated once in csrc/yf_images_yuv.h and restated as ptq.yuv420sp_to_rgb_u8;
 * like the resize, not pinned against a real cv2), then the bytes are interpolated.  Pixel (y, x) takes the chroma pair of UV row y >> 1
 * at byte columns 2 * (x >> 1), + 1; chroma is not interpolated.  The surface is read where it lies: no BGR copy is made.
 *   One surface of a ragged batch (40 bytes): height x width luma bytes, rows stride_y apart, first at offset_y; height / 2 rows of
 *   width chroma bytes, stride_uv apart, first at offset_uv.  Valid: height and width even and in [2, 16384] (cv2 refuses odd sides),
 *   stride_y >= width, stride_uv >= width, offset_y + (height - 1) * stride_y + width <= pixels_bytes and
 *   offset_uv + (height / 2 - 1) * stride_uv + width <= pixels_bytes.  No alignment is asked of offsets or strides; the planes may lie
 *   anywhere in the buffer, UV before Y included.  No load touches a byte outside a plane's extent as the descriptor states it. */
typedef struct yf_image_yuv {
  uint64_t offset_y, offset_uv;
  int32_t  height, width;
  int64_t  stride_y, stride_uv;
} yf_image_yuv;
/* format: YF_PIX_NV12 or YF_PIX_NV21.  Uniform: picture i's Y plane at d_pixels + i * frame_stride, its UV plane uv_offset bytes after
 * that (uv_offset >= 0, frame_stride >= 0); every argument is checked on the host before any launch.  Ragged: the kernel checks each
 * descriptor; an invalid one gives d_status 1 and a frame of all -128 (fp16: all 0) and is never read.  The _f16 forms write the fp16
 * network's frames (56x56 only; see the fp16 section below).  One launch each, asynchronous on `stream`, no allocation, no host
 * synchronisation; n = 0 launches nothing and returns 0.
 * There are no run_decode forms: the frames are the interface.  After a YUV prepare the caller runs yf_network_run_device (56),
 * yf_network_run_device_hw (160) or yf_network_fp16_run_device, then yf_images_decode_ragged_device, yf_images_decode160_ragged_device
 * or yf_images_decode_f32_ragged_device with yf_image descriptors of the pictures' sizes: those three decodes read only `height` and
 * `width` of a descriptor (offset and row_stride may be anything), so boxes come out in the Y plane's pixels.  INTEGRATION.md has the
 * sequence. */
YF_API long yf_images_prepare_yuv_device(const void* d_pixels, size_t pixels_bytes, int format, int height, int width, long stride_y,
                                         long uv_offset, long stride_uv, long frame_stride, long n, int out_hw, void* d_frames,
                                         void* stream);
YF_API long yf_images_prepare_yuv_ragged_device(const void* d_pixels, size_t pixels_bytes, int format, const yf_image_yuv* d_images, long n,
                                                int out_hw, void* d_frames, int32_t* d_status, void* stream);
YF_API long yf_images_prepare_yuv_f16_device(const void* d_pixels, size_t pixels_bytes, int format, int height, int width, long stride_y,
                                             long uv_offset, long stride_uv, long frame_stride, long n, void* d_frames_f16, void* stream);
YF_API long yf_images_prepare_yuv_f16_ragged_device(const void* d_pixels, size_t pixels_bytes, int format, const yf_image_yuv* d_images,
                                                    long n, void* d_frames_f16, int32_t* d_status, void* stream);

/* Images -> frames (the caller's workspace d_frames int8[n][56][56][3]) -> heads d_heads int8[n][7][7][18] -> yf_det records
 * d_dets[n][cap], d_counts int32[n], boxes in each image's own pixels: w_scale = (float)((double)W / 56.0), h_scale likewise (the
 * script's `W/56.` applied to a float32 array).  mode: YF_DECODE_PY (the script's), YF_DECODE_FW, YF_DECODE_FW_HOST.
 * Uniform: the scales are scalars and decode stays fused in the network launch (yf_network_run_decode_device). */
YF_API long yf_images_run_decode_device(ai_handle net, const void* d_pixels, size_t pixels_bytes, int format, int height, int width,
                                        long row_stride, long frame_stride, long n, void* d_frames, void* d_heads, int mode,
                                        void* d_dets, void* d_counts, int cap, void* stream);
/* Ragged: yf_network_run_device, then a per-image-scale decode; an invalid image (d_status 1) gets count 0. */
YF_API long yf_images_run_decode_ragged_device(ai_handle net, const void* d_pixels, size_t pixels_bytes, int format,
                                               const yf_image* d_images, long n, void* d_frames, void* d_heads, int mode,
                                               void* d_dets, void* d_counts, int cap, int32_t* d_status, void* stream);
/* Decode tables.  This library keeps its own copy of the sigmoid / exp tables on each device (the shipped pair at first) together with the id of
 * what it uploaded.  An entry point that takes a network and decodes int8 heads here -- the ragged 56x56 run, both 160x160 runs -- compares
 * yf_network_decode_tables' id with that id before it launches and, if they differ (the network was initialised from a model file with another
 * output quantisation, or went back to the shipped model), uploads the network's pair again: synchronously, after waiting for the device, as the
 * first upload is synchronous, and not inside stream capture.  The uniform 56x56 run decodes inside the network's own launch with the network's
 * tables.  The entry points that take NO network (yf_images_decode_ragged_device, yf_images_decode160_device,
 * yf_images_decode160_ragged_device) decode with the pair last given to this setter, under the same id rule; without a call that is the shipped
 * pair.  sig_bits, exp_bits: float32 bits, index q + 128, the sigmoid table not decreasing; id: what yf_network_decode_tables returned with them
 * (equal ids must mean equal tables).  Host-only, copies the tables.  0, or -1 (NULL or a decreasing sigmoid table).  The fp16 / float32 entries
 * use no tables. */
YF_API int yf_images_set_decode_tables(const uint32_t sig_bits[256], const uint32_t exp_bits[256], uint64_t id);
/* Per-image scales for heads that already exist (d_heads int8[n][7][7][18]); a descriptor whose height or width is outside
 * [1, 16384] gets count 0. */
YF_API long yf_images_decode_ragged_device(const void* d_heads, const yf_image* d_images, long n, int mode,
                                           void* d_dets, void* d_counts, int cap, void* stream);

/* Greedy IoU suppression of decoded records: YoloFaceDetector.non_max_suppression of yoloface/tensorflow/yoloface_test.py:145-190
 * (threshold 0.4 there, line 32), per frame, on the records of any decode above (or of yf_network_decode_device, the fused decode, the
 * camera pipeline).  d_dets yf_det[n][cap], d_counts int32[n] -> d_out yf_det[n][cap], d_out_counts int32[n]; d_out may equal d_dets and
 * d_out_counts d_counts (in place).  Records and counts 4-byte aligned.
 *   input:  the first m = min(max(count, 0), cap) records of the frame, in decode order.  A frame whose count is above cap (the decode
 *           wrote only cap records) is suppressed over the cap records that exist: cap >= 147, the number of candidates, gives the
 *           reference's answer.  cap <= YF_IMAGES_NMS_MAX_CAP.
 *   order:  descending conf, the float32 stored in the record; ties go later record first (np.argsort(conf, kind="stable")[::-1]).  The
 *           reference's conf.argsort()[::-1] uses numpy's default sort, which is not stable, so its order among equal confidences depends
 *           on the numpy build: this tie rule is the library's choice, and agrees with the reference whenever the confidences differ.
 *           Ties are common: the confidence comes from an int8 logit, and the sigmoid table gives 1.0f to several of them.
 *   arithmetic: float64, one IEEE operation per numpy operation, in the reference's order, no contraction (csrc/yf_images_nms.h):
 *           area = (x2 - x1 + 1) * (y2 - y1 + 1); w = max(0.0, min(x2) - max(x1) + 1), h likewise; inter = w * h;
 *           union = (area[i] + area[j]) - inter; record j survives the kept record i iff inter / union <= iou_threshold.  The int32 edges
 *           convert exactly and products above 2^53 round as numpy's do.  Unions <= 0 occur (YF_DECODE_FW clamps can give x1 > x2, and
 *           YF_DECODE_PY edges INT32_MIN): they follow IEEE, 0 / 0 = NaN is suppressed at every threshold, 0 / negative = -0.0.
 *   output: the kept records byte for byte, in keep order (descending confidence, as boxes[keep]), at d_out[f][0..kept), kept in
 *           d_out_counts[f].  Slots at and beyond the kept count are not written.
 * iou_threshold: any value but NaN (at 0 overlapping records are suppressed and disjoint ones survive; at 1 or more only records whose
 * union with a kept one is zero are).  One launch, no allocation, no synchronisation.  Returns n; n = 0 launches nothing and
 * writes nothing. */
#define YF_IMAGES_NMS_MAX_CAP 256
YF_API long yf_images_nms_device(const void* d_dets, const void* d_counts, long n, int cap, double iou_threshold,
                                 void* d_out, void* d_out_counts, void* stream);

/* ---- 160x160 frames: the network is fully convolutional and a larger input finds smaller faces (yf_network_run_device_hw: heads
 * int8[n][20][20][18]).  The decode is tflite_prediction.py:43-63 with the hard-coded 7 of line 50 read as the script's own nx, ny (20):
 * stride 8 and the anchors unchanged, W/56. read as W/160.  3 x 20 x 20 = 1200 candidates per frame.  Only the script's decode exists at
 * this size: the firmware's loop (49 cells, clamp to 55, LCD axis swap) has no meaning here, so there is no mode argument. */
#define YF_IMAGES_GRID160      20
#define YF_IMAGES_CAND160    1200          /* 3 anchors x 20 x 20 */
/* d_heads int8[n][20][20][18] (16-byte aligned) -> records as yf_network_decode_device writes them in YF_DECODE_PY: order (anchor, row,
 * col), conf > 0.7f, d_counts int32[n] = the true count (may exceed cap), only the first cap records written (slots beyond
 * min(count, cap) are not touched).  1 <= cap <= 1200.  One launch of its own; n = 0 launches nothing and returns 0. */
YF_API long yf_images_decode160_device(const void* d_heads, long n, float w_scale, float h_scale,
                                       void* d_dets, void* d_counts, int cap, void* stream);
/* Per-image scales: w_scale = (float)((double)W / 160.0), h_scale likewise.  d_status (int32[n], as yf_images_prepare_ragged_device
 * wrote it) may be NULL; status 1 or a side outside [1, 16384] gives count 0. */
YF_API long yf_images_decode160_ragged_device(const void* d_heads, const yf_image* d_images, const int32_t* d_status, long n,
                                              void* d_dets, void* d_counts, int cap, void* stream);
/* Images -> frames (d_frames int8[n][160][160][3], the caller's workspace) -> yf_network_run_device_hw(net, 160, 160) -> heads ->
 * records, on one stream: the prepare above at out_hw = 160, the network with the requantisation rounding selected on it, then the decode
 * of 20x20 heads as a launch of its own.  Arguments are checked as by the 56x56 forms, all before the first launch; in the ragged form an
 * invalid image (d_status 1) gets an all -128 frame and count 0. */
YF_API long yf_images_run_decode160_device(ai_handle net, const void* d_pixels, size_t pixels_bytes, int format, int height, int width,
                                           long row_stride, long frame_stride, long n, void* d_frames, void* d_heads,
                                           void* d_dets, void* d_counts, int cap, void* stream);
YF_API long yf_images_run_decode160_ragged_device(ai_handle net, const void* d_pixels, size_t pixels_bytes, int format,
                                                  const yf_image* d_images, long n, void* d_frames, void* d_heads,
                                                  void* d_dets, void* d_counts, int cap, int32_t* d_status, void* stream);
/* yf_images_nms_device for up to 1200 records per frame: the same input, order, arithmetic and output, word for word, with
 * 1 <= cap <= YF_IMAGES_NMS_WIDE_MAX_CAP; on inputs both accept the two give identical bytes.  One workgroup per four frames; what a
 * frame costs follows its own record count, not cap: a frame of up to 64 records is one wave's work in registers, a larger one is ranked
 * and suppressed by the workgroup in LDS, serially in the number of kept records as the reference's loop is. */
#define YF_IMAGES_NMS_WIDE_MAX_CAP 1200
YF_API long yf_images_nms_wide_device(const void* d_dets, const void* d_counts, long n, int cap, double iou_threshold,
                                      void* d_out, void* d_out_counts, void* stream);

/* ---- the fp16 network (yf_network_fp16_init / yf_network_fp16_run_device: fp16 frames [n][56][56][3] in, float32 logits [n][7][7][18]
 * out): the reference's float caller, yoloface/tensorflow/h5_predition.py:29-73, for a batch.  The arithmetic is stated once, in
 * csrc/yf_images_float.h, which the kernels and a host build share.
 *   frames:  frame[y][x][c] = fp16(R[y][x][rgb(c)] / 255.), R = cv2.resize(image, (56, 56)) as above; 18 816 bytes per frame, d_frames_f16
 *            16-byte aligned.  The script's float64 `/255.`, the model's float32 and the network's fp16 give the same half for each of
 *            the 256 bytes.  Only 56x56: the fp16 network has no other size.  Arguments are checked as by the int8 forms; in the ragged
 *            form an invalid image gets d_status 1 and a frame of fp16 zeros (pixel 0), and is never read.
 *   decode:  d_logits float32 [n][7][7][18] (4-byte aligned) -> yf_det records in the order (anchor, row, col), conf > 0.7f (a NaN does
 *            not fire), one IEEE float32 operation per numpy operation of h5_predition.py:51-72 in the script's order:
 *            sigmoid(x) = 1.0f / (1.0f + E(-x)); cx = (sigmoid(tx) + col) * 8, cy likewise with row; w = E(tw) * anchor_w, h likewise;
 *            edges cx -+ w / 2, cy -+ h / 2, times w_scale / h_scale, float32 -> int32 as YF_DECODE_PY (truncation; out of range and
 *            NaN -> INT32_MIN).  E(x) is the float32 nearest to the float64 value of e^x, on the whole float32 domain (+inf above
 *            ~88.72, subnormals, 0, NaN -> NaN) -- the library's choice: numpy's own float32 exp differs from it by up to 2 ulp,
 *            depending on the numpy build and the CPU, which can move an edge of the script's by 1.
 *            The record's q_conf is 0 (there is no int8 logit); conf is the float32 sigmoid above.  d_counts[f] is the true count, which
 *            may exceed cap; only the first cap records are written, slots at and beyond min(count, cap) are not touched.
 *            1 <= cap <= 147.  The records feed yf_images_nms_device unchanged.
 * Each call: asynchronous on `stream`, no allocation, no host synchronisation, every argument checked before the first launch; n = 0
 * launches nothing and returns 0. */
YF_API long yf_images_prepare_f16_device(const void* d_pixels, size_t pixels_bytes, int format, int height, int width,
                                         long row_stride, long frame_stride, long n, void* d_frames_f16, void* stream);
YF_API long yf_images_prepare_f16_ragged_device(const void* d_pixels, size_t pixels_bytes, int format, const yf_image* d_images, long n,
                                                void* d_frames_f16, int32_t* d_status, void* stream);
YF_API long yf_images_decode_f32_device(const void* d_logits, long n, float w_scale, float h_scale,
                                        void* d_dets, void* d_counts, int cap, void* stream);
/* Per-image scales: w_scale = (float)((double)W / 56.0), h_scale likewise.  d_status (int32[n], as the ragged prepare wrote it) may be
 * NULL; status 1 or a side outside [1, 16384] gives count 0. */
YF_API long yf_images_decode_f32_ragged_device(const void* d_logits, const yf_image* d_images, const int32_t* d_status, long n,
                                               void* d_dets, void* d_counts, int cap, void* stream);
/* Images -> fp16 frames (d_frames_f16, the caller's workspace) -> yf_network_fp16_run_device -> logits (d_logits) -> records, on one
 * stream.  A network on which yf_network_fp16_init has not succeeded is an error (the network's own text is passed on) and nothing is
 * launched. */
YF_API long yf_images_run_decode_f16_device(ai_handle net, const void* d_pixels, size_t pixels_bytes, int format, int height, int width,
                                            long row_stride, long frame_stride, long n, void* d_frames_f16, void* d_logits,
                                            void* d_dets, void* d_counts, int cap, void* stream);
YF_API long yf_images_run_decode_f16_ragged_device(ai_handle net, const void* d_pixels, size_t pixels_bytes, int format,
                                                   const yf_image* d_images, long n, void* d_frames_f16, void* d_logits,
                                                   void* d_dets, void* d_counts, int cap, int32_t* d_status, void* stream);

/* ---- scoring records against ground truth: calculate_iou / calculate_ap / calculate_map of yoloface/tensorflow/yolov3_train_tf.py:657-759
 * (what evaluate_model, :809-869, reports) on the records of any decode or suppression above, without the records leaving the device.  The
 * arithmetic is stated once, in csrc/yf_images_eval.h, which the kernels and a host build share: float64, one IEEE operation per Python
 * operation, in the reference's order, no contraction.
 *   input:  d_dets yf_det[n][cap], d_counts int32[n]: the first min(max(count, 0), cap) records of each frame, as for the suppression;
 *           a record's frame is its place in the array (the `frame` field is not read).  1 <= cap <= YF_IMAGES_NMS_WIDE_MAX_CAP.
 *           d_gt yf_gt_box[n][gt_cap] (8-byte aligned), d_gt_counts int32[n], clamped the same way; 1 <= gt_cap <= YF_IMAGES_EVAL_MAX_GT.
 *           A ground-truth row may hold anything, infinities and NaN included: it behaves as it does in Python.
 *   iou:    NOT the suppression's formula -- there is no + 1: w = max(0, min(x2) - max(x1)), h likewise, inter = w * h,
 *           union = (area_d + area_g) - inter, iou = inter / union if union > 0 else 0.0.
 *   match:  per record the ground truth of its frame with the largest IoU, the first one among equals, none at IoU 0 (d_best: its
 *           index, or -1).  The record is a candidate iff that IoU >= iou_threshold.
 *   order:  descending conf, the float32 stored in the record; ties go EARLIER record first (lower frame, then lower slot: the stable
 *           list.sort of :713) -- the opposite of the suppression's tie rule.  -0.0 ties with +0.0.  The reference's comment says "by
 *           confidence"; the key it wrote, x[4] behind an image id, reads the box's y2.  By confidence is the library's choice.
 *           Python's sort is not defined for a NaN confidence, which no decode produces; the library's choice: NaN sorts after every
 *           number.
 *   claim:  in that order a candidate whose ground truth is unclaimed claims it and is a true positive (d_tp 1); every other record is a
 *           false positive (d_tp 0), also a candidate whose ground truth was claimed before: there is no second choice.
 *   curve:  over the m records of the batch in that order: precision = ctp / (ctp + cfp + 1e-16), recall = ctp / max(1, num_gt), the
 *           precision made non-increasing from the back, ap = sum over i = 1 .. m - 1 of (recall[i] - recall[i - 1]) * precision[i],
 *           added in that order.  The reference leaves the term of i = 0 out, and so does this: m <= 1 gives 0.0. */
typedef struct yf_gt_box { double x1, y1, x2, y2; } yf_gt_box;                       /* 32 bytes */
typedef struct yf_eval_result { double ap; int64_t detections, ground_truths, true_positives; } yf_eval_result;
#define YF_IMAGES_EVAL_MAX_GT 256
#define YF_IMAGES_EVAL_SORT_TILE 1024      /* records per tile of the sort below (yf_images_eval_sort_tile returns it) */
/* Match and claim.  Writes d_tp[n][cap] and, unless it is NULL, d_best int32[n][cap] for the records that exist; slots beyond them are not
 * written.  One launch, one wave per frame in passes of 64 records: what a frame costs follows its own counts, not the caps.
 * iou_threshold: any value but NaN.  No allocation, no synchronisation; returns n; n = 0 launches nothing -- after the checks, as
 * everywhere in this library: d_dets, d_counts, d_gt, d_gt_counts and d_tp must be valid pointers for an empty batch too. */
YF_API long yf_images_match_device(const void* d_dets, const void* d_counts, long n, int cap,
                                   const yf_gt_box* d_gt, const int32_t* d_gt_counts, int gt_cap, double iou_threshold,
                                   uint8_t* d_tp, int32_t* d_best, void* stream);
/* Average precision of the batch from the flags of the match.  The order is a stable least-significant-digit radix sort of the mapped
 * confidence bits (the input position already ascends with frame and slot); the cumulative counts and the envelope are scans over tiles
 * of YF_IMAGES_EVAL_SORT_TILE records; the terms of the true positives are added in order by one wave.  All scratch is the caller's:
 * d_work (16-byte aligned) of at least yf_images_average_precision_workspace(n, cap) bytes (0 for arguments the call would refuse); a
 * smaller work_bytes is an error and nothing is launched.  num_gt is the sum of the clamped d_gt_counts.  d_result receives one
 * yf_eval_result; d_curve, unless NULL, double[m][2] = (recall, envelope precision) in the order above -- its capacity n * cap is the
 * caller's to provide.  n * cap < 2^31.  20 launches on `stream` whatever the counts (2 to gather the keys, 4 x 3 to sort, 6 for the
 * curve and the sum), nothing is read back, no allocation, no synchronisation; returns n; n = 0 launches nothing and writes nothing --
 * after the checks: every pointer but d_curve, d_work included, must be valid for an empty batch too.  Five of the launches are one
 * workgroup each (the scans over frames, digits and tiles); their time grows with the number of tiles, see profiles/eval_bench.txt. */
YF_API size_t yf_images_average_precision_workspace(long n, int cap);
YF_API long yf_images_average_precision_device(const void* d_dets, const void* d_counts, const uint8_t* d_tp, long n, int cap,
                                               const int32_t* d_gt_counts, int gt_cap, void* d_work, size_t work_bytes,
                                               yf_eval_result* d_result, double* d_curve, void* stream);
YF_API int yf_images_eval_sort_tile(void);

/* ---- tiled detection: a large image as overlapping tiles, each one a frame of the network, and the tiles' records one image's records
 * again.  The reference has no tiling (its callers squeeze the whole photograph into one 56x56 frame, where a 60-pixel face of a
 * 1920x1080 picture is less than 2 pixels): the grid, the order of the tiles and of the merged records and the saturation of a
 * translated edge are this library's own definition, stated once in csrc/yf_images_tiles.h, which the kernels and a host build share.
 * A C host's sequence: plan (host), upload descriptors, tiles and first, any ragged run above over the tile descriptors, gather,
 * yf_images_nms_wide_device in place -- INTEGRATION.md.
 *   grid:   per axis of length L, tile side T >= 1, stride 1 <= S <= T: L <= T gives one tile [0, L); otherwise
 *           k = (L - T + S - 1) / S + 1 tiles of side T at i * S for i < k - 1 and at L - T for the last, flush with the edge.  An image's
 *           tiles are in row-major order, y outer.  whole != 0: an image whose grid has more than one tile gets the whole image (origin
 *           0, 0, H x W) as one more region, its FIRST tile; a one-tile grid already is the whole image and is not doubled. */
typedef struct yf_tile { int32_t image, x0, y0, height, width; } yf_tile;           /* 20 bytes */
/* Host-only, no GPU call.  images[n]: the parents (only offset, height, width, row_stride are read; no pixel).  Returns the number of
 * tiles t; with tiles == NULL it only counts and writes nothing.  Otherwise tiles[t], tile_images[t] and first[n + 1] (all required) are
 * written: tile_images[j] is a descriptor the ragged entry points take unchanged -- offset = parent.offset + y0 * parent.row_stride +
 * x0 * C, the parent's row stride -- and first[i] .. first[i + 1] is the tile range of image i (first[0] = 0, first[n] = t).
 * -1 with an error text: a bad argument (format, n < 0, a tile side < 1, a stride outside [1, tile side], a missing array), a parent
 * with a side outside [1, 16384], t above tiles_cap, or t >= 2^31. */
YF_API long yf_images_plan_tiles(const yf_image* images, long n, int format, int tile_h, int tile_w, int stride_y, int stride_x,
                                 int whole, yf_tile* tiles, yf_image* tile_images, int32_t* first, long tiles_cap);
/* The merge on the device.  d_dets yf_det[t][cap], d_counts int32[t]: what any decode above wrote for the t tiles; of tile j the first
 * m_j = min(max(count, 0), cap) records are read, the suppression's clamp.  1 <= cap <= 1200, 1 <= out_cap <= YF_IMAGES_NMS_WIDE_MAX_CAP,
 * t * cap < 2^31, n < 2^31.  d_tiles yf_tile[t] (only x0 and y0 are read: membership comes from d_first alone), d_first int32[n + 1].
 *   output: d_out yf_det[n][out_cap] (no overlap with d_dets), d_out_counts int32[n].  For image i the tiles first[i] <= j < first[i + 1]
 *           in ascending j, each tile's m_j records in their order: this concatenation goes to d_out[i][0..).  d_out_counts[i] = the
 *           sum of the m_j, the true total, which may exceed out_cap; only the first out_cap records of the concatenation are written
 *           (the cut may fall inside a tile), slots at and beyond min(total, out_cap) are not written.
 *   record: the read one byte for byte, except frame = i, and x1, x2 + x0, y1, y2 + y0, the sum in int64 clamped to int32: an
 *           INT32_MIN edge of YF_DECODE_PY moves by the origin, a saturated INT32_MAX edge of YF_DECODE_FW stays.
 *   safety: for a non-decreasing d_first with first[0] = 0 and first[n] = t the result is as above.  For any other content the output
 *           is unspecified, but no access leaves the buffers: every index that comes from device memory is range-checked before use.
 * Two launches (a scan of the tile counts per image, one wave per tile to copy) whose cost follows the tiles and the records, never cap
 * or out_cap; no allocation, no synchronisation, capturable.  d_work: 16-byte aligned, at least yf_images_gather_tiles_workspace(t)
 * bytes (4 per tile, rounded up to 16; 0 for t <= 0); a smaller work_bytes is an error and nothing is launched.  Returns n; n = 0 or
 * t = 0 launches nothing (t = 0 with n > 0 writes nothing either) -- after the checks: every pointer must be valid then too. */
YF_API size_t yf_images_gather_tiles_workspace(long t);
YF_API long   yf_images_gather_tiles_device(const void* d_dets, const void* d_counts, long t, int cap,
                                            const yf_tile* d_tiles, const int32_t* d_first, long n,
                                            void* d_out, void* d_out_counts, int out_cap,
                                            void* d_work, size_t work_bytes, void* stream);

/* ---- face chips: every record's region cut from its picture and resized to one fixed size, what a recogniser, a landmark model or a
 * blur filter takes next -- from the source where it lies, packed pixels or an NV12 / NV21 surface, without the records leaving the
 * device.  The reference stops at the boxes (cv2.rectangle, yoloface/tflite/tflite_prediction.py:64): the region rule, the order of the
 * chips and the status codes are this library's own definition, stated once in csrc/yf_images_crop.h, which the kernels and a host build
 * share.  A C host's sequence: any run above, a suppression, the crop -- INTEGRATION.md.
 *   input:  d_dets yf_det[n][cap], d_counts int32[n], as any decode, suppression or tile merge above writes them; of frame i the first
 *           m_i = min(max(count, 0), cap) records are read, the suppression's clamp.  1 <= cap <= YF_IMAGES_NMS_WIDE_MAX_CAP,
 *           n * cap < 2^31.  The picture of frame i is descriptor i of d_images (yf_image for the four packed formats, yf_image_yuv for
 *           NV12 / NV21); the kernel checks each descriptor exactly as the ragged prepares do.  After a tile merge the pictures are the
 *           parents.
 *   order:  chip k = first[i] + s is slot s of frame i; d_first int32[n + 1] (written) is the exclusive prefix of the m_i, first[n] the
 *           true total, which may exceed chips_cap.  Only chips k < chips_cap are written; chip slots and info rows at and beyond
 *           min(total, chips_cap) are not touched.
 *   region: int64 arithmetic on the int32 edges, which are inclusive.  bw = x2 - x1 + 1, bh = y2 - y1 + 1, either < 1: status 1.
 *           Margin: mx = bw * margin_permille / 1000, my likewise (floor); x1 -= mx, x2 += mx, y1 -= my, y2 += my.  With
 *           YF_CROP_SQUARE: side = max(x2 - x1 + 1, y2 - y1 + 1), x1 -= (side - (x2 - x1 + 1)) / 2, x2 = x1 + side - 1, y likewise.
 *           Clamp to [0, W - 1] x [0, H - 1]; x1 > x2 or y1 > y2: status 1.  The region is not squared again after the clamp.
 *   chip:   cv2.resize(P[y1 : y2 + 1, x1 : x2 + 1], (out_w, out_h)), INTER_LINEAR as everywhere in this library; P the picture's three
 *           colour bytes, or the converted surface (each sampled pixel converted first, its chroma pair taken by its absolute row and
 *           column in the surface, so odd origins and odd sides are right).  out_format, YF_PIX_RGB8 or YF_PIX_BGR8, is the byte order of
 *           the chip.  d_chips uint8 [chips_cap][out_h][out_w][3], 16-byte aligned; out_h and out_w multiples of 16 in [16, 256].
 *   info:   d_info yf_chip[chips_cap]: the frame, the slot, the region actually sampled (x0, y0, width, height: chip pixel (cx, cy) lies
 *           near picture pixel (x0 + cx * width / out_w, y0 + cy * height / out_h)) and the status: 0 a chip, 1 an empty region, 2 the
 *           picture's descriptor is invalid (checked first: every record of such a picture has status 2).  A chip of status 1 or 2 is
 *           all zero bytes, its picture is never read, and x0 = y0 = width = height = 0.
 *   safety: counts and records are device memory that may hold anything; every index derived from them is range-checked before use, and
 *           no load leaves a picture's extent as its descriptor states it.
 * Two launches (a scan of the clamped counts into d_first, one workgroup per chip that exists) whose cost follows the records, never cap
 * or chips_cap; asynchronous on `stream`, no allocation, no host synchronisation, capturable; every argument is checked before the first
 * launch, and each entry refuses the other family's formats with a text.  Every pointer must be valid (d_dets, d_counts, d_first and
 * d_info 4-byte aligned, d_images 8-byte aligned) for an empty batch too.  Returns n; n = 0 launches nothing and returns 0, after the
 * checks. */
typedef struct yf_chip { int32_t frame, slot, x0, y0, width, height, status; } yf_chip;     /* 28 bytes */
#define YF_CROP_SQUARE 1
YF_API long yf_images_crop_records_device(const void* d_pixels, size_t pixels_bytes, int format, const yf_image* d_images,
                                          const void* d_dets, const void* d_counts, long n, int cap, int out_h, int out_w,
                                          int out_format, int margin_permille, int flags, void* d_chips, long chips_cap,
                                          int32_t* d_first, yf_chip* d_info, void* stream);
YF_API long yf_images_crop_records_yuv_device(const void* d_pixels, size_t pixels_bytes, int format, const yf_image_yuv* d_images,
                                              const void* d_dets, const void* d_counts, long n, int cap, int out_h, int out_w,
                                              int out_format, int margin_permille, int flags, void* d_chips, long chips_cap,
                                              int32_t* d_first, yf_chip* d_info, void* stream);

/* ---- redaction: the write side of the boxes.  Every record's region of its picture is pixelated (a block mosaic) or filled with one
 * colour, in place, in the picture where it lies -- packed pixels or an NV12 / NV21 surface -- without the records leaving the device:
 * video anonymisation, dataset scrubbing, a privacy filter in front of a recorder or encoder.  The reference has no such step; the
 * definition is this library's own, stated once in csrc/yf_images_redact.h, which the kernels and a host build share.  A C host's
 * sequence: any run above, a suppression, the redaction -- INTEGRATION.md.
 *   input:  d_dets, d_counts, n, cap, d_images, margin_permille, flags as the crop above takes them: of frame i the first
 *           m_i = min(max(count, 0), cap) records count, the region of a record is the crop's region (margin, YF_CROP_SQUARE, clamp; a
 *           record without a region is skipped), the picture of frame i is descriptor i.  d_pixels is read and WRITTEN.
 *   mosaic: mode YF_REDACT_MOSAIC, block = k in {4, 8, 16, 32, 64}; colour is ignored.  The block grid is anchored at picture pixel
 *           (0, 0); blocks at the right and bottom edge are clipped.  A region touches the blocks bx in [x0 / k, (x0 + width - 1) / k],
 *           by likewise; the redacted set of a picture is the union of the blocks its records touch.  Every pixel of a block of the set
 *           gets, per colour byte channel, v = (sum + cnt / 2) / cnt over the block's cnt pixels as they were before the call.  The
 *           fourth byte of BGRA / RGBA is neither read nor written.  NV12 / NV21: the blocks of the Y plane, and for each the chroma
 *           block of the same (bx, by) -- k / 2 pairs by k / 2 rows, clipped to W / 2 and H / 2 -- whose first bytes are averaged
 *           together and whose second bytes together.  The result does not depend on the order of a frame's records, and a second call
 *           changes nothing.
 *   fill:   mode YF_REDACT_FILL, block = 0, colour = 0x00RRGGBB (NV12 / NV21: 0x00YYUUVV); a non-zero top byte is refused.  Every pixel
 *           of every region, the exact region, gets R, G, B in the bytes where the format keeps them; alpha is untouched.  NV12 / NV21:
 *           the region's Y bytes and the chroma pairs cx in [x0 >> 1, (x0 + width - 1) >> 1], cy in [y0 >> 1, (y0 + height - 1) >> 1],
 *           (U, V) for NV12 and (V, U) for NV21.
 *   output: nothing outside the redacted set is written, row padding and the bytes between pictures included.  d_first int32[n + 1]
 *           (written): the exclusive prefix of the m_i, first[n] the total, as for chips; it is also the kernels' schedule.  d_status
 *           int32[n] (written): 0, or 1 for a picture whose descriptor is invalid (checked as the ragged prepares check it), which is
 *           neither read nor written.
 *   alias:  for the mosaic the pictures of different frames must not share bytes.  The call cannot check this: a caller who breaks it
 *           gets unspecified picture contents, but never an access outside a picture's extent.  The fill tolerates shared pictures,
 *           because all writers write the same bytes.
 *   safety: counts, records and d_first (read back) are device memory that may hold anything; every index derived from them is
 *           range-checked before use, and no load or store leaves a picture's or plane's extent as its descriptor states it.
 * Two launches (the crop's scan of the clamped counts into d_first, one workgroup per record that exists); asynchronous on `stream`, no
 * allocation, no host synchronisation, capturable; every argument is checked before the first launch, and each entry refuses the other
 * family's formats with a text.  Every pointer must be valid (d_dets, d_counts, d_first and d_status 4-byte aligned, d_images 8-byte
 * aligned) for an empty batch too.  Returns n; n = 0 launches nothing and returns 0, after the checks. */
enum { YF_REDACT_MOSAIC = 0, YF_REDACT_FILL = 1 };
YF_API long yf_images_redact_records_device(void* d_pixels, size_t pixels_bytes, int format, const yf_image* d_images, const void* d_dets,
                                            const void* d_counts, long n, int cap, int mode, int block, uint32_t colour,
                                            int margin_permille, int flags, int32_t* d_first, int32_t* d_status, void* stream);
YF_API long yf_images_redact_records_yuv_device(void* d_pixels, size_t pixels_bytes, int format, const yf_image_yuv* d_images,
                                                const void* d_dets, const void* d_counts, long n, int cap, int mode, int block,
                                                uint32_t colour, int margin_permille, int flags, int32_t* d_first, int32_t* d_status,
                                                void* stream);

/* ---- redaction by blur: the third way to hide a face, the one video anonymisers use by default.  Every record's region is replaced by
 * a coarse grid of its own means resized back to the region, in place, in the picture where it lies.  The grid is per face -- every face
 * gets the same number of cells, so a large face is hidden as well as a small one, which a mosaic of a fixed block is not.  The
 * reference has no such step; the definition is this library's own, stated once in csrc/yf_images_blur.h, which the kernels and a host
 * build share.  A C host's sequence and the video loop with the tracker in front: INTEGRATION.md.
 *   input:  d_dets, d_counts, n, cap, d_images, margin_permille, flags as the redaction above takes them (records, regions, pictures
 *           are exactly its own).  d_pixels is read and WRITTEN.
 *   grid:   grid = g in [1, YF_BLUR_MAX_GRID].  A region of width x height pixels has gx = max(1, min(g, width / m)) by gy (likewise
 *           from height) cells, m = YF_BLUR_MIN_CELL for packed pixels and the Y plane, 2 for the chroma plane: no cell is narrower than
 *           m, so that a small region does not come back as it was (only a 1 x 1 region keeps its bytes).  Cell cx holds the region's
 *           columns [cx * width / gx, (cx + 1) * width / gx), rows likewise (integer division).
 *   means:  per cell and colour byte channel v = (sum + cnt / 2) / cnt over the cell's pixels as they were before the call, exact
 *           integers in 64 bits.  The fourth byte of BGRA / RGBA is neither read nor written.
 *   result: the region's pixels become cv2.resize(G, (width, height)), INTER_LINEAR, of the [gy, gx, channels] grid of means G, as
 *           csrc/yf_images_taps.h restates it.  A constant region stays constant.
 *   yuv:    the Y plane is a one-channel picture over the region; the chroma plane a two-channel picture of pairs over the fill's chroma
 *           region (cx in [x0 >> 1, (x0 + width - 1) >> 1], cy likewise) with its own gx, gy, means and resample.  First bytes are
 *           averaged together and second bytes together: U / V order does not matter to the blur.
 *   overlap: a pixel in several regions of its frame belongs to the lowest slot whose region contains it and gets that record's value;
 *           a chroma pair to the lowest slot whose chroma region contains it.  Every record's grid is computed from the pixels as they
 *           were before the call, whoever owns them: the order of a frame's records matters only for who owns an overlap.  A second
 *           call blurs the blur: unlike the mosaic, the call is NOT idempotent.
 *   work:   record k = first[f] + s keeps its grid in slot k of d_work; yf_images_blur_workspace(records_cap, grid) = records_cap * grid
 *           * grid * 4 bytes rounded up to 16 (0 for arguments the call refuses).  Its contents are the library's own.  A record with
 *           k >= records_cap has no slot and is FILLED with colour (0x00RRGGBB; NV12 / NV21: 0x00YYUUVV) by the fill's rule under the same
 *           ownership rule: a face never stays visible because a buffer was small.  records_cap = 0 is legal and turns the call into a
 *           fill; records_cap = n * cap fills nothing.
 *   output: nothing but the owned pixels of the regions is written, row padding and the bytes between pictures included.  d_first
 *           int32[n + 1] (written): the exclusive prefix of the m_i; first[n] is the records_cap that would have sufficed.  d_status
 *           int32[n] (written), two bits: bit 0 the picture's descriptor is invalid, the picture is neither read nor written; bit 1
 *           (value 2) the frame has a record without a slot (first[f + 1] > first[f] and first[f + 1] > records_cap).
 *   alias:  the pictures of different frames must not share bytes (otherwise unspecified contents, never an access outside a picture's
 *           extent).
 *   safety: counts, records and d_first (read back) are device memory that may hold anything; every index derived from them is
 *           range-checked before use, and no load or store leaves a picture's or plane's extent as its descriptor states it.
 * Three launches on one stream (the crop's scan; the means, one workgroup per record with a slot, which reads the pictures only; the
 * paint, one workgroup per record, which reads the slots only): no kernel reads a byte that another workgroup of its launch writes.
 * Asynchronous on `stream`, no allocation, no host synchronisation, capturable; every argument is checked before the first launch
 * (n, cap, grid, colour's top byte, margin_permille, flags, records_cap in [0, n * cap], work_bytes, d_work non-NULL and 16-byte aligned
 * when the workspace is not 0), and each entry refuses the other family's formats with a text.  Pointer rules as for the redaction.
 * Returns n; n = 0 launches nothing and returns 0, after the checks. */
#define YF_BLUR_MAX_GRID 16
#define YF_BLUR_MIN_CELL 4
YF_API size_t yf_images_blur_workspace(long records_cap, int grid);
YF_API long yf_images_blur_records_device(void* d_pixels, size_t pixels_bytes, int format, const yf_image* d_images, const void* d_dets,
                                          const void* d_counts, long n, int cap, int grid, uint32_t colour, int margin_permille, int flags,
                                          void* d_work, size_t work_bytes, long records_cap, int32_t* d_first, int32_t* d_status,
                                          void* stream);
YF_API long yf_images_blur_records_yuv_device(void* d_pixels, size_t pixels_bytes, int format, const yf_image_yuv* d_images,
                                              const void* d_dets, const void* d_counts, long n, int cap, int grid, uint32_t colour,
                                              int margin_permille, int flags, void* d_work, size_t work_bytes, long records_cap,
                                              int32_t* d_first, int32_t* d_status, void* stream);

/* ---- drawing: where every script of the reference ends.  The outline of every record is drawn in place into the picture where it lies
 * -- packed pixels or an NV12 / NV21 surface -- without the records leaving the device: cv2.rectangle(img, (x1, y1), (x2, y2), (0, 0, 255),
 * 2) of yoloface/tflite/tflite_prediction.py:59-64 (and LCD_DrawRectangle of the firmware) for a whole batch, in one colour or, with keys,
 * in a colour per record -- the track id of the tracker below keeps a face's colour over the frames.  The definition is stated once in
 * csrc/yf_images_draw.h, which the kernels and a host build share.  The video loop with drawing: INTEGRATION.md.
 *   input:  d_dets, d_counts, n, cap, d_images as the redaction above takes them; d_pixels is WRITTEN (never read).
 *   set:    the record's four int32 edges as they are (no margin, no square, no clamp), xa = min(x1, x2), xb = max(x1, x2), y likewise,
 *           int64 arithmetic.  half = h in [0, 3].  For a pixel (x, y): ex = max(xa - x, x - xb, 0), ix = min(x - xa, xb - x), ey and iy
 *           likewise.  Drawn iff ex <= h and ey <= h; and ex == 0 or ey == 0 or ex * ex + ey * ey <= h * h (round outer corners); and
 *           ex > 0 or ey > 0 or min(ix, iy) <= h (the interior stays); and the pixel lies in the picture.  h = 0: the one-pixel outline of
 *           LCD_DrawRectangle and cv2.rectangle(..., 1).  h = 1: what OpenCV's drawing.cpp is read to draw for thickness 2 (a band of three
 *           pixels per edge, a disc of radius 1 at each corner) -- read from memory of the source, NOT pinned against a real cv2.
 *   colour: d_keys NULL: colour = 0x00RRGGBB (NV12 / NV21: 0x00YYUUVV) for every record, a non-zero top byte is refused; key_stride,
 *           d_palette, palette_n must be 0, NULL, 0.  d_keys given: the record in slot s of frame f gets
 *           d_palette[key % palette_n] & 0xFFFFFF, key the uint32 at d_keys + (f * cap + s) * key_stride; key_stride a multiple of 4 in
 *           [4, 64] (the id fields of a yf_track_info array: the array, stride 16), 1 <= palette_n <= 256, both 4-byte aligned device
 *           memory.  R, G, B go where the format keeps them; alpha is never written.
 *   overlap: a pixel drawn by several records of its frame gets the colour of the highest slot that draws it.
 *   yuv:    the Y byte of every drawn pixel; a chroma pair is written iff at least one of its four luma pixels is drawn, with the chroma
 *           of the highest slot that draws any of them; (U, V) for NV12, (V, U) for NV21.
 *   output: nothing but the drawn set is written, row padding and the bytes between pictures included.  d_first int32[n + 1] and d_status
 *           int32[n] as the redaction writes them (status 1: the picture's descriptor is invalid, the picture is not touched).
 *   alias:  with keys the pictures of different frames must not share bytes (otherwise unspecified contents, never an access outside a
 *           picture's extent); without keys pictures may be shared.
 *   safety: counts, records, d_first (read back), keys and palette are device memory that may hold anything; every index derived from
 *           them is range-checked before use, and no store leaves a picture's or plane's extent as its descriptor states it.  What a
 *           record costs follows the pixels it writes, never its edges.
 * Two launches (the crop's scan, one workgroup per record that exists); asynchronous on `stream`, no allocation, no host synchronisation,
 * capturable; every argument is checked before the first launch, and each entry refuses the other family's formats with a text.  Pointer
 * rules as for the redaction.  Returns n; n = 0 launches nothing and returns 0, after the checks. */
YF_API long yf_images_draw_records_device(void* d_pixels, size_t pixels_bytes, int format, const yf_image* d_images, const void* d_dets,
                                          const void* d_counts, long n, int cap, int half, uint32_t colour, const void* d_keys,
                                          int key_stride, const uint32_t* d_palette, int palette_n, int32_t* d_first, int32_t* d_status,
                                          void* stream);
YF_API long yf_images_draw_records_yuv_device(void* d_pixels, size_t pixels_bytes, int format, const yf_image_yuv* d_images,
                                              const void* d_dets, const void* d_counts, long n, int cap, int half, uint32_t colour,
                                              const void* d_keys, int key_stride, const uint32_t* d_palette, int palette_n,
                                              int32_t* d_first, int32_t* d_status, void* stream);

/* ---- tracking: the step between "the boxes of this frame" and "what to do with this frame" of a video.  Each frame's records (after a
 * suppression) are associated with per-stream track state: every face gets an identity that lasts over the frames, and a face the
 * detector misses for a few frames is held over with its last box -- so a redaction (above) does not show it on exactly those frames,
 * and a recogniser behind the chips knows which chip is which.  The output is records again, which the crop and the redaction take as
 * they are.  The reference has no tracker; the definition is this library's own, stated once in csrc/yf_images_track.h (the match, the
 * update, the order of the output, what is out of scope), which the kernel and a host build share.  The video loop: INTEGRATION.md.
 *   state:  d_state yf_track_state[streams] (8-byte aligned), yf_images_track_state_bytes(streams) bytes (0 for streams <= 0).  An
 *           all-zero state is the empty state: a hipMemsetAsync resets a stream (or all).  The bytes are untrusted: whatever they hold,
 *           the step reads and writes only inside them.
 *   input:  the batch holds n = streams * steps frames, d_dets yf_det[n][cap], d_counts int32[n], 1 <= cap <= YF_IMAGES_NMS_WIDE_MAX_CAP.
 *           layout YF_TRACK_TIME_MAJOR: frame f = t * streams + s, one frame of every camera per step; YF_TRACK_STREAM_MAJOR:
 *           f = s * steps + t, a clip per stream.  Of a frame the first min(max(count, 0), cap, 64) records count, in the order they
 *           lie; a larger count sets bit 0 of the frame's status.  The steps of a stream are taken in order t = 0 .. steps - 1; the
 *           state at d_state[s] is read before the first and written after the last.
 *   params: a host pointer, copied.  A slot's box and a detection match if they share a pixel and their IoU (the suppression's
 *           arithmetic, float64) is >= match_iou (any value but NaN); the match is greedy by descending IoU (an optimal assignment in
 *           its place: yf_images_track_motion_assign_device, below).  A track is reported once
 *           it has min_hits >= 1 matches, and kept over max_misses >= 0 frames without one.  The library's suggestion for faces at a
 *           video rate is {0.3, 1, 5}; that is a choice, not something measured.
 *   output: d_out yf_det[n][out_cap], d_info yf_track_info[n][out_cap], d_out_counts int32[n], out_cap >= 1 (64 holds every track).
 *           Per frame the reported tracks in ascending id: the track's last record with `frame` set to f, beside {id, hits, misses,
 *           age}; misses > 0 marks a held-over track.  d_out_counts[f] is the true number; only the first out_cap are written and
 *           nothing beyond min(count, out_cap).  d_status int32[n] or NULL: bit 0 as above, bit 1: a detection found all 64 slots
 *           taken and was dropped.
 * One launch (one wave per stream, the state in registers over the stream's steps); asynchronous on `stream`, no allocation, no host
 * synchronisation, capturable.  Every argument is checked before the launch: NULL pointers (d_status excepted), 4-byte alignment of the
 * records, counts and outputs, 8-byte alignment of the state, cap, out_cap, match_iou, min_hits, max_misses, layout, streams and
 * steps >= 0 with streams * steps <= 2^31 - 2.  Returns n; n = 0 launches nothing and returns 0, after the checks; a failure returns -1
 * (unlike the entries above: here 0 is a valid n) with a text in yf_images_last_error_text. */
#define YF_TRACK_SLOTS 64
typedef struct yf_track        { uint32_t id; int32_t hits, misses, age; yf_det det; } yf_track;           /* 44 bytes; id 0 = free slot */
typedef struct yf_track_state  { uint32_t issued, reserved; yf_track slot[YF_TRACK_SLOTS]; } yf_track_state; /* 2824 bytes per stream */
typedef struct yf_track_info   { uint32_t id; int32_t hits, misses, age; } yf_track_info;                  /* 16 bytes, parallel to an output record */
typedef struct yf_track_params { double match_iou; int32_t min_hits, max_misses; } yf_track_params;
enum { YF_TRACK_TIME_MAJOR = 0, YF_TRACK_STREAM_MAJOR = 1 };
YF_API size_t yf_images_track_state_bytes(long streams);
YF_API long   yf_images_track_device(const void* d_dets, const void* d_counts, long streams, long steps, int layout, int cap,
                                     const yf_track_params* params, void* d_state, void* d_out, void* d_info, void* d_out_counts,
                                     int out_cap, int32_t* d_status, void* stream);

/* ---- tracking with a motion model: the tracker above with a constant-velocity g-h (alpha-beta) filter on every edge of a track's box.
 * The box of a held-over track moves on with the velocity the track had, so a redaction still covers a moving face on the frames the
 * detector misses it, and the face keeps its id when it is detected again -- the match is taken against the PREDICTED box.  A second
 * entry beside the one above, which does not change; the definition is stated once in csrc/yf_images_motion.h (the filter, its integer
 * arithmetic, what is still out of scope), which the kernel, a host build and a sanitizer program share.
 *   state:  d_state yf_track_motion_state[streams] (8-byte aligned), yf_images_track_motion_state_bytes(streams) bytes: 7176 per stream,
 *           a slot the base tracker's 44 bytes, 4 of padding and pos[4], vel[4] (int64, 1/256 pixel and 1/256 pixel per step, of x1, y1,
 *           x2, y2).  All zero is the empty state; the bytes are untrusted (every pos and vel read is clamped to +-2^40 first).  THE TWO
 *           ENTRIES' STATES ARE DIFFERENT FORMATS OF DIFFERENT SIZES: a yf_track_state must never be passed here, nor this state above.
 *   params: a host pointer, copied: base as above; alpha, beta, damp in [0, 256] (units of 1/256), smooth 0 or 1.  Per step and edge,
 *           P' = pos + vel; matched to a detection z: r = 256 z - P', pos = P' + alpha r / 256, vel += beta r / 256; unmatched: pos = P',
 *           vel = damp vel / 256.  (256, 0) is the tracker above, byte for byte, from the empty state; (256, 256) predicts with the last
 *           frame-to-frame difference.  The library's suggestion is {192, 128, 256, 0}: a choice, not something measured -- there is no
 *           accuracy or identity-switch figure for real video.  What exists since: yf_images_score_tracks_device below scores the
 *           reported tracks against labelled identities, and profiles/track_score_bench.txt holds its figures for the settings on
 *           SYNTHETIC clips; a figure on labelled video still does not exist.
 *   output: as above.  A held-over track (misses > 0) is reported with its last record's edges replaced by the filter's position
 *           rounded to pixels; with smooth 1 a matched track too (the filtered box), with smooth 0 it reports its detection verbatim.
 *           A predicted box is not clamped to the picture; the crop, the redaction, the blur and the drawing clip themselves.
 * The input, the layouts, the checks (and alpha, beta, damp, smooth), n = 0, the return value and the error text are the entry's above;
 * one launch, one wave per stream, the state in registers over the stream's steps; asynchronous, no allocation, capturable.  Still out
 * of scope: a covariance, clamping a predicted box; the optimal assignment is the entry below, appearance and re-identification the
 * stage further below (yf_images_reid_device). */
typedef struct yf_track_motion        { yf_track base; int32_t pad; int64_t pos[4]; int64_t vel[4]; } yf_track_motion;    /* 112 bytes */
typedef struct yf_track_motion_state  { uint32_t issued, reserved; yf_track_motion slot[YF_TRACK_SLOTS]; } yf_track_motion_state; /* 7176 bytes per stream */
typedef struct yf_track_motion_params { yf_track_params base; int32_t alpha, beta, damp, smooth; } yf_track_motion_params;         /* 32 bytes */
YF_API size_t yf_images_track_motion_state_bytes(long streams);
YF_API long   yf_images_track_motion_device(const void* d_dets, const void* d_counts, long streams, long steps, int layout, int cap,
                                            const yf_track_motion_params* params, void* d_state, void* d_out, void* d_info,
                                            void* d_out_counts, int out_cap, int32_t* d_status, void* stream);

/* ---- tracking with a motion model and optimal assignment: the entry above with a choice of the match.  Both entries above associate
 * detections with tracks by the global greedy rule -- repeatedly the eligible pair of the largest IoU --, which costs identities where
 * two faces pass each other: one detection overlaps both tracks, greedy gives it to the one it overlaps most, the other detection is
 * stranded: one new id, one track held over.  YF_ASSIGN_OPTIMAL replaces that match by a maximum-weight assignment over the eligible
 * pairs -- the weight of a pair is its IoU at 2^-30 resolution; maximum total IoU, not cardinality first --, with its ties settled by one
 * prescribed shortest-augmenting-path procedure in integers, so that the kernel, a host build and Python agree bit for bit.  The
 * definition is stated once in csrc/yf_images_assign.h (the weights, the procedure, the bound on its potentials).
 *   assign: YF_ASSIGN_GREEDY: the entry above under another name (its kernel is launched); YF_ASSIGN_OPTIMAL: the above.
 *   state, input, params, output: the entry's above (7176 bytes per stream); only the match differs.  Gains (256, 0) with
 *           YF_ASSIGN_OPTIMAL is "the base tracker with optimal assignment": NO ENTRY ON THE 2824-BYTE STATE IS ADDED.
 * The checks (the entry's above in its order, then assign), n = 0, the return value and the error text are the entry's above; one launch,
 * one wave per stream, 16 KB of LDS per wave; asynchronous, no allocation, no host synchronisation, capturable.  A frame with m
 * detections costs at most m (m + 1) / 2 rounds of the search, 2080 at m = 64; a frame without an eligible pair skips it.
 * Still missing: a covariance, clamping a predicted box (appearance and re-identification: yf_images_reid_device below).  Which match keeps identities better is
 * measured by yf_images_score_tracks_device below -- on synthetic clips so far (profiles/track_score_bench.txt: without the motion model
 * the optimal assignment exchanges two faces that pass each other where the greedy match does not), not on labelled video. */
enum { YF_ASSIGN_GREEDY = 0, YF_ASSIGN_OPTIMAL = 1 };
YF_API long   yf_images_track_motion_assign_device(const void* d_dets, const void* d_counts, long streams, long steps, int layout, int cap,
                                                   const yf_track_motion_params* params, int assign, void* d_state, void* d_out,
                                                   void* d_info, void* d_out_counts, int out_cap, int32_t* d_status, void* stream);

/* ---- scoring tracks against labelled identities: the CLEAR-MOT score (Bernardin and Stiefelhagen, 2008) of what a tracker above
 * reported against ground-truth tracks -- misses, false positives, IDENTITY SWITCHES, MOTA and MOTP --, per stream over the steps of a
 * clip, on the device: the records do not leave it.  It is what measures the tracker's settings against each other (greedy or optimal,
 * with or without the motion model, the gains); the first figures, on synthetic clips and not on video, are in
 * profiles/track_score_bench.txt.  A new entry beside the tracker's, which do not change.  The reference has no tracker; the definition
 * is this library's own, stated once in csrc/yf_images_score.h (the rows and columns that count, the continuity rule, the switches, the
 * counters, what is out of scope), which the kernel, a host build and a sanitizer program share.  Everything after the IoU is integers.
 *   truth:  d_gt yf_gt_track[n][gt_cap], d_gt_counts int32[n], 1 <= gt_cap <= 64: per frame the labelled objects {id, x1, y1, x2, y2},
 *           edges inclusive pixels as in a record; valid ids are 1 .. YF_SCORE_MAX_IDS and an id names one object of its stream.  Of a
 *           frame the first min(max(count, 0), gt_cap, 64) rows count (a larger count: status bit 0); a row of id 0, of an id above 256
 *           or of an id an earlier row of the frame has is void (status bit 2): it counts for nothing.
 *   tracks: a tracker's output as it lies: d_out yf_det[n][out_cap], d_info yf_track_info[n][out_cap] (only `id` is read),
 *           d_out_counts int32[n], out_cap >= 1; the first min(max(count, 0), out_cap, 64) records count (a larger count: status bit 1);
 *           a record of id 0 is void (status bit 3; the trackers emit none).  n = streams * steps frames in `layout`, as above.
 *   state:  d_state yf_score_state[streams] (8-byte aligned), yf_images_score_state_bytes(streams) bytes: 3136 per stream -- eight
 *           uint64 counters, then per ground-truth id the hypothesis id it was last matched to and the frames it was present and
 *           tracked.  All zero is the empty state; the bytes are untrusted: whatever they hold, a step reads and writes only inside
 *           them (only a range-checked ground-truth id indexes them).  The counters add modulo 2^64, present and tracked saturate.
 *   step:   a pair is eligible as in the tracker (the boxes share a pixel, IoU >= score_iou, any value but NaN); an object keeps the
 *           hypothesis id it was last matched to while that pair stays eligible, the remaining rows and columns are assigned by
 *           yfi_assign_solve (maximum total IoU at 2^-30 resolution); a new match to another id than the last one is one switch.
 *   output: the state; d_match int32[n][gt_cap] or NULL: for each of a frame's rows that count the column of its hypothesis, or -1
 *           (places beyond them are not written); d_status int32[n] or NULL: the bits above.
 * One launch (one wave per stream, the counters and the per-object tables in registers over the stream's steps, 16 KB of LDS);
 * asynchronous on `stream`, no allocation, no host synchronisation, capturable.  Every argument is checked before the launch
 * (yfi_score_check): NULL pointers (d_match and d_status excepted), 4-byte alignment of the arrays and 8-byte alignment of the state,
 * out_cap, gt_cap, score_iou, layout, streams and steps >= 0 with streams * steps <= 2^31 - 2.  Returns n; n = 0 launches nothing and
 * returns 0, after the checks; a failure returns -1 with a text in yf_images_last_error_text.
 * yf_images_score_summary is host only, no GPU call, like yf_images_plan_tiles: host_states are `streams` downloaded states (any
 * alignment); *out receives the sums of the counters over the streams, objects (entries with present > 0, counted per stream),
 * mostly_tracked (5 tracked >= 4 present), mostly_lost (5 tracked <= present), and
 *   mota = gt ? 1.0 - (double)(misses + false_positives + switches) / (double)gt : 0.0,
 *   motp = matches ? ((double)overlap / (double)matches) / 1073741824.0 : 0.0 -- the mean IoU of the matched pairs at 2^-30 resolution;
 * each weight carries the + 1 of the assignment's weights, so motp lies 2^-30 above the truncated mean.  Returns 0, or -1 (out NULL,
 * streams < 0, host_states NULL with streams > 0).
 * Out of scope: IDF1 and HOTA (one assignment over the whole clip, hypothesis ids without a bound), fragmentations, more than 256
 * labelled objects per stream or 64 per frame, and any figure for real labelled video. */
#define YF_SCORE_MAX_IDS 256
typedef struct yf_gt_track      { uint32_t id; int32_t x1, y1, x2, y2; } yf_gt_track;                          /* 20 bytes */
typedef struct yf_score_state   { uint64_t frames, gt, hyp, matches, misses, false_positives, switches, overlap;
                                  uint32_t last[YF_SCORE_MAX_IDS]; int32_t present[YF_SCORE_MAX_IDS], tracked[YF_SCORE_MAX_IDS]; } yf_score_state; /* 3136 bytes per stream */
typedef struct yf_score_summary { uint64_t frames, gt, hyp, matches, misses, false_positives, switches, overlap;
                                  int64_t objects, mostly_tracked, mostly_lost; double mota, motp; } yf_score_summary;  /* 104 bytes */
YF_API size_t yf_images_score_state_bytes(long streams);
YF_API long   yf_images_score_tracks_device(const void* d_out, const void* d_info, const void* d_out_counts, int out_cap, const void* d_gt,
                                            const void* d_gt_counts, int gt_cap, long streams, long steps, int layout, double score_iou,
                                            void* d_state, int32_t* d_match, int32_t* d_status, void* stream);
YF_API int    yf_images_score_summary(const void* host_states, long streams, yf_score_summary* out);

/* ---- appearance: a descriptor per record, and re-identification of lost tracks.  The three trackers above associate by box overlap
 * alone: a face that is hidden for longer than max_misses steps loses its track and returns under a new id, which the score above counts
 * as an identity switch.  These two entries are the second look at the picture: a small appearance descriptor per reported record, and
 * a stage behind a tracker that gives a newly born track the identity of a recently lost one that looks the same.  New entries beside the
 * existing ones, which do not change.  The reference has neither; the definitions are this library's own, stated once in
 * csrc/yf_images_describe.h and csrc/yf_images_reid.h, which the kernels, a host build and a sanitizer program share.  Integers
 * throughout.  The video loop with both: INTEGRATION.md.
 *
 * yf_images_describe_records_device, yf_images_describe_records_yuv_device: a yf_face_desc per record.
 *   input:  d_pixels, pixels_bytes, format, d_images, d_dets, d_counts, n, cap, margin_permille, flags as the blur above takes them:
 *           records, counts, regions and the picture checks are exactly its own.  d_pixels is only READ.
 *   output: d_desc yf_face_desc[n][cap] (4-byte aligned): the record in slot s of frame f goes to d_desc[f][s]; only the slots of the
 *           first m_f = min(max(count, 0), cap) records of a frame are written, the slots beyond them are not touched.
 *   valid:  a record's descriptor is INVALID, all 68 bytes zero, when the record has no region, when the region is narrower or lower
 *           than YF_DESC_GRID = 8 pixels, or when the picture's descriptor is invalid.  Otherwise flags = YF_DESC_VALID (bit 0) and the
 *           region is cut into 8 x 8 cells with the blur's cell bounds (cell c of a side: [c * side / 8, (c + 1) * side / 8), never
 *           empty); v[cy * 8 + cx] is the cell's mean luma in exact 64-bit integers -- packed formats: S the sum over the cell's pixels
 *           of 77 R + 150 G + 29 B, v = (S + 128 cnt) / (256 cnt), alpha never read; NV12 / NV21: v = (sum of Y + cnt / 2) / cnt, only
 *           the Y plane is read.
 *   d_first int32[n + 1] and d_status int32[n] are written as the redaction writes them; status 1: the picture's descriptor is invalid.
 * The descriptor is a tiny template, NOT a learned embedding.  The re-identification below takes any 64 bytes: a caller with a
 * recogniser behind the chips can hand over its own embedding quantised to uint8 in the place of this one.
 * Two launches on one stream (the crop's scan; one workgroup per record that exists, rows summed across the lanes, 64-bit accumulation
 * only per cell).  Asynchronous on `stream`, no allocation, no host synchronisation, capturable; every argument is checked before the
 * first launch (yfi_describe_check: n, cap, n * cap, margin_permille, flags, NULL pointers, 4-byte alignment of d_dets, d_counts, d_desc,
 * d_first, d_status, 8-byte alignment of d_images), and each entry refuses the other family's formats with a text.  Counts, records and
 * d_first (read back) are untrusted device memory, range-checked before use; no load leaves a picture's or plane's extent.  Returns n;
 * n = 0 launches nothing and returns 0, after the checks.
 *
 * yf_images_reid_device: the ids of a tracker's output rewritten.  It sits behind any of the three tracker entries and reads their output
 * as it lies -- d_info yf_track_info[n][out_cap], d_out_counts int32[n] -- with d_desc yf_face_desc[n][out_cap], the descriptors of
 * d_out (the entry above with cap = out_cap).  It writes d_info_out yf_track_info[n][out_cap]: the id replaced, hits, misses and age
 * copied; d_info_out may be d_info itself.  Draw keys, chips, redaction and yf_images_score_tracks_device take the result unchanged.  THE
 * RECORDS KEEP THE TRACKER'S ORDER: the ids of a frame are then no longer ascending.
 *   state:  d_state yf_reid_state[streams] (8-byte aligned), yf_images_reid_state_bytes(streams) bytes: 5128 per stream -- a clock and
 *           64 entries {id, the identity reported; alias, the tracker id currently mapped to it; seen, the clock when it was last bound;
 *           flags, bit 0 "has a descriptor"; v[64]}.  All zero is the empty state; the bytes are untrusted: whatever they hold, a step
 *           reads and writes only inside them.
 *   params: yf_reid_params {max_distance >= 0, max_age >= 0, blend in [0, 256]}, a host pointer that is copied.
 *   distance of two descriptors a, b with byte sums A, B: d = sum_i |(64 a_i - A) - (64 b_i - B)|, the mean-removed sum of absolute
 *           differences: exact in int32, at most 64 * 64 * 255, unchanged by a common brightness offset up to rounding.
 *   step:   of a frame the first m = min(max(count, 0), out_cap, 64) records count (a larger count: status bit 0); a record of tracker id
 *           0 is void, its id stays 0 (status bit 1).  The clock advances (modulo 2^32).  (bind) A record whose tracker id is the alias of
 *           an entry -- the lowest such entry -- reports that entry's id, and if it was detected in this frame (misses == 0) and its
 *           descriptor is valid the entry's descriptor moves towards it, per byte (old * (256 - blend) + new * blend + 128) >> 8.
 *           (expire) An entry that no record bound and whose age now - seen exceeds max_age is freed.  (re-identify) Among the unbound
 *           records that were detected with a valid descriptor and the unbound entries with a descriptor, the pair of the smallest
 *           distance <= max_distance is taken -- ties: the lowest record, then the lowest entry --, the entry's alias becomes the record's
 *           tracker id and the record reports the entry's id, again and again until no pair is left.  (births) Every record still
 *           unbound takes the lowest free entry, or evicts the unbound entry of the largest age (ties: the lowest), with id = alias =
 *           its tracker id.
 *   output: d_info_out; d_what int32[n][out_cap] or NULL: 0 void, 1 known, 2 re-identified, 3 born; d_status int32[n] or NULL.  The
 *           places at and beyond min(count, out_cap) are not written; records at and beyond 64 are copied as they are (what 0).
 * n = streams * steps frames in the tracker's layouts; the steps of stream s are taken in order on d_state[s].  One launch (one wave
 * per stream, a lane per entry, the entry's 20 words in registers over the stream's steps, the 64 x 64 distances in 16 KB of LDS; a frame
 * without an unbound record computes no distance); asynchronous on `stream`, no allocation, no host synchronisation, capturable.  Every
 * argument is checked before the launch (yfi_reid_check): NULL pointers (d_what and d_status excepted), 4-byte alignment of the arrays
 * and 8-byte alignment of the state, out_cap >= 1, the parameters, layout, streams and steps >= 0 with streams * steps <= 2^31 - 2.
 * Returns n; n = 0 launches nothing and returns 0, after the checks; a failure returns -1 with a text in yf_images_last_error_text.
 * Out of scope: an id the tracker itself exchanged between two faces cannot be corrected; an entry whose track the tracker still holds
 * over cannot be claimed by another track; colour descriptors and learned embeddings are not included.  The suggested max_distance is
 * a choice made on synthetic textures (profiles/reid_bench.txt); nothing is measured on labelled video. */
#define YF_DESC_GRID 8
#define YF_DESC_BYTES 64
#define YF_DESC_VALID 1u
#define YF_REID_ENTRIES 64
#define YF_REID_KNOWN 1
#define YF_REID_REIDENTIFIED 2
#define YF_REID_BORN 3
typedef struct yf_face_desc   { uint32_t flags; uint8_t v[YF_DESC_BYTES]; } yf_face_desc;                             /* 68 bytes */
typedef struct yf_reid_entry  { uint32_t id, alias, seen, flags; uint8_t v[YF_DESC_BYTES]; } yf_reid_entry;           /* 80 bytes */
typedef struct yf_reid_state  { uint32_t clock, reserved; yf_reid_entry entry[YF_REID_ENTRIES]; } yf_reid_state;     /* 5128 bytes per stream */
typedef struct yf_reid_params { int32_t max_distance, max_age, blend; } yf_reid_params;
YF_API long   yf_images_describe_records_device(const void* d_pixels, size_t pixels_bytes, int format, const yf_image* d_images,
                                                const void* d_dets, const void* d_counts, long n, int cap, int margin_permille, int flags,
                                                void* d_desc, int32_t* d_first, int32_t* d_status, void* stream);
YF_API long   yf_images_describe_records_yuv_device(const void* d_pixels, size_t pixels_bytes, int format, const yf_image_yuv* d_images,
                                                    const void* d_dets, const void* d_counts, long n, int cap, int margin_permille,
                                                    int flags, void* d_desc, int32_t* d_first, int32_t* d_status, void* stream);
YF_API size_t yf_images_reid_state_bytes(long streams);
YF_API long   yf_images_reid_device(const void* d_info, const void* d_out_counts, const void* d_desc, int out_cap, long streams, long steps,
                                    int layout, const yf_reid_params* params, void* d_state, void* d_info_out, int32_t* d_what,
                                    int32_t* d_status, void* stream);

/* ---- letterboxed frames: the picture resized with its aspect kept, centred in the square frame, the rest padded with one grey, and the
 * boxes mapped back through the same rectangle.  Every entry above stretches the picture onto the frame, as the reference's scripts do
 * (cv2.resize(img, (56, 56))); that stays the default.  Every mainstream YOLO trainer letterboxes instead, so a retrained model (.yfm, or
 * a float model quantised through yf_calib) wants such frames for inference AND for its calibration.  THE SHIPPED MODEL WAS TRAINED ON
 * STRETCHED PICTURES, and no effect of letterboxing on its accuracy has been measured: yf_images_match_device /
 * yf_images_average_precision_device score either preprocessing on labelled pictures.  The definition is this library's own, stated once
 * in csrc/yf_images_fit.h, which the kernels, a host build and a sanitizer program share.
 *   fit:    for a picture of H x W and a frame side S (56 or 160), in int64: W >= H: width = S, height = max(1, (2 H S + W) / (2 W)) --
 *           the exact ratio rounded half up --, W < H symmetric; x0 = (S - width) / 2, y0 = (S - height) / 2 (floor: the odd pixel of
 *           padding goes right and bottom, as ultralytics' LetterBox centres it).  A square picture: {0, 0, S, S}.  yf_images_fit
 *           computes it on the host: 0, or -1 with a text for sides outside [1, 16384], an out_hw that is not 56 or 160, or fit NULL.
 *   frame:  inside the rectangle frame[y0 + y][x0 + x][c] = (int8)(R[y][x][rgb(c)] - 128), R = cv2.resize(picture, (width, height))
 *           INTER_LINEAR (the arithmetic of the plain prepare at a run-time output size); outside (int8)(pad - 128), pad a byte 0..255,
 *           one grey for the three channels (the trainers use 114).  fp16 frames: fp16(v / 255.) of the same bytes.  NV12 / NV21: each
 *           sampled pixel converted first, as in the plain YUV prepare.  A padded pixel loads nothing from the picture.  For a square
 *           picture the frame equals the plain prepare's byte for byte.
 *   boxes:  the YF_DECODE_PY decode (at both grids, and of the fp16 network's float32 logits), with another tail: after the four edges in
 *           frame pixels, x = (x - (float)x0) * x_scale, y = (y - (float)y0) * y_scale in float32, one IEEE operation per step, with
 *           x_scale = (float)((double)W / (double)width), y_scale = (float)((double)H / (double)height) -- per axis, the scales the
 *           resize used --, then float32 -> int32 as every decode (truncation; out of range and NaN -> INT32_MIN).  Boxes are not
 *           clipped: an edge can land in the padding, outside the picture.  There is no firmware mode.  For a square picture the records
 *           equal the plain ragged decode's byte for byte.
 * The batches are ragged only (one descriptor per picture; a uniform batch is descriptors of one size).  d_status[i] = 1 for an invalid
 * descriptor: its frame is all -128 (fp16: zeros), its picture is never read and its count is 0.  The decodes recompute the fit from the
 * descriptor's height and width alone (a yf_image_yuv batch: a yf_image per surface with its sides); d_status may be NULL there.  True
 * counts go to d_counts, only the first cap records are written, nothing beyond min(count, cap): cap in [1, 147] at 56 and for the float
 * logits, [1, 1200] at 160.  The run_* entries are prepare, the network and the decode on `stream`; as for the plain path there is none
 * for NV12 / NV21: the frames are the interface (yf_images_prepare_fit_yuv_ragged_device, yf_network_run_device,
 * yf_images_decode_fit_ragged_device).  Calibration frames for yf_calib are these frames: INTEGRATION.md.
 * All asynchronous on `stream`, no allocation, no host synchronisation, capturable (the int8 decodes under the decode-table rule of
 * yf_images_set_decode_tables above: a first call outside capture).  Every argument is checked before the first launch -- each entry
 * refuses the other family's formats, pad outside [0, 255], out_hw other than 56 or 160, a cap out of range, NULL or misaligned
 * pointers as the plain entries do -- and n = 0 launches nothing after the checks.  Return n, or 0 and a text. */
typedef struct yf_fit { int32_t x0, y0, width, height; } yf_fit;                   /* where the picture lies in its frame */
YF_API int  yf_images_fit(int height, int width, int out_hw, yf_fit* fit);
YF_API long yf_images_prepare_fit_ragged_device(const void* d_pixels, size_t pixels_bytes, int format, const yf_image* d_images, long n,
                                                int out_hw, int pad, void* d_frames, int32_t* d_status, void* stream);
YF_API long yf_images_prepare_fit_yuv_ragged_device(const void* d_pixels, size_t pixels_bytes, int format, const yf_image_yuv* d_images,
                                                    long n, int out_hw, int pad, void* d_frames, int32_t* d_status, void* stream);
YF_API long yf_images_prepare_fit_f16_ragged_device(const void* d_pixels, size_t pixels_bytes, int format, const yf_image* d_images, long n,
                                                    int pad, void* d_frames_f16, int32_t* d_status, void* stream);
YF_API long yf_images_prepare_fit_yuv_f16_ragged_device(const void* d_pixels, size_t pixels_bytes, int format, const yf_image_yuv* d_images,
                                                        long n, int pad, void* d_frames_f16, int32_t* d_status, void* stream);
YF_API long yf_images_decode_fit_ragged_device(const void* d_heads, const yf_image* d_images, const int32_t* d_status, long n, int out_hw,
                                               void* d_dets, void* d_counts, int cap, void* stream);
YF_API long yf_images_decode_f32_fit_ragged_device(const void* d_logits, const yf_image* d_images, const int32_t* d_status, long n,
                                                   void* d_dets, void* d_counts, int cap, void* stream);
YF_API long yf_images_run_decode_fit_ragged_device(ai_handle net, const void* d_pixels, size_t pixels_bytes, int format,
                                                   const yf_image* d_images, long n, int out_hw, int pad, void* d_frames, void* d_heads,
                                                   void* d_dets, void* d_counts, int cap, int32_t* d_status, void* stream);
YF_API long yf_images_run_decode_fit_f16_ragged_device(ai_handle net, const void* d_pixels, size_t pixels_bytes, int format,
                                                       const yf_image* d_images, long n, int pad, void* d_frames_f16, void* d_logits,
                                                       void* d_dets, void* d_counts, int cap, int32_t* d_status, void* stream);

/* ---- area-averaged frames: every source pixel counted.  The resize of every entry above is cv2.resize's INTER_LINEAR, which reads four
 * source pixels per output pixel whatever the reduction; a 1920 x 1080 picture reduced to 56 x 56 then shows the network 12 544 of its
 * 2 073 600 pixels, and fine texture aliases into the frame.  These entries write the same frames with the exact area average instead.
 * LINEAR STAYS THE DEFAULT: THE SHIPPED MODEL WAS TRAINED ON LINEARLY RESIZED PICTURES and no effect of the filter on its accuracy has
 * been measured; a model calibrated (yf_calib) or trained on area-averaged frames wants them at inference too -- the same filter in
 * both places.  The definition is this library's own, integers only, stated once in csrc/yf_images_area.h, which the
 * kernels, a host build and a sanitizer program share:
 *   axis:   n_in source and n_out output positions on the grid of n_in n_out sub-positions; a(d, s) = the length of the overlap of
 *           [d n_in, (d + 1) n_in) and [s n_out, (s + 1) n_out), an integer; the a(d, .) sum to n_in.  Any ratio: reduction, enlargement,
 *           identity.
 *   pixel:  S = sum of ay(y, sy) ax(x, sx) p[sy][sx], v = (2 S + H W) / (2 H W) in 64-bit integer division: the exact average, rounded
 *           half up.  No floats, no rounded weight tables: the result does not depend on the order of addition.
 *   frame:  (int8)(v - 128), or fp16(v / 255.); RGB order, the alpha byte never read.  NV12 / NV21: every source pixel converted first (the
 *           arithmetic of the plain YUV prepare), then averaged.
 *   fit:    YF_FIT_STRETCH: the picture onto the whole frame.  YF_FIT_LETTERBOX: onto the rectangle of yf_images_fit, the rest of the frame
 *           (int8)(pad - 128) (fp16 of pad / 255.); a square picture has the same bytes either way.  pad is checked always and read only
 *           when letterboxed.  The decodes do not change: boxes map back through the fit, not through the filter -- the plain ragged
 *           decodes for YF_FIT_STRETCH, yf_images_decode_fit_ragged_device / yf_images_decode_f32_fit_ragged_device for YF_FIT_LETTERBOX.
 *   cv2:    for integer ratios v is the rounded block mean, INTER_AREA's integer path (at exactly 2x (a + b + c + d + 2) >> 2, the linear
 *           prepare's bytes); for other ratios OpenCV accumulates float weights and this is the exact value they approximate.  Not
 *           pinned against a real cv2.
 * The batches are ragged only (a uniform batch is descriptors of one size) and there are no run_* forms: the frames are the interface, as
 * for NV12 / NV21.  The work grows with the source pictures, not with the frames: a frame is split into bands of whole output rows, one
 * job per (frame, band), yf_images_area_bands(n, out_hw) bands per frame -- from n and out_hw alone, the sizes live in device memory --
 * and the frames do not depend on the split.  d_status[i] = 1 for an invalid descriptor: its frame is all -128 (fp16: zeros) and its
 * picture is never read.  No load touches a byte outside a picture's own extent: 16-byte loads lie wholly inside a row's width * C bytes,
 * unaligned heads and tails are read byte by byte, and no alignment is asked of offsets or strides.  Asynchronous on `stream`, no
 * allocation, no host synchronisation, capturable.  Every argument is checked before the first launch -- each entry refuses the other
 * family's formats, an out_hw other than 56 or 160, a fit other than the two, pad outside [0, 255], NULL or misaligned pointers as the
 * letterbox entries do -- and n = 0 launches nothing after the checks.  Return n, or 0 and a text. */
enum { YF_FIT_STRETCH = 0, YF_FIT_LETTERBOX = 1 };
YF_API int  yf_images_area_bands(long n, int out_hw);          /* bands per frame of a batch of n; 0 for n < 0 or another out_hw */
YF_API long yf_images_prepare_area_ragged_device(const void* d_pixels, size_t pixels_bytes, int format, const yf_image* d_images, long n,
                                                 int out_hw, int fit, int pad, void* d_frames, int32_t* d_status, void* stream);
YF_API long yf_images_prepare_area_yuv_ragged_device(const void* d_pixels, size_t pixels_bytes, int format, const yf_image_yuv* d_images,
                                                     long n, int out_hw, int fit, int pad, void* d_frames, int32_t* d_status, void* stream);
YF_API long yf_images_prepare_area_f16_ragged_device(const void* d_pixels, size_t pixels_bytes, int format, const yf_image* d_images, long n,
                                                     int fit, int pad, void* d_frames_f16, int32_t* d_status, void* stream);
YF_API long yf_images_prepare_area_yuv_f16_ragged_device(const void* d_pixels, size_t pixels_bytes, int format, const yf_image_yuv* d_images,
                                                         long n, int fit, int pad, void* d_frames_f16, int32_t* d_status, void* stream);

YF_API const char* yf_images_last_error_text(void);
/* sha256 prefix over the library's sources and flags (csrc/Makefile IMAGES_SRCS), checked by images.py before it loads an existing file */
YF_API const char* yf_images_build_id(void);

#ifdef __cplusplus
}
#endif
#endif
