"""ctypes binding of libyf_images.so (include/yf_images.h): decoded images of any size -> the network's int8 frames, resized exactly as
`cv2.resize(img, (out, out))` (INTER_LINEAR) computes -- "exactly" meaning bit-exact against `ptq.resize_linear_u8`, a restatement of OpenCV 4's
imgproc/resize.cpp that has not been pinned against a real cv2 -- and on through the network to boxes in each image's own pixels.

`detect(network, images)` is lines 29-61 of the reference's yoloface/tflite/tflite_prediction.py for a whole batch: imread (BGR), BGR -> RGB,
cv2.resize to 56x56, minus 128, int8, the network, decode, boxes scaled by W/56. and H/56.  With `iou_threshold` it adds the greedy IoU
suppression of yoloface/tensorflow/yoloface_test.py:145-190 on the GPU (`nms_device`, include/yf_images.h).  `size=160` runs the same path
on 160x160 frames (20x20 heads, 1200 candidates per image: `run_decode160_ragged_device`, `nms_wide_device`).  `dtype="fp16"` runs the fp16
network instead, as the reference's float caller yoloface/tensorflow/h5_predition.py:29-73 does: fp16 frames of pixel / 255., float32 logits,
the decode in float32 (`run_decode_f16_ragged_device`; the arithmetic: csrc/yf_images_float.h).

`evaluate(network, images, ground_truths)` scores those boxes against labelled ones as the reference's training script does
(yoloface/tensorflow/yolov3_train_tf.py:657-759, calculate_iou / calculate_ap / calculate_map): `match_device` and
`average_precision_device` on the same stream, without the records leaving the GPU (the arithmetic: csrc/yf_images_eval.h).

`detect_tiled(network, images, tile)` runs a large picture as overlapping tiles, each one a frame of the network, and makes the tiles'
records one picture's records again on the GPU: `plan_tiles` (the grid), the ragged run over the tile descriptors, `gather_tiles_device`
(merge and translation), `nms_wide_device` across the tile borders.  The reference has no tiling; the definition is the library's own
(csrc/yf_images_tiles.h).

`detect_chips(network, images)` goes one step past the boxes, where the reference stops at cv2.rectangle: every kept box is cut out of its
picture and resized to one fixed size on the GPU, from the pixels (or the NV12 / NV21 surface) that are already there --
`crop_records_device`, `crop_records_yuv_device`; the region rule is the library's own (csrc/yf_images_crop.h, `ptq.crop_region`).

`detect_redacted(network, images)` is the write side of the boxes: every kept box is pixelated (a block mosaic) or filled with one colour
in its picture on the GPU, packed pixels or an NV12 / NV21 surface, and the redacted pictures come back in the caller's shapes --
`redact_records_device`, `redact_records_yuv_device`; the definition is the library's own (csrc/yf_images_redact.h, `ptq.redact_u8`,
`ptq.redact_yuv420sp`).

`detect_blurred(network, images)` hides the boxes the soft way, the one video anonymisers use by default: every kept box becomes a coarse
grid of its own means resized back to the box, so that every face gets the same number of cells whatever its size --
`blur_records_device`, `blur_records_yuv_device`, `blur_workspace`; the definition is the library's own (csrc/yf_images_blur.h,
`ptq.blur_u8`, `ptq.blur_yuv420sp`).

`detect_drawn(network, images)` is the line every script of the reference ends with, cv2.rectangle(img, (x1, y1), (x2, y2), (0, 0, 255), 2)
(tflite_prediction.py:59-64), for the whole batch on the GPU: the outline of every kept box drawn in place, in one colour or -- with a
`Tracker` -- in a colour per track that a face keeps over the frames; `draw_records_device`, `draw_records_yuv_device`; the definition:
csrc/yf_images_draw.h, `ptq.draw_rectangles_u8`, `ptq.draw_rectangles_yuv420sp`.

`detect_tracked(network, images, tracker, steps)` is the step a video needs between the boxes of a frame and what is done with the frame:
a `Tracker` keeps per-stream track state on the device and associates each frame's kept boxes with it, so that every face has an identity
over the frames and a face the detector misses for a few frames is held over with its last box -- `track_device`; its output is records
again, which `crop_records_device` and `redact_records_device` take as they are.  The reference has no tracker; the definition is the
library's own (csrc/yf_images_track.h, `ptq.track_step`).

`Tracker(..., motion=True)` adds a motion model to that step: a constant-velocity g-h (alpha-beta) filter on every edge of a track's box,
in integers, so that the box of a held-over track moves on with the velocity the track had and the match is taken against the PREDICTED
box -- a moving face stays hidden on the frames the detector misses it, and keeps its id when it is seen again -- `track_motion_device`,
`track_motion_state_bytes`, `YfTrackMotionParams`; a second entry with a larger state (7176 bytes per stream against 2824) beside the
first, which does not change; the definition is the library's own (csrc/yf_images_motion.h, `ptq.track_motion_step`).  The gains
(alpha, beta, damp) are in 1/256; `MOTION_GAINS` = (192, 128, 256) is the library's suggestion, a choice and not a measurement: there is
no accuracy or identity-switch figure for real video -- what exists since is `evaluate_tracking` / `TrackScore` (below) and their figures
on synthetic clips, profiles/track_score_bench.txt.  (256, 0, any) is the tracker without the model, byte for byte.  Still out of scope:
a covariance (a Kalman filter) and clamping a predicted box to the picture (the crop, the redaction, the blur and the drawing clip
themselves); appearance and re-identification are `ReId`'s (below).  `Tracker(..., assign="optimal")` replaces the greedy match -- repeatedly the pair
of the largest IoU, which strands a detection where two faces pass each other -- by the maximum-weight assignment over the eligible
pairs, `track_motion_assign_device` (csrc/yf_images_assign.h, `ptq.track_assign_match`); it runs on the 7176-byte state with or
without `motion`.  `detect_tracked`, `detect_drawn`, `detect_redacted` and `detect_blurred`
take such a tracker as they take the plain one; with a tracker the last two hide the REPORTED TRACKS, held-over ones included.

`evaluate_tracking(network, images, ground_truths, tracker, steps)` scores what a tracker reports against labelled identities -- the
CLEAR-MOT score (Bernardin and Stiefelhagen, 2008): misses, false positives, identity switches, MOTA, MOTP -- on the device, per stream
over the steps of a clip, without the records leaving it: `TrackScore`, `score_tracks_device`, `score_state_bytes`, `score_summary`,
`pack_track_truth`; the definition is the library's own (csrc/yf_images_score.h, `ptq.track_score_step`, `ptq.track_score_summary`).  It
is what measures the tracker's settings against each other; the figures that exist are those of synthetic clips
(profiles/track_score_bench.txt), none of labelled video.  Out of scope: IDF1, HOTA, fragmentations, more than 256 labelled objects per
stream or 64 per frame.

`ReId(streams)` is the second look at the picture behind a tracker: `describe_records_device` gives every reported box an appearance
descriptor -- its region as an 8 x 8 grid of mean luma, a tiny template and not a learned embedding (csrc/yf_images_describe.h,
`ptq.describe_u8`) -- and `reid_device` rewrites the tracker's ids, so that a track born while a lost one that looks the same is still
remembered reports the lost one's id (csrc/yf_images_reid.h, `ptq.reid_step`): a face hidden for longer than max_misses steps keeps its
identity, which no setting of the tracker alone achieves.  `detect_tracked`, `detect_drawn` and `evaluate_tracking` take `reid=`.  The
stage takes any 64 bytes per record, so a recogniser's embedding quantised to uint8 can stand in for the template.  `REID_MAX_DISTANCE`
is a choice made on synthetic textures (profiles/reid_bench.txt); nothing is measured on labelled video.  Out of scope: an id the
tracker itself exchanged between two faces, an entry whose track the tracker still holds over, colour descriptors, learned embeddings.

`fit="letterbox"` on `detect`, every `detect_*` call and `evaluate` replaces the stretch onto the square frame by what every mainstream
YOLO trainer does: the picture resized with its aspect kept into a centred rectangle of the frame (`fit_of`), the rest padded with the
grey `pad`, and the boxes mapped back through the same rectangle -- `prepare_fit_*`, `decode_fit_ragged_device`,
`decode_f32_fit_ragged_device`, `run_decode_fit_*`; the definition is the library's own (csrc/yf_images_fit.h, `ptq.letterbox_fit`,
`ptq.letterbox_u8`).  It is for retrained models and their calibration frames: the shipped model was trained on stretched pictures, and
what letterboxing does to its accuracy has not been measured.  fit="stretch", the default, is every call as it was.

`interp="area"` on the same calls replaces the filter of that resize: cv2.resize's INTER_LINEAR reads four source pixels per output pixel
whatever the reduction (12 544 of the 2 073 600 pixels of a 1920 x 1080 picture reach a 56 x 56 frame, and fine texture aliases), the area
average counts every source pixel with the share of it an output pixel covers, exactly, in integers -- `prepare_area_*`, `area_bands`; the
definition is the library's own (csrc/yf_images_area.h, `ptq.resize_area_u8`).  It combines with either fit, both sizes, both dtypes,
packed pictures, NV12 / NV21 surfaces and tiles.  The shipped model was trained on linearly resized pictures and what the filter does to
its accuracy has not been measured; calibration frames must be made with the filter the deployed pipeline uses.  interp="linear", the
default, is every call as it was.

All of these start alike: `_stage` packs the batch and launches images -> records on the device's current stream, and what it returns
(`_Batch`: the records, the pixels, the pictures' descriptors, the stream) is what a call's own stage is launched on.

NV12 / NV21 surfaces -- 4:2:0 semi-planar, what hardware video and JPEG decoders write and what `detect_video` of the reference's
yoloface/tensorflow/yoloface_test.py:318-385 has behind cv2.VideoCapture -- are read where they lie: `pack_yuv_images`, the four
`prepare_yuv_*` bindings, and `detect` / `evaluate` with fmt="nv12" or "nv21".  The frame of a surface is the frame of
`cv2.cvtColor(yuv, cv2.COLOR_YUV2BGR_NV12)` under the BGR path, bit-exact against `ptq.yuv420sp_to_rgb_u8` (a restatement of OpenCV 4's
color_yuv.simd.hpp, BT.601 limited range, not pinned against a real cv2; the arithmetic: csrc/yf_images_yuv.h).  Out of scope: YUYV / UYVY,
I420, BT.709, full-range variants, odd-sided surfaces, and tiling (`detect_tiled`, `evaluate(tile=...)`: a tile's origin would have to be even).
"""
import ctypes
import dataclasses
import os

import numpy as np

from . import binding, libs

YF_PIX_BGR8, YF_PIX_RGB8, YF_PIX_BGRA8, YF_PIX_RGBA8 = 0, 1, 2, 3
YF_PIX_NV12, YF_PIX_NV21 = 4, 5        # 4:2:0 semi-planar, BT.601 limited range; not YUYV / UYVY, I420, BT.709, full range or odd sides
FORMATS = {"bgr": YF_PIX_BGR8, "rgb": YF_PIX_RGB8, "bgra": YF_PIX_BGRA8, "rgba": YF_PIX_RGBA8, "nv12": YF_PIX_NV12, "nv21": YF_PIX_NV21}
YUV_FORMATS = (YF_PIX_NV12, YF_PIX_NV21)
CHANNELS = {YF_PIX_BGR8: 3, YF_PIX_RGB8: 3, YF_PIX_BGRA8: 4, YF_PIX_RGBA8: 4}
MAX_SIDE = 16384
NMS_MAX_CAP = 256
NMS_WIDE_MAX_CAP = 1200
GRID160, CAND160 = 20, 1200
FRAME_BYTES = {56: 56 * 56 * 3, 160: 160 * 160 * 3}
EVAL_MAX_GT = 256
EVAL_SORT_TILE = 1024            # records per tile of average_precision_device's sort (YF_IMAGES_EVAL_SORT_TILE; checked in load())


class YfImage(ctypes.Structure):
    _fields_ = [("offset", ctypes.c_uint64), ("height", ctypes.c_int32), ("width", ctypes.c_int32), ("row_stride", ctypes.c_int64)]


IMAGE_DTYPE = np.dtype([("offset", "<u8"), ("height", "<i4"), ("width", "<i4"), ("row_stride", "<i8")])
assert IMAGE_DTYPE.itemsize == ctypes.sizeof(YfImage) == 24


# an NV12 / NV21 surface of a ragged batch (yf_image_yuv)
YUV_IMAGE_DTYPE = np.dtype([("offset_y", "<u8"), ("offset_uv", "<u8"), ("height", "<i4"), ("width", "<i4"), ("stride_y", "<i8"),
                            ("stride_uv", "<i8")])
assert YUV_IMAGE_DTYPE.itemsize == 40


# a tile of an image (yf_tile): the image's index, the tile's origin in the image's pixels and its size
TILE_DTYPE = np.dtype([("image", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("height", "<i4"), ("width", "<i4")])
assert TILE_DTYPE.itemsize == 20


# the info row of a face chip (yf_chip): its frame and slot, the region actually sampled, and the status (0 a chip, 1 an empty region,
# 2 the picture's descriptor is invalid)
CHIP_DTYPE = np.dtype([("frame", "<i4"), ("slot", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("width", "<i4"), ("height", "<i4"), ("status", "<i4")])
assert CHIP_DTYPE.itemsize == 28
YF_CROP_SQUARE = 1
ORDERS, ORDER_WHAT = {"rgb": YF_PIX_RGB8, "bgr": YF_PIX_BGR8}, "order {!r}: 'rgb' or 'bgr'"
YF_REDACT_MOSAIC, YF_REDACT_FILL = 0, 1
REDACT_MODES, MODE_WHAT = {"mosaic": YF_REDACT_MOSAIC, "fill": YF_REDACT_FILL}, "mode {!r}: 'mosaic' or 'fill'"
BLUR_MAX_GRID, BLUR_MIN_CELL = 16, 4   # YF_BLUR_MAX_GRID, YF_BLUR_MIN_CELL


# the tracker (yf_track_params, yf_track_info, yf_track_state): 64 slots per stream, at most 64 detections of a frame count
class YfTrackParams(ctypes.Structure):
    _fields_ = [("match_iou", ctypes.c_double), ("min_hits", ctypes.c_int32), ("max_misses", ctypes.c_int32)]


TRACK_INFO_DTYPE = np.dtype([("id", "<u4"), ("hits", "<i4"), ("misses", "<i4"), ("age", "<i4")])
TRACK_SLOTS, TRACK_STATE_BYTES = 64, 2824
assert TRACK_INFO_DTYPE.itemsize == 16 and ctypes.sizeof(YfTrackParams) == 16
YF_TRACK_TIME_MAJOR, YF_TRACK_STREAM_MAJOR = 0, 1
TRACK_LAYOUTS = {"time": YF_TRACK_TIME_MAJOR, "stream": YF_TRACK_STREAM_MAJOR}
LAYOUT_WHAT = "layout {!r}: 'time' (frame t * streams + s) or 'stream' (frame s * steps + t)"
YF_TRACK_CLIPPED, YF_TRACK_DROPPED = 1, 2      # the bits of a frame's status


# the tracker with a motion model (yf_track_motion_params, yf_track_motion_state): a slot is the tracker's 44 bytes, 4 of padding and
# pos[4], vel[4] (int64, 1/256 pixel); gains in 1/256
class YfTrackMotionParams(ctypes.Structure):
    _fields_ = [("base", YfTrackParams), ("alpha", ctypes.c_int32), ("beta", ctypes.c_int32), ("damp", ctypes.c_int32), ("smooth", ctypes.c_int32)]


TRACK_MOTION_STATE_BYTES = 7176
MOTION_GAINS = (192, 128, 256)                 # (alpha, beta, damp): the library's suggestion -- a choice, not a measurement
assert ctypes.sizeof(YfTrackMotionParams) == 32
# the match of the tracker with a motion model (yf_images_track_motion_assign_device): the global greedy one, or the optimal assignment
YF_ASSIGN_GREEDY, YF_ASSIGN_OPTIMAL = 0, 1
ASSIGNS = {"greedy": YF_ASSIGN_GREEDY, "optimal": YF_ASSIGN_OPTIMAL}
ASSIGN_NAMES = {code: name for name, code in ASSIGNS.items()}
ASSIGN_WHAT = "assign {!r}: 'greedy' (repeatedly the pair of the largest IoU) or 'optimal' (the maximum total IoU)"
# the score of tracks against labelled identities (yf_gt_track, yf_score_state, yf_score_summary): at most 64 labelled objects of a frame
# count, their ids 1 .. 256
SCORE_MAX_IDS, SCORE_MAX_GT, SCORE_STATE_BYTES = 256, 64, 3136
SCORE_COUNTERS = ("frames", "gt", "hyp", "matches", "misses", "false_positives", "switches", "overlap")
GT_TRACK_DTYPE = np.dtype([("id", "<u4"), ("x1", "<i4"), ("y1", "<i4"), ("x2", "<i4"), ("y2", "<i4")])
SCORE_STATE_DTYPE = np.dtype([(name, "<u8") for name in SCORE_COUNTERS]
                             + [("last", "<u4", (SCORE_MAX_IDS,)), ("present", "<i4", (SCORE_MAX_IDS,)), ("tracked", "<i4", (SCORE_MAX_IDS,))])
SCORE_SUMMARY_DTYPE = np.dtype([(name, "<u8") for name in SCORE_COUNTERS]
                               + [("objects", "<i8"), ("mostly_tracked", "<i8"), ("mostly_lost", "<i8"), ("mota", "<f8"), ("motp", "<f8")])
assert GT_TRACK_DTYPE.itemsize == 20 and SCORE_STATE_DTYPE.itemsize == SCORE_STATE_BYTES and SCORE_SUMMARY_DTYPE.itemsize == 104
YF_SCORE_GT_CLIPPED, YF_SCORE_HYP_CLIPPED, YF_SCORE_GT_VOID, YF_SCORE_HYP_VOID = 1, 2, 4, 8      # the bits of a frame's status


# appearance descriptors and re-identification (yf_face_desc, yf_reid_entry, yf_reid_state, yf_reid_params): an 8 x 8 grid of mean luma
# per record, a table of 64 identities per stream
class YfReidParams(ctypes.Structure):
    _fields_ = [("max_distance", ctypes.c_int32), ("max_age", ctypes.c_int32), ("blend", ctypes.c_int32)]


DESC_BYTES, REID_ENTRIES, REID_STATE_BYTES = 64, 64, 5128
FACE_DESC_DTYPE = np.dtype([("flags", "<u4"), ("v", "u1", (DESC_BYTES,))])
REID_ENTRY_DTYPE = np.dtype([("id", "<u4"), ("alias", "<u4"), ("seen", "<u4"), ("flags", "<u4"), ("v", "u1", (DESC_BYTES,))])
REID_STATE_DTYPE = np.dtype([("clock", "<u4"), ("reserved", "<u4"), ("entry", REID_ENTRY_DTYPE, (REID_ENTRIES,))])
assert FACE_DESC_DTYPE.itemsize == 68 and REID_ENTRY_DTYPE.itemsize == 80 and REID_STATE_DTYPE.itemsize == REID_STATE_BYTES
assert ctypes.sizeof(YfReidParams) == 12
YF_REID_CLIPPED, YF_REID_VOID = 1, 2           # the bits of a frame's status
YF_REID_KNOWN, YF_REID_REIDENTIFIED, YF_REID_BORN = 1, 2, 3
# the library's suggestion for ReId: A CHOICE MADE ON SYNTHETIC TEXTURES, between the largest same-face distance (62528) and the
# smallest different-face distance (79244) that tools/reid_bench.py saw on its clips (profiles/reid_bench.txt) -- not a figure from
# labelled video
REID_MAX_DISTANCE = 70000
REID_MAX_AGE, REID_BLEND = 300, 64              # ten seconds at 30 frames a second; a quarter of the new descriptor per frame: choices


# a ground-truth box (yf_gt_box) and the result of average_precision_device (yf_eval_result)
# where a picture lies in its letterboxed frame (yf_fit), and the two ways a picture becomes a frame
FIT_DTYPE = np.dtype([("x0", "<i4"), ("y0", "<i4"), ("width", "<i4"), ("height", "<i4")])
FITS, FIT_WHAT = ("stretch", "letterbox"), "fit {!r}: 'stretch' (cv2.resize onto the frame) or 'letterbox' (the aspect kept, the rest padded)"
# the filter of the resize: cv2.resize's INTER_LINEAR (four source pixels per output pixel), or the exact area average of every source pixel
INTERPS, INTERP_WHAT = ("linear", "area"), "interp {!r}: 'linear' (cv2.resize's INTER_LINEAR) or 'area' (every source pixel averaged)"
YF_FIT_STRETCH, YF_FIT_LETTERBOX = 0, 1
GT_DTYPE = np.dtype([("x1", "<f8"), ("y1", "<f8"), ("x2", "<f8"), ("y2", "<f8")])
EVAL_RESULT_DTYPE = np.dtype([("ap", "<f8"), ("detections", "<i8"), ("ground_truths", "<i8"), ("true_positives", "<i8")])
assert GT_DTYPE.itemsize == 32 and EVAL_RESULT_DTYPE.itemsize == 32


class ImagesError(RuntimeError):
    pass


def lib_path():
    """libyf_images.so sits beside the libyf_network.so that binding loads (its rpath $ORIGIN finds that one)."""
    return os.path.join(os.path.dirname(binding.LIB_PATH), "libyf_images.so")


def _images_srcs():
    return libs.make_var("IMAGES_SRCS").split()


def expected_build_id():
    """The id csrc/Makefile bakes into libyf_images.so (yf_images_build_id): sha256 over IMAGES_SRCS and flags.mk."""
    return libs.source_id(_images_srcs() + ["flags.mk"], "")


def library_is_current():
    """True when the in-tree libyf_images.so can be loaded without running make: it is newer than its sources, the Makefile, flags.mk and
    the libyf_network.so it links against.  Its baked-in id is still checked after loading."""
    return libs.newer_than(lib_path(), _images_srcs() + ["Makefile", "flags.mk", binding.LIB_PATH])


def _entries():
    """yf_images_<name> -> argument types, for every entry point that returns the number of frames it took (a long): include/yf_images.h"""
    vp, cl, ci, cs, cf, cd = ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_size_t, ctypes.c_float, ctypes.c_double
    uniform = [vp, cs, ci, ci, ci, cl, cl, cl]          # d_pixels, pixels_bytes, format, height, width, row_stride, frame_stride, n
    ragged = [vp, cs, ci, vp, cl]                       # d_pixels, pixels_bytes, format, d_images, n
    nms = [vp, vp, cl, ci, cd, vp, vp, vp]
    return {
        "prepare_device": uniform + [ci, vp, vp],
        "prepare_ragged_device": ragged + [ci, vp, vp, vp],
        # d_pixels, pixels_bytes, format, height, width, stride_y, uv_offset, stride_uv, frame_stride, n
        "prepare_yuv_device": [vp, cs, ci, ci, ci, cl, cl, cl, cl, cl] + [ci, vp, vp],
        "prepare_yuv_ragged_device": ragged + [ci, vp, vp, vp],
        "prepare_yuv_f16_device": [vp, cs, ci, ci, ci, cl, cl, cl, cl, cl] + [vp, vp],
        "prepare_yuv_f16_ragged_device": ragged + [vp, vp, vp],
        "run_decode_device": [vp] + uniform + [vp, vp, ci, vp, vp, ci, vp],
        "run_decode_ragged_device": [vp] + ragged + [vp, vp, ci, vp, vp, ci, vp, vp],
        "decode_ragged_device": [vp, vp, cl, ci, vp, vp, ci, vp],
        "nms_device": nms,
        "decode160_device": [vp, cl, cf, cf, vp, vp, ci, vp],
        "decode160_ragged_device": [vp, vp, vp, cl, vp, vp, ci, vp],
        "run_decode160_device": [vp] + uniform + [vp, vp, vp, vp, ci, vp],
        "run_decode160_ragged_device": [vp] + ragged + [vp, vp, vp, vp, ci, vp, vp],
        "nms_wide_device": nms,
        "prepare_f16_device": uniform + [vp, vp],
        "prepare_f16_ragged_device": ragged + [vp, vp, vp],
        "decode_f32_device": [vp, cl, cf, cf, vp, vp, ci, vp],
        "decode_f32_ragged_device": [vp, vp, vp, cl, vp, vp, ci, vp],
        "run_decode_f16_device": [vp] + uniform + [vp, vp, vp, vp, ci, vp],
        "run_decode_f16_ragged_device": [vp] + ragged + [vp, vp, vp, vp, ci, vp, vp],
        "match_device": [vp, vp, cl, ci, vp, vp, ci, cd, vp, vp, vp],
        "average_precision_device": [vp, vp, vp, cl, ci, vp, ci, vp, cs, vp, vp, vp],
        "plan_tiles": [vp, cl, ci, ci, ci, ci, ci, ci, vp, vp, vp, cl],
        "gather_tiles_device": [vp, vp, cl, ci, vp, vp, cl, vp, vp, ci, vp, cs, vp],
        # d_pixels, pixels_bytes, format, d_images, d_dets, d_counts, n, cap, out_h, out_w, out_format, margin_permille, flags, d_chips,
        # chips_cap, d_first, d_info, stream
        "crop_records_device": [vp, cs, ci, vp, vp, vp, cl, ci, ci, ci, ci, ci, ci, vp, cl, vp, vp, vp],
        "crop_records_yuv_device": [vp, cs, ci, vp, vp, vp, cl, ci, ci, ci, ci, ci, ci, vp, cl, vp, vp, vp],
        # d_pixels, pixels_bytes, format, d_images, d_dets, d_counts, n, cap, mode, block, colour, margin_permille, flags, d_first, d_status,
        # stream
        "redact_records_device": [vp, cs, ci, vp, vp, vp, cl, ci, ci, ci, ctypes.c_uint32, ci, ci, vp, vp, vp],
        "redact_records_yuv_device": [vp, cs, ci, vp, vp, vp, cl, ci, ci, ci, ctypes.c_uint32, ci, ci, vp, vp, vp],
        # d_pixels, pixels_bytes, format, d_images, d_dets, d_counts, n, cap, grid, colour, margin_permille, flags, d_work, work_bytes,
        # records_cap, d_first, d_status, stream
        "blur_records_device": [vp, cs, ci, vp, vp, vp, cl, ci, ci, ctypes.c_uint32, ci, ci, vp, cs, cl, vp, vp, vp],
        "blur_records_yuv_device": [vp, cs, ci, vp, vp, vp, cl, ci, ci, ctypes.c_uint32, ci, ci, vp, cs, cl, vp, vp, vp],
        # d_pixels, pixels_bytes, format, d_images, d_dets, d_counts, n, cap, half, colour, d_keys, key_stride, d_palette, palette_n, d_first,
        # d_status, stream
        "draw_records_device": [vp, cs, ci, vp, vp, vp, cl, ci, ci, ctypes.c_uint32, vp, ci, vp, ci, vp, vp, vp],
        "draw_records_yuv_device": [vp, cs, ci, vp, vp, vp, cl, ci, ci, ctypes.c_uint32, vp, ci, vp, ci, vp, vp, vp],
        # d_dets, d_counts, streams, steps, layout, cap, params, d_state, d_out, d_info, d_out_counts, out_cap, d_status, stream
        "track_device": [vp, vp, cl, cl, ci, ci, vp, vp, vp, vp, vp, ci, vp, vp],
        "track_motion_device": [vp, vp, cl, cl, ci, ci, vp, vp, vp, vp, vp, ci, vp, vp],
        # ... with assign after params
        "track_motion_assign_device": [vp, vp, cl, cl, ci, ci, vp, ci, vp, vp, vp, vp, ci, vp, vp],
        # d_out, d_info, d_out_counts, out_cap, d_gt, d_gt_counts, gt_cap, streams, steps, layout, score_iou, d_state, d_match, d_status, stream
        "score_tracks_device": [vp, vp, vp, ci, vp, vp, ci, cl, cl, ci, cd, vp, vp, vp, vp],
        # d_pixels, pixels_bytes, format, d_images, d_dets, d_counts, n, cap, margin_permille, flags, d_desc, d_first, d_status, stream
        "describe_records_device": [vp, cs, ci, vp, vp, vp, cl, ci, ci, ci, vp, vp, vp, vp],
        "describe_records_yuv_device": [vp, cs, ci, vp, vp, vp, cl, ci, ci, ci, vp, vp, vp, vp],
        # d_info, d_out_counts, d_desc, out_cap, streams, steps, layout, params, d_state, d_info_out, d_what, d_status, stream
        "reid_device": [vp, vp, vp, ci, cl, cl, ci, vp, vp, vp, vp, vp, vp],
        # letterboxed frames: d_pixels, pixels_bytes, format, d_images, n, [out_hw,] pad, d_frames, d_status, stream
        "prepare_fit_ragged_device": ragged + [ci, ci, vp, vp, vp],
        "prepare_fit_yuv_ragged_device": ragged + [ci, ci, vp, vp, vp],
        "prepare_fit_f16_ragged_device": ragged + [ci, vp, vp, vp],
        "prepare_fit_yuv_f16_ragged_device": ragged + [ci, vp, vp, vp],
        "decode_fit_ragged_device": [vp, vp, vp, cl, ci, vp, vp, ci, vp],
        "decode_f32_fit_ragged_device": [vp, vp, vp, cl, vp, vp, ci, vp],
        "run_decode_fit_ragged_device": [vp] + ragged + [ci, ci, vp, vp, vp, vp, ci, vp, vp],
        "run_decode_fit_f16_ragged_device": [vp] + ragged + [ci, vp, vp, vp, vp, ci, vp, vp],
        # area-averaged frames: d_pixels, pixels_bytes, format, d_images, n, [out_hw,] fit, pad, d_frames, d_status, stream
        "prepare_area_ragged_device": ragged + [ci, ci, ci, vp, vp, vp],
        "prepare_area_yuv_ragged_device": ragged + [ci, ci, ci, vp, vp, vp],
        "prepare_area_f16_ragged_device": ragged + [ci, ci, vp, vp, vp],
        "prepare_area_yuv_f16_ragged_device": ragged + [ci, ci, vp, vp, vp],
    }


_ENTRIES = _entries()
_lib = None


def load():
    """dlopen libyf_images.so after libyf_network.so (binding.load() first: one HIP runtime per process, binding._one_hip_runtime), rebuilding
    it when its sources are newer; an existing file is used without a build only if it is current and carries the expected id."""
    global _lib
    if _lib is not None:
        return _lib
    binding.load()
    path = lib_path()
    # (a YF_LIB_PATH override of the network library: its sibling, unchecked like binding.load; `make all` builds both libraries)
    lib = libs.open_library(path, library_is_current, [("yf_images_build_id", expected_build_id)], unchecked_override=True)
    lib.yf_images_build_id.restype = ctypes.c_char_p
    lib.yf_images_build_id.argtypes = []
    for name, argtypes in _ENTRIES.items():
        fn = getattr(lib, "yf_images_" + name)
        fn.restype, fn.argtypes = ctypes.c_long, argtypes
    lib.yf_images_last_error_text.restype = ctypes.c_char_p
    lib.yf_images_last_error_text.argtypes = []
    lib.yf_images_set_decode_tables.restype = ctypes.c_int
    lib.yf_images_set_decode_tables.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
    lib.yf_images_average_precision_workspace.restype = ctypes.c_size_t
    lib.yf_images_average_precision_workspace.argtypes = [ctypes.c_long, ctypes.c_int]
    lib.yf_images_blur_workspace.restype = ctypes.c_size_t
    lib.yf_images_blur_workspace.argtypes = [ctypes.c_long, ctypes.c_int]
    lib.yf_images_track_state_bytes.restype = ctypes.c_size_t
    lib.yf_images_track_state_bytes.argtypes = [ctypes.c_long]
    lib.yf_images_track_motion_state_bytes.restype = ctypes.c_size_t
    lib.yf_images_track_motion_state_bytes.argtypes = [ctypes.c_long]
    lib.yf_images_score_state_bytes.restype = ctypes.c_size_t
    lib.yf_images_score_state_bytes.argtypes = [ctypes.c_long]
    lib.yf_images_reid_state_bytes.restype = ctypes.c_size_t
    lib.yf_images_reid_state_bytes.argtypes = [ctypes.c_long]
    lib.yf_images_score_summary.restype = ctypes.c_int
    lib.yf_images_score_summary.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p]
    lib.yf_images_gather_tiles_workspace.restype = ctypes.c_size_t
    lib.yf_images_gather_tiles_workspace.argtypes = [ctypes.c_long]
    lib.yf_images_fit.restype = ctypes.c_int
    lib.yf_images_fit.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.yf_images_area_bands.restype = ctypes.c_int
    lib.yf_images_area_bands.argtypes = [ctypes.c_long, ctypes.c_int]
    lib.yf_images_eval_sort_tile.restype = ctypes.c_int
    lib.yf_images_eval_sort_tile.argtypes = []
    if lib.yf_images_eval_sort_tile() != EVAL_SORT_TILE:
        raise RuntimeError(f"{path}: sort tile {lib.yf_images_eval_sort_tile()}, images.EVAL_SORT_TILE says {EVAL_SORT_TILE}")
    _lib = lib
    return lib


def format_code(fmt):
    if isinstance(fmt, str):
        if fmt.lower() not in FORMATS:
            raise ValueError(f"format {fmt!r}: one of {sorted(FORMATS)}")
        return FORMATS[fmt.lower()]
    if int(fmt) not in CHANNELS and int(fmt) not in YUV_FORMATS:
        raise ValueError(f"format {fmt!r}: one of YF_PIX_BGR8, YF_PIX_RGB8, YF_PIX_BGRA8, YF_PIX_RGBA8, YF_PIX_NV12, YF_PIX_NV21")
    return int(fmt)


def is_yuv(fmt):
    return format_code(fmt) in YUV_FORMATS


def _packed_code(fmt, what):
    """the code of a packed format; NV12 / NV21 have no pixels of C bytes"""
    code = format_code(fmt)
    if code in YUV_FORMATS:
        raise ValueError(f"{what}: format {fmt!r} is a two-plane surface; {what} takes {sorted(k for k, v in FORMATS.items() if v in CHANNELS)}"
                         " (NV12 / NV21: pack_yuv_images, prepare_yuv_*; tiles of such surfaces are not supported)")
    return code


def pack_images(images, fmt="bgr", align=16):
    """uint8 images [H, W, C] (arrays or views, C = 3 or 4 as `fmt` says) -> (pixels uint8[bytes], descriptors IMAGE_DTYPE[n]).
    An image whose pixels lie packed along its rows (channel stride 1, pixel stride C) keeps its row stride, so a crop of a larger picture is
    copied as the span from its first to its last pixel, parent row stride and all; any other layout is made contiguous first.  Every image
    starts on an `align`-byte boundary.  Negative strides are refused."""
    code = _packed_code(fmt, "pack_images")
    C = CHANNELS[code]
    spans, desc, off = [], np.zeros(len(images), IMAGE_DTYPE), 0
    for i, img in enumerate(images):
        a = np.asarray(img)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != C:
            raise ValueError(f"image {i}: expected uint8 [H, W, {C}] for format {fmt!r}, got {a.dtype} {a.shape}")
        h, w = a.shape[:2]
        if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
            raise ValueError(f"image {i}: {h}x{w} is outside 1..{MAX_SIDE} per side")
        if any(s < 0 for s in a.strides):
            raise ValueError(f"image {i}: negative strides {a.strides} (flip with np.ascontiguousarray first)")
        if not (a.strides[2] == 1 and a.strides[1] == C and (h == 1 or a.strides[0] >= w * C)):
            a = np.ascontiguousarray(a)
        rs = a.strides[0] if h > 1 else w * C
        extent = (h - 1) * rs + w * C
        span = np.lib.stride_tricks.as_strided(a, shape=(extent,), strides=(1,))
        off = -(-off // align) * align
        desc[i] = (off, h, w, rs)
        spans.append((off, span))
        off += extent
    buf = np.zeros(max(off, 1), np.uint8)
    for o, span in spans:
        buf[o:o + span.shape[0]] = span
    return buf, desc


def _plane_span(a, i, what):
    """a plane uint8 [rows, W] whose bytes lie along its rows -> (the bytes from its first to its last as one view, its row pitch); any
    other layout is made contiguous first"""
    rows, w = a.shape
    if any(s < 0 for s in a.strides):
        raise ValueError(f"image {i}: negative strides {a.strides} of the {what} plane (flip with np.ascontiguousarray first)")
    if not (a.strides[1] == 1 and (rows == 1 or a.strides[0] >= w)):
        a = np.ascontiguousarray(a)
    pitch = a.strides[0] if rows > 1 else w
    return np.lib.stride_tricks.as_strided(a, shape=((rows - 1) * pitch + w,), strides=(1,)), pitch


def pack_yuv_images(images, fmt, align=16):
    """NV12 / NV21 surfaces -> (pixels uint8[bytes], descriptors YUV_IMAGE_DTYPE[n]).  An image is cv2's layout, one uint8 [H * 3 / 2, W]
    array (H rows of Y, then H / 2 rows of chroma byte pairs), or a pair (y [H, W], uv [H / 2, W]) of arrays or views, which may carry
    their own row pitches: a plane whose bytes lie along its rows keeps its pitch, as `pack_images` keeps a crop's.  Every plane starts on
    an `align`-byte boundary, a surface's Y plane before its UV plane.  Odd sides (cv2 refuses them too), sides outside 2..16384, other
    dtypes or shapes and negative strides are refused."""
    code = format_code(fmt)
    if code not in YUV_FORMATS:
        raise ValueError(f"pack_yuv_images: format {fmt!r}: 'nv12' or 'nv21'")
    spans, desc, off = [], np.zeros(len(images), YUV_IMAGE_DTYPE), 0
    for i, img in enumerate(images):
        if isinstance(img, (tuple, list)):
            if len(img) != 2:
                raise ValueError(f"image {i}: a pair (y, uv) or one [H * 3 / 2, W] array, got {len(img)} planes")
            y, uv = np.asarray(img[0]), np.asarray(img[1])
        else:
            a = np.asarray(img)
            if a.dtype != np.uint8 or a.ndim != 2:
                raise ValueError(f"image {i}: expected uint8 [H * 3 / 2, W] or a pair (y, uv), got {a.dtype} {a.shape}")
            if a.shape[0] % 3 != 0:
                raise ValueError(f"image {i}: {a.shape[0]} rows are not H * 3 / 2 of an even H (odd sides are refused)")
            h = a.shape[0] // 3 * 2
            y, uv = a[:h], a[h:]
        if y.dtype != np.uint8 or uv.dtype != np.uint8 or y.ndim != 2 or uv.ndim != 2:
            raise ValueError(f"image {i}: expected uint8 planes y [H, W] and uv [H / 2, W], got {y.dtype} {y.shape} and {uv.dtype} {uv.shape}")
        h, w = y.shape
        if h % 2 or w % 2:
            raise ValueError(f"image {i}: {h}x{w} has an odd side (NV12 / NV21 surfaces have even sides)")
        if not (2 <= h <= MAX_SIDE and 2 <= w <= MAX_SIDE):
            raise ValueError(f"image {i}: {h}x{w} is outside 2..{MAX_SIDE} per side")
        if uv.shape != (h // 2, w):
            raise ValueError(f"image {i}: the uv plane is {uv.shape}, a {h}x{w} surface has {(h // 2, w)}")
        y_span, sy = _plane_span(y, i, "y")
        uv_span, suv = _plane_span(uv, i, "uv")
        off = -(-off // align) * align
        off_y = off
        off = -(-(off + y_span.shape[0]) // align) * align
        desc[i] = (off_y, off, h, w, sy, suv)
        spans += [(off_y, y_span), (off, uv_span)]
        off += uv_span.shape[0]
    buf = np.zeros(max(off, 1), np.uint8)
    for o, span in spans:
        buf[o:o + span.shape[0]] = span
    return buf, desc


def yuv_sizes(desc):
    """YUV_IMAGE_DTYPE[n] -> IMAGE_DTYPE[n] for the ragged decodes, which read only height and width: boxes in the Y plane's pixels"""
    out = np.zeros(desc.shape[0], IMAGE_DTYPE)
    out["height"], out["width"], out["row_stride"] = desc["height"], desc["width"], desc["width"]
    return out


def _call(name, n, *args):
    """yf_images_<name>(*args), which returns n or fails with a text"""
    lib = load()
    rc = getattr(lib, "yf_images_" + name)(*args)
    if rc != n:
        raise ImagesError(f"yf_images_{name}: {(lib.yf_images_last_error_text() or b'').decode()} (returned {rc}, expected {n})")


def set_decode_tables(sig, ex, ident):
    """The tables the decodes that take no network use from now on (yf_images_set_decode_tables): what `network.decode_tables()` returned."""
    lib = load()
    sig, ex = np.ascontiguousarray(sig, np.float32), np.ascontiguousarray(ex, np.float32)
    if sig.size != 256 or ex.size != 256 or lib.yf_images_set_decode_tables(sig.ctypes.data, ex.ctypes.data, int(ident)) != 0:
        raise ImagesError(f"yf_images_set_decode_tables: {(lib.yf_images_last_error_text() or b'').decode() or 'two tables of 256 float32'}")


def prepare_device(d_pixels, pixels_bytes, fmt, height, width, row_stride, frame_stride, n, out_hw, d_frames, stream=None):
    _call("prepare_device", n, d_pixels, pixels_bytes, format_code(fmt), height, width, row_stride, frame_stride, n, out_hw, d_frames, stream)


def prepare_ragged_device(d_pixels, pixels_bytes, fmt, d_images, n, out_hw, d_frames, d_status, stream=None):
    _call("prepare_ragged_device", n, d_pixels, pixels_bytes, format_code(fmt), d_images, n, out_hw, d_frames, d_status, stream)


def _yuv_code(fmt):
    code = format_code(fmt)
    if code not in YUV_FORMATS:
        raise ValueError(f"format {fmt!r}: 'nv12' or 'nv21'")
    return code


def prepare_yuv_device(d_pixels, pixels_bytes, fmt, height, width, stride_y, uv_offset, stride_uv, frame_stride, n, out_hw, d_frames, stream=None):
    """n NV12 / NV21 surfaces of height x width -> int8 frames (yf_images_prepare_yuv_device): surface i's Y plane at i * frame_stride, its
    UV plane uv_offset bytes after that."""
    _call("prepare_yuv_device", n, d_pixels, pixels_bytes, _yuv_code(fmt), height, width, stride_y, uv_offset, stride_uv, frame_stride, n, out_hw,
          d_frames, stream)


def prepare_yuv_ragged_device(d_pixels, pixels_bytes, fmt, d_images, n, out_hw, d_frames, d_status, stream=None):
    """d_images: YUV_IMAGE_DTYPE[n] on the device (yf_images_prepare_yuv_ragged_device)"""
    _call("prepare_yuv_ragged_device", n, d_pixels, pixels_bytes, _yuv_code(fmt), d_images, n, out_hw, d_frames, d_status, stream)


def prepare_yuv_f16_device(d_pixels, pixels_bytes, fmt, height, width, stride_y, uv_offset, stride_uv, frame_stride, n, d_frames_f16, stream=None):
    _call("prepare_yuv_f16_device", n, d_pixels, pixels_bytes, _yuv_code(fmt), height, width, stride_y, uv_offset, stride_uv, frame_stride, n,
          d_frames_f16, stream)


def prepare_yuv_f16_ragged_device(d_pixels, pixels_bytes, fmt, d_images, n, d_frames_f16, d_status, stream=None):
    _call("prepare_yuv_f16_ragged_device", n, d_pixels, pixels_bytes, _yuv_code(fmt), d_images, n, d_frames_f16, d_status, stream)


def _run_yuv_ragged(network, d_px, nbytes, fmt, d_yuv_desc, d_desc, n, d_frames, d_heads, d_dets, d_counts, cap, d_status, size, f16, s):
    """What the run_decode_*_ragged_device entries do for packed pixels, for NV12 / NV21 surfaces, on stream `s`: the YUV prepare, the
    network's device run, the ragged decode of that size and dtype with the descriptors of the pictures' sizes (d_desc, IMAGE_DTYPE)."""
    if f16:
        prepare_yuv_f16_ragged_device(d_px, nbytes, fmt, d_yuv_desc, n, d_frames, d_status, stream=s)
        network.fp16_run_device(d_frames, d_heads, n, stream=s)
        decode_f32_ragged_device(d_heads, d_desc, n, d_dets, d_counts, cap, d_status=d_status, stream=s)
        return
    prepare_yuv_ragged_device(d_px, nbytes, fmt, d_yuv_desc, n, size, d_frames, d_status, stream=s)
    if size == 56:
        network.run_device(d_frames, d_heads, n, stream=s)
        decode_ragged_device(d_heads, d_desc, n, d_dets, d_counts, cap, stream=s)
    else:
        network.run_device_hw(size, size, d_frames, d_heads, n, stream=s)
        decode160_ragged_device(d_heads, d_desc, n, d_dets, d_counts, cap, d_status=d_status, stream=s)


def run_decode_device(network, d_pixels, pixels_bytes, fmt, height, width, row_stride, frame_stride, n, d_frames, d_heads, d_dets, d_counts,
                      cap, mode=binding.YF_DECODE_PY, stream=None):
    _call("run_decode_device", n, network.handle, d_pixels, pixels_bytes, format_code(fmt), height, width, row_stride, frame_stride, n, d_frames,
          d_heads, mode, d_dets, d_counts, cap, stream)


def run_decode_ragged_device(network, d_pixels, pixels_bytes, fmt, d_images, n, d_frames, d_heads, d_dets, d_counts, cap, d_status,
                             mode=binding.YF_DECODE_PY, stream=None):
    _call("run_decode_ragged_device", n, network.handle, d_pixels, pixels_bytes, format_code(fmt), d_images, n, d_frames, d_heads, mode, d_dets,
          d_counts, cap, d_status, stream)


def decode_ragged_device(d_heads, d_images, n, d_dets, d_counts, cap, mode=binding.YF_DECODE_PY, stream=None):
    _call("decode_ragged_device", n, d_heads, d_images, n, mode, d_dets, d_counts, cap, stream)


def _nms(name, d_dets, d_counts, n, cap, iou_threshold, d_out, d_out_counts, stream):
    d_out = d_dets if d_out is None else d_out
    d_out_counts = d_counts if d_out_counts is None else d_out_counts
    _call(name, n, d_dets, d_counts, n, cap, float(iou_threshold), d_out, d_out_counts, stream)


def nms_device(d_dets, d_counts, n, cap, iou_threshold, d_out=None, d_out_counts=None, stream=None):
    """Greedy IoU suppression of decoded records (yf_images_nms_device): d_dets yf_det[n][cap], d_counts int32[n] -> d_out, d_out_counts
    (in place when not given).  Order: descending conf, ties later record first; float64 arithmetic as yoloface_test.py:165-190 states it."""
    _nms("nms_device", d_dets, d_counts, n, cap, iou_threshold, d_out, d_out_counts, stream)


def decode160_device(d_heads, n, d_dets, d_counts, cap, w_scale=1.0, h_scale=1.0, stream=None):
    """Decode of 20x20 heads (yf_images_decode160_device): d_heads int8[n][20][20][18] -> d_dets yf_det[n][cap], d_counts int32[n]."""
    _call("decode160_device", n, d_heads, n, w_scale, h_scale, d_dets, d_counts, cap, stream)


def decode160_ragged_device(d_heads, d_images, n, d_dets, d_counts, cap, d_status=None, stream=None):
    _call("decode160_ragged_device", n, d_heads, d_images, d_status, n, d_dets, d_counts, cap, stream)


def run_decode160_device(network, d_pixels, pixels_bytes, fmt, height, width, row_stride, frame_stride, n, d_frames, d_heads, d_dets, d_counts,
                         cap, stream=None):
    _call("run_decode160_device", n, network.handle, d_pixels, pixels_bytes, format_code(fmt), height, width, row_stride, frame_stride, n,
          d_frames, d_heads, d_dets, d_counts, cap, stream)


def run_decode160_ragged_device(network, d_pixels, pixels_bytes, fmt, d_images, n, d_frames, d_heads, d_dets, d_counts, cap, d_status,
                                stream=None):
    _call("run_decode160_ragged_device", n, network.handle, d_pixels, pixels_bytes, format_code(fmt), d_images, n, d_frames, d_heads, d_dets,
          d_counts, cap, d_status, stream)


def nms_wide_device(d_dets, d_counts, n, cap, iou_threshold, d_out=None, d_out_counts=None, stream=None):
    """nms_device for up to NMS_WIDE_MAX_CAP records per frame (yf_images_nms_wide_device): the same semantics, in place when d_out is not
    given."""
    _nms("nms_wide_device", d_dets, d_counts, n, cap, iou_threshold, d_out, d_out_counts, stream)


def prepare_f16_device(d_pixels, pixels_bytes, fmt, height, width, row_stride, frame_stride, n, d_frames_f16, stream=None):
    """Images -> the fp16 network's frames (yf_images_prepare_f16_device): d_frames_f16 fp16 [n][56][56][3], pixel / 255. in RGB order."""
    _call("prepare_f16_device", n, d_pixels, pixels_bytes, format_code(fmt), height, width, row_stride, frame_stride, n, d_frames_f16, stream)


def prepare_f16_ragged_device(d_pixels, pixels_bytes, fmt, d_images, n, d_frames_f16, d_status, stream=None):
    _call("prepare_f16_ragged_device", n, d_pixels, pixels_bytes, format_code(fmt), d_images, n, d_frames_f16, d_status, stream)


def decode_f32_device(d_logits, n, d_dets, d_counts, cap, w_scale=1.0, h_scale=1.0, stream=None):
    """Decode of the fp16 network's logits (yf_images_decode_f32_device): d_logits float32 [n][7][7][18] -> d_dets yf_det[n][cap],
    d_counts int32[n]; h5_predition.py:51-72 in float32 (csrc/yf_images_float.h)."""
    _call("decode_f32_device", n, d_logits, n, w_scale, h_scale, d_dets, d_counts, cap, stream)


def decode_f32_ragged_device(d_logits, d_images, n, d_dets, d_counts, cap, d_status=None, stream=None):
    _call("decode_f32_ragged_device", n, d_logits, d_images, d_status, n, d_dets, d_counts, cap, stream)


def run_decode_f16_device(network, d_pixels, pixels_bytes, fmt, height, width, row_stride, frame_stride, n, d_frames_f16, d_logits, d_dets,
                          d_counts, cap, stream=None):
    _call("run_decode_f16_device", n, network.handle, d_pixels, pixels_bytes, format_code(fmt), height, width, row_stride, frame_stride, n,
          d_frames_f16, d_logits, d_dets, d_counts, cap, stream)


def run_decode_f16_ragged_device(network, d_pixels, pixels_bytes, fmt, d_images, n, d_frames_f16, d_logits, d_dets, d_counts, cap, d_status,
                                 stream=None):
    _call("run_decode_f16_ragged_device", n, network.handle, d_pixels, pixels_bytes, format_code(fmt), d_images, n, d_frames_f16, d_logits,
          d_dets, d_counts, cap, d_status, stream)


def fit_of(h, w, size):
    """Where a picture of h x w lies in a letterboxed frame of side `size` (yf_images_fit; host only): -> (x0, y0, width, height).  The
    definition: csrc/yf_images_fit.h, ptq.letterbox_fit."""
    lib, out = load(), np.zeros(1, FIT_DTYPE)
    if lib.yf_images_fit(int(h), int(w), int(size), out.ctypes.data) != 0:
        raise ImagesError(f"yf_images_fit: {(lib.yf_images_last_error_text() or b'').decode()}")
    return tuple(int(out[0][k]) for k in ("x0", "y0", "width", "height"))


def prepare_fit_ragged_device(d_pixels, pixels_bytes, fmt, d_images, n, out_hw, d_frames, d_status, pad=114, stream=None):
    """Packed pictures -> letterboxed int8 frames (yf_images_prepare_fit_ragged_device): each picture resized with its aspect kept into
    the rectangle of `fit_of`, the rest of its frame (int8)(pad - 128).  ptq.letterbox_u8."""
    _call("prepare_fit_ragged_device", n, d_pixels, pixels_bytes, _packed_code(fmt, "prepare_fit_ragged_device"), d_images, n, out_hw, pad,
          d_frames, d_status, stream)


def prepare_fit_yuv_ragged_device(d_pixels, pixels_bytes, fmt, d_images, n, out_hw, d_frames, d_status, pad=114, stream=None):
    """... for NV12 / NV21 surfaces (yf_images_prepare_fit_yuv_ragged_device): d_images YUV_IMAGE_DTYPE[n]"""
    _call("prepare_fit_yuv_ragged_device", n, d_pixels, pixels_bytes, _yuv_code(fmt), d_images, n, out_hw, pad, d_frames, d_status, stream)


def prepare_fit_f16_ragged_device(d_pixels, pixels_bytes, fmt, d_images, n, d_frames_f16, d_status, pad=114, stream=None):
    """... to the fp16 network's frames, fp16 [n][56][56][3] of byte / 255. (yf_images_prepare_fit_f16_ragged_device)"""
    _call("prepare_fit_f16_ragged_device", n, d_pixels, pixels_bytes, _packed_code(fmt, "prepare_fit_f16_ragged_device"), d_images, n, pad,
          d_frames_f16, d_status, stream)


def prepare_fit_yuv_f16_ragged_device(d_pixels, pixels_bytes, fmt, d_images, n, d_frames_f16, d_status, pad=114, stream=None):
    _call("prepare_fit_yuv_f16_ragged_device", n, d_pixels, pixels_bytes, _yuv_code(fmt), d_images, n, pad, d_frames_f16, d_status, stream)


def decode_fit_ragged_device(d_heads, d_images, n, out_hw, d_dets, d_counts, cap, d_status=None, stream=None):
    """The decode of the heads of letterboxed frames (yf_images_decode_fit_ragged_device): d_heads int8 [n][7][7][18] (out_hw 56) or
    [n][20][20][18] (160), d_images IMAGE_DTYPE[n] (only the sides are read) -> boxes in each picture's own pixels, mapped back through
    its fit."""
    _call("decode_fit_ragged_device", n, d_heads, d_images, d_status, n, out_hw, d_dets, d_counts, cap, stream)


def decode_f32_fit_ragged_device(d_logits, d_images, n, d_dets, d_counts, cap, d_status=None, stream=None):
    _call("decode_f32_fit_ragged_device", n, d_logits, d_images, d_status, n, d_dets, d_counts, cap, stream)


def run_decode_fit_ragged_device(network, d_pixels, pixels_bytes, fmt, d_images, n, out_hw, d_frames, d_heads, d_dets, d_counts, cap, d_status,
                                 pad=114, stream=None):
    """Packed pictures -> letterboxed frames -> the network -> records in the pictures' pixels (yf_images_run_decode_fit_ragged_device)"""
    _call("run_decode_fit_ragged_device", n, network.handle, d_pixels, pixels_bytes, _packed_code(fmt, "run_decode_fit_ragged_device"), d_images,
          n, out_hw, pad, d_frames, d_heads, d_dets, d_counts, cap, d_status, stream)


def run_decode_fit_f16_ragged_device(network, d_pixels, pixels_bytes, fmt, d_images, n, d_frames_f16, d_logits, d_dets, d_counts, cap, d_status,
                                     pad=114, stream=None):
    _call("run_decode_fit_f16_ragged_device", n, network.handle, d_pixels, pixels_bytes, _packed_code(fmt, "run_decode_fit_f16_ragged_device"),
          d_images, n, pad, d_frames_f16, d_logits, d_dets, d_counts, cap, d_status, stream)


def _run_fit_yuv_ragged(network, d_px, nbytes, fmt, d_yuv_desc, d_desc, n, d_frames, d_heads, d_dets, d_counts, cap, d_status, size, f16, pad, s):
    """`_run_yuv_ragged` with letterboxed frames: the YUV fit prepare, the network's device run, the fit decode of that size and dtype"""
    if f16:
        prepare_fit_yuv_f16_ragged_device(d_px, nbytes, fmt, d_yuv_desc, n, d_frames, d_status, pad=pad, stream=s)
        network.fp16_run_device(d_frames, d_heads, n, stream=s)
        decode_f32_fit_ragged_device(d_heads, d_desc, n, d_dets, d_counts, cap, d_status=d_status, stream=s)
        return
    prepare_fit_yuv_ragged_device(d_px, nbytes, fmt, d_yuv_desc, n, size, d_frames, d_status, pad=pad, stream=s)
    if size == 56:
        network.run_device(d_frames, d_heads, n, stream=s)
    else:
        network.run_device_hw(size, size, d_frames, d_heads, n, stream=s)
    decode_fit_ragged_device(d_heads, d_desc, n, size, d_dets, d_counts, cap, d_status=d_status, stream=s)


def _fit_code(fit):
    if fit not in FITS:
        raise ValueError(FIT_WHAT.format(fit))
    return FITS.index(fit)


def area_bands(n, out_hw):
    """How many bands of output rows the area prepare splits each frame of a batch of n into (yf_images_area_bands; host only): one job
    per (frame, band), from n and out_hw alone.  The frames do not depend on it."""
    bands = int(load().yf_images_area_bands(int(n), int(out_hw)))
    if bands < 1:
        raise ImagesError(f"yf_images_area_bands({n}, {out_hw}): n >= 0 and out_hw 56 or 160")
    return bands


def prepare_area_ragged_device(d_pixels, pixels_bytes, fmt, d_images, n, out_hw, d_frames, d_status, fit="stretch", pad=114, stream=None):
    """Packed pictures -> area-averaged int8 frames (yf_images_prepare_area_ragged_device): every source pixel counted with the share of it
    an output pixel covers, rounded half up -- `ptq.resize_area_u8`; fit="letterbox": resized so to the rectangle of `fit_of`, the rest of
    the frame (int8)(pad - 128) -- `ptq.letterbox_u8(..., interp="area")`.  The definition: csrc/yf_images_area.h."""
    _call("prepare_area_ragged_device", n, d_pixels, pixels_bytes, _packed_code(fmt, "prepare_area_ragged_device"), d_images, n, out_hw,
          _fit_code(fit), pad, d_frames, d_status, stream)


def prepare_area_yuv_ragged_device(d_pixels, pixels_bytes, fmt, d_images, n, out_hw, d_frames, d_status, fit="stretch", pad=114, stream=None):
    """... for NV12 / NV21 surfaces (yf_images_prepare_area_yuv_ragged_device): d_images YUV_IMAGE_DTYPE[n]; every pixel converted, then averaged"""
    _call("prepare_area_yuv_ragged_device", n, d_pixels, pixels_bytes, _yuv_code(fmt), d_images, n, out_hw, _fit_code(fit), pad, d_frames,
          d_status, stream)


def prepare_area_f16_ragged_device(d_pixels, pixels_bytes, fmt, d_images, n, d_frames_f16, d_status, fit="stretch", pad=114, stream=None):
    """... to the fp16 network's frames, fp16 [n][56][56][3] of byte / 255. (yf_images_prepare_area_f16_ragged_device)"""
    _call("prepare_area_f16_ragged_device", n, d_pixels, pixels_bytes, _packed_code(fmt, "prepare_area_f16_ragged_device"), d_images, n,
          _fit_code(fit), pad, d_frames_f16, d_status, stream)


def prepare_area_yuv_f16_ragged_device(d_pixels, pixels_bytes, fmt, d_images, n, d_frames_f16, d_status, fit="stretch", pad=114, stream=None):
    _call("prepare_area_yuv_f16_ragged_device", n, d_pixels, pixels_bytes, _yuv_code(fmt), d_images, n, _fit_code(fit), pad, d_frames_f16,
          d_status, stream)


def _run_area_ragged(network, d_px, nbytes, fmt, d_pictures, d_desc, n, d_frames, d_heads, d_dets, d_counts, cap, d_status, size, f16, fit, pad, s):
    """interp="area" of `_stage`, composed on stream `s` as `_run_yuv_ragged` and `_run_fit_yuv_ragged` compose theirs: the area prepare of
    the family and dtype (d_pictures: the descriptors it takes), the network's device run, and the decode that exists for the fit -- the
    plain ragged one for "stretch", the fit one for "letterbox" -- with the descriptors of the frames' sizes (d_desc, IMAGE_DTYPE)."""
    letterbox = fit == "letterbox"
    if f16:
        prepare = prepare_area_yuv_f16_ragged_device if is_yuv(fmt) else prepare_area_f16_ragged_device
        prepare(d_px, nbytes, fmt, d_pictures, n, d_frames, d_status, fit=fit, pad=pad, stream=s)
        network.fp16_run_device(d_frames, d_heads, n, stream=s)
        decode = decode_f32_fit_ragged_device if letterbox else decode_f32_ragged_device
        decode(d_heads, d_desc, n, d_dets, d_counts, cap, d_status=d_status, stream=s)
        return
    prepare = prepare_area_yuv_ragged_device if is_yuv(fmt) else prepare_area_ragged_device
    prepare(d_px, nbytes, fmt, d_pictures, n, size, d_frames, d_status, fit=fit, pad=pad, stream=s)
    if size == 56:
        network.run_device(d_frames, d_heads, n, stream=s)
    else:
        network.run_device_hw(size, size, d_frames, d_heads, n, stream=s)
    if letterbox:
        decode_fit_ragged_device(d_heads, d_desc, n, size, d_dets, d_counts, cap, d_status=d_status, stream=s)
    elif size == 56:
        decode_ragged_device(d_heads, d_desc, n, d_dets, d_counts, cap, stream=s)
    else:
        decode160_ragged_device(d_heads, d_desc, n, d_dets, d_counts, cap, d_status=d_status, stream=s)


def match_device(d_dets, d_counts, n, cap, d_gt, d_gt_counts, gt_cap, iou_threshold, d_tp, d_best=None, stream=None):
    """Records against their frame's ground truths (yf_images_match_device): d_dets yf_det[n][cap], d_counts int32[n], d_gt GT_DTYPE[n][gt_cap],
    d_gt_counts int32[n] -> d_tp uint8[n][cap] (1 true positive, 0 false positive) and, if given, d_best int32[n][cap] (the best ground
    truth's index or -1).  Order of the claim: descending conf, ties earlier record first; float64 as yolov3_train_tf.py:657-746 states it."""
    _call("match_device", n, d_dets, d_counts, n, cap, d_gt, d_gt_counts, gt_cap, float(iou_threshold), d_tp, d_best, stream)


def average_precision_workspace(n, cap):
    """Bytes of scratch average_precision_device needs for n frames of cap records (0 for arguments it would refuse)."""
    return int(load().yf_images_average_precision_workspace(n, cap))


def average_precision_device(d_dets, d_counts, d_tp, n, cap, d_gt_counts, gt_cap, d_work, work_bytes, d_result, d_curve=None, stream=None):
    """Average precision of the batch from match_device's flags (yf_images_average_precision_device): d_result one EVAL_RESULT_DTYPE,
    d_curve (optional) float64 [n * cap][2] = (recall, envelope precision) of the first `detections` records in order; d_work at least
    average_precision_workspace(n, cap) bytes, 16-byte aligned."""
    _call("average_precision_device", n, d_dets, d_counts, d_tp, n, cap, d_gt_counts, gt_cap, d_work, work_bytes, d_result, d_curve, stream)


def _pair(v, what):
    """an int or (y, x) -> (y, x)"""
    y, x = (v, v) if np.ndim(v) == 0 else v
    if int(y) != y or int(x) != x:
        raise ValueError(f"{what} {v!r}: an integer or (y, x) integers")
    return int(y), int(x)


def plan_tiles(shapes_or_descriptors, fmt, tile, stride=None, whole=True):
    """The tile grid of a batch (yf_images_plan_tiles; host only): -> (tiles TILE_DTYPE[t], tile_desc IMAGE_DTYPE[t], first int32[n + 1]).
    `shapes_or_descriptors`: an IMAGE_DTYPE array (as `pack_images` returns: the tile descriptors then point into the same pixel buffer,
    parent row stride and all) or a list of (height, width), taken as packed images one after the other.  `tile`, `stride`: an int or
    (y, x); stride=None means the tile side, so no overlap.  Per axis of length L: one tile [0, L) if L <= T, else
    (L - T + S - 1) // S + 1 tiles of side T, the last one flush with the edge; row-major, y outer.  `whole`: an image of more than one
    tile gets the whole image as its first tile.  Image i's tiles are first[i] .. first[i + 1]."""
    code = _packed_code(fmt, "plan_tiles")
    C = CHANNELS[code]
    if isinstance(shapes_or_descriptors, np.ndarray) and shapes_or_descriptors.dtype == IMAGE_DTYPE:
        desc = np.ascontiguousarray(shapes_or_descriptors).reshape(-1)
    else:
        desc, off = np.zeros(len(shapes_or_descriptors), IMAGE_DTYPE), 0
        for i, (h, w) in enumerate(shapes_or_descriptors):
            desc[i] = (off, h, w, int(w) * C)
            off += int(h) * int(w) * C
    th, tw = _pair(tile, "tile")
    sy, sx = (th, tw) if stride is None else _pair(stride, "stride")
    lib, n = load(), desc.shape[0]
    args = (desc.ctypes.data, n, code, th, tw, sy, sx, int(bool(whole)))
    t = lib.yf_images_plan_tiles(*args, None, None, None, 0)
    if t < 0:
        raise ImagesError(f"yf_images_plan_tiles: {(lib.yf_images_last_error_text() or b'').decode()}")
    tiles, tile_desc, first = np.zeros(t, TILE_DTYPE), np.zeros(t, IMAGE_DTYPE), np.zeros(n + 1, np.int32)
    if lib.yf_images_plan_tiles(*args, tiles.ctypes.data, tile_desc.ctypes.data, first.ctypes.data, t) != t:
        raise ImagesError(f"yf_images_plan_tiles: {(lib.yf_images_last_error_text() or b'').decode()}")
    return tiles, tile_desc, first


def pack_tiles(images, fmt="bgr", tile=160, stride=None, whole=True):
    """`pack_images`, then `plan_tiles` on its descriptors: -> (pixels uint8[bytes], tile_desc IMAGE_DTYPE[t], tiles TILE_DTYPE[t],
    first int32[n + 1]).  The pixels are stored once; overlapping tiles share them."""
    buf, desc = pack_images(images, fmt)
    tiles, tile_desc, first = plan_tiles(desc, fmt, tile, stride, whole)
    return buf, tile_desc, tiles, first


def gather_tiles_workspace(t):
    """Bytes of scratch gather_tiles_device needs for t tiles."""
    return int(load().yf_images_gather_tiles_workspace(t))


def gather_tiles_device(d_dets, d_counts, t, cap, d_tiles, d_first, n, d_out, d_out_counts, out_cap, d_work, work_bytes, stream=None):
    """The records of t tiles merged per image (yf_images_gather_tiles_device): d_dets yf_det[t][cap], d_counts int32[t], d_tiles
    TILE_DTYPE[t], d_first int32[n + 1] -> d_out yf_det[n][out_cap]: image i's tiles in order, their records in theirs, frame = i, the
    edges moved by the tile's origin; d_out_counts int32[n] the true totals (only the first out_cap records are written)."""
    _call("gather_tiles_device", n, d_dets, d_counts, t, cap, d_tiles, d_first, n, d_out, d_out_counts, out_cap, d_work, work_bytes, stream)


def pack_ground_truths(ground_truths):
    """one [k, 4] array (x1, y1, x2, y2) per image -> (GT_DTYPE [n, gt_cap], int32 [n]), gt_cap the largest k (at least 1)"""
    gts = [np.asarray(g, np.float64).reshape(-1, 4) for g in ground_truths]
    gt_cap = max([1] + [g.shape[0] for g in gts])
    if gt_cap > EVAL_MAX_GT:
        raise ValueError(f"{gt_cap} ground-truth boxes in one image: at most {EVAL_MAX_GT}")
    packed = np.zeros((len(gts), gt_cap), GT_DTYPE)
    for i, g in enumerate(gts):
        packed[i, :g.shape[0]] = np.ascontiguousarray(g).view(GT_DTYPE).reshape(-1)
    return packed, np.array([g.shape[0] for g in gts], np.int32)


def _check_frames(size, dtype):
    if size not in (56, 160):
        raise ValueError(f"size {size!r}: 56 or 160")
    if dtype not in ("int8", "fp16"):
        raise ValueError(f"dtype {dtype!r}: 'int8' or 'fp16'")
    if dtype == "fp16" and size != 56:
        raise ValueError("dtype 'fp16': the fp16 network has 56x56 frames only")


@dataclasses.dataclass
class _Batch:
    """A batch as `_stage` left it on the device.  The tensors live as long as the object: hold it until the stream is synchronised."""
    n: int                  # pictures
    cap: int                # records a picture can hold: d_dets uint8 [n, cap, 28]
    device: object
    stream: object          # the device's current stream at staging: everything was launched on it, nothing waited for
    d_dets: object          # the records a caller works on: after the suppression if there was one; with tiles, those of a picture's tiles merged
    d_counts: object        # int32 [n], how many of them each picture has
    d_status: object       # int32 per frame of the network (a picture, or with tiles a tile): 1 the library refused its descriptor
    d_totals: object        # with tiles int32 [n], the merged records per picture before the suppression and the cut at cap; else None
    d_px: object            # the pictures' bytes, as pack_images / pack_yuv_images laid them out
    nbytes: int
    d_pictures: object      # the pictures' descriptors as the crop and redact entries take them: YUV_IMAGE_DTYPE [n] for NV12 / NV21
                            # surfaces, IMAGE_DTYPE [n] for packed pictures (with tiles: of the parent pictures, not of the tiles)
    held: tuple             # everything else the launches read or write

    def boxes(self, counts):
        """the first counts[i] records of every picture i -> a list of int32 [k, 4] arrays (x1, y1, x2, y2); after a synchronise"""
        dets = self.d_dets.cpu().numpy().view(binding.DET_DTYPE).reshape(self.n, self.cap)
        out = []
        for i in range(self.n):
            d = dets[i, :int(counts[i])]
            out.append(np.stack([d["x1"], d["y1"], d["x2"], d["y2"]], axis=1).astype(np.int32).reshape(-1, 4))
        return out

    def check_totals(self, what):
        """with tiles: a picture whose merged records did not fit into cap raises; after a synchronise"""
        if self.d_totals is None:
            return
        totals = self.d_totals.cpu().numpy()
        over = np.nonzero(totals > self.cap)[0]
        if over.size:
            i = int(over[0])
            raise ImagesError(f"{what}: image {i} has {int(totals[i])} merged records, out_cap holds {self.cap}"
                              + (f" (and {over.size - 1} more image(s) above it)" if over.size > 1 else ""))


def _stage(network, images, fmt, cap, device, iou_threshold, size, dtype, tile=None, stride=None, whole=True, out_cap=None, fit="stretch",
           pad=114, interp="linear"):
    """What every `detect_*` call and `evaluate` launch first, with the records left on the device -- the place to hang a new stage
    behind: packs the pictures, allocates the workspaces and runs images -> frames -> network -> records (and the suppression when
    iou_threshold is not None) at `size` and `dtype` on the device's current stream, without synchronising.  cap=None holds every candidate
    (147 / 1200).  With `tile` (and `stride`, `whole`: `plan_tiles`) the frames are the pictures' tiles, every candidate of a tile is
    held, and the tiles' records are merged per picture (`gather_tiles_device`) into out_cap slots (None: 1200) and suppressed there
    (`nms_wide_device`); the pixels are packed once, the tiles share them.  fit="stretch" resizes every frame's picture (or tile) onto the
    whole frame, as the reference does; fit="letterbox" keeps its aspect, pads the rest of the frame with the grey `pad` and maps the boxes
    back through the same rectangle (`prepare_fit_*`, `run_decode_fit_*`, `decode_fit_*`; with tiles, every tile and the whole-picture
    tile is letterboxed, and a square tile is the same either way).  interp="linear" resizes as cv2.resize's INTER_LINEAR does, every
    launch as it was; interp="area" averages every source pixel of the picture (or tile) instead (`prepare_area_*`, then the network
    and the decode of the fit, `_run_area_ragged`; a tile is a descriptor into its parent's pixels, so tiles need nothing of their own)."""
    if fit not in FITS:
        raise ValueError(FIT_WHAT.format(fit))
    if interp not in INTERPS:
        raise ValueError(INTERP_WHAT.format(interp))
    if not 0 <= int(pad) <= 255:
        raise ValueError(f"pad {pad!r}: 0 to 255")
    letterbox, pad = fit == "letterbox", int(pad)
    if tile is not None:
        out_cap = NMS_WIDE_MAX_CAP if out_cap is None else out_cap
        if not 1 <= out_cap <= NMS_WIDE_MAX_CAP:
            raise ValueError(f"out_cap {out_cap!r}: 1 to {NMS_WIDE_MAX_CAP}")
    _check_frames(size, dtype)
    import torch
    yuv, n = is_yuv(fmt), len(images)
    buf, pictures = pack_yuv_images(images, fmt) if yuv else pack_images(images, fmt)
    desc = yuv_sizes(pictures) if yuv else pictures     # a frame's descriptor for the run and the decode: IMAGE_DTYPE
    if tile is not None:
        tiles, desc, first = plan_tiles(pictures, fmt, tile, stride, whole)
        cap = None
    grid, t = size // 8, desc.shape[0]
    if cap is None:
        cap = 3 * grid * grid
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else device)
    upload = lambda a: torch.from_numpy(a.view(np.uint8)).to(dev)
    d_px, d_desc = torch.from_numpy(buf).to(dev), upload(desc)
    d_pictures = d_desc if desc is pictures else upload(pictures)
    f16 = dtype == "fp16"
    d_frames = torch.empty((t, size, size, 3), dtype=torch.float16 if f16 else torch.int8, device=dev)
    d_heads = torch.empty((t, grid, grid, 18), dtype=torch.float32 if f16 else torch.int8, device=dev)
    d_dets = torch.empty((t, cap, binding.DET_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    d_counts = torch.empty(t, dtype=torch.int32, device=dev)
    d_status = torch.empty(t, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev)
    s = stream.cuda_stream
    run, nms = (run_decode_ragged_device, nms_device) if size == 56 else (run_decode160_ragged_device, nms_wide_device)
    if f16:
        run = run_decode_f16_ragged_device
    else:
        set_decode_tables(*network.decode_tables())     # a model file may bring its own; a later decode of these heads without the network finds them
    if interp == "area":
        _run_area_ragged(network, d_px.data_ptr(), buf.nbytes, fmt, (d_pictures if yuv else d_desc).data_ptr(), d_desc.data_ptr(), t,
                         d_frames.data_ptr(), d_heads.data_ptr(), d_dets.data_ptr(), d_counts.data_ptr(), cap, d_status.data_ptr(), size, f16,
                         fit, pad, s)
    elif yuv and letterbox:
        _run_fit_yuv_ragged(network, d_px.data_ptr(), buf.nbytes, fmt, d_pictures.data_ptr(), d_desc.data_ptr(), t, d_frames.data_ptr(),
                            d_heads.data_ptr(), d_dets.data_ptr(), d_counts.data_ptr(), cap, d_status.data_ptr(), size, f16, pad, s)
    elif yuv:
        _run_yuv_ragged(network, d_px.data_ptr(), buf.nbytes, fmt, d_pictures.data_ptr(), d_desc.data_ptr(), t, d_frames.data_ptr(),
                        d_heads.data_ptr(), d_dets.data_ptr(), d_counts.data_ptr(), cap, d_status.data_ptr(), size, f16, s)
    elif letterbox and f16:
        run_decode_fit_f16_ragged_device(network, d_px.data_ptr(), buf.nbytes, fmt, d_desc.data_ptr(), t, d_frames.data_ptr(),
                                         d_heads.data_ptr(), d_dets.data_ptr(), d_counts.data_ptr(), cap, d_status.data_ptr(), pad=pad, stream=s)
    elif letterbox:
        run_decode_fit_ragged_device(network, d_px.data_ptr(), buf.nbytes, fmt, d_desc.data_ptr(), t, size, d_frames.data_ptr(),
                                     d_heads.data_ptr(), d_dets.data_ptr(), d_counts.data_ptr(), cap, d_status.data_ptr(), pad=pad, stream=s)
    else:
        run(network, d_px.data_ptr(), buf.nbytes, fmt, d_desc.data_ptr(), t, d_frames.data_ptr(), d_heads.data_ptr(),
            d_dets.data_ptr(), d_counts.data_ptr(), cap, d_status.data_ptr(), stream=s)
    held = (d_desc, d_frames, d_heads)
    if tile is None:
        if iou_threshold is not None:
            nms(d_dets.data_ptr(), d_counts.data_ptr(), n, cap, iou_threshold, stream=s)
        return _Batch(n, cap, dev, stream, d_dets, d_counts, d_status, None, d_px, buf.nbytes, d_pictures, held)
    d_tiles, d_first = upload(tiles), torch.from_numpy(first).to(dev)
    d_out = torch.empty((n, out_cap, binding.DET_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    d_totals = torch.empty(n, dtype=torch.int32, device=dev)
    work_bytes = gather_tiles_workspace(t)
    d_work = torch.empty(max(work_bytes, 16), dtype=torch.uint8, device=dev)
    gather_tiles_device(d_dets.data_ptr(), d_counts.data_ptr(), t, cap, d_tiles.data_ptr(), d_first.data_ptr(), n, d_out.data_ptr(),
                        d_totals.data_ptr(), out_cap, d_work.data_ptr(), work_bytes, stream=s)
    d_kept = d_totals
    if iou_threshold is not None:                       # the records in place, the kept counts beside the totals
        d_kept = torch.empty(n, dtype=torch.int32, device=dev)
        nms_wide_device(d_out.data_ptr(), d_totals.data_ptr(), n, out_cap, iou_threshold, d_out.data_ptr(), d_kept.data_ptr(), stream=s)
    return _Batch(n, out_cap, dev, stream, d_out, d_kept, d_status, d_totals, d_px, buf.nbytes, d_pictures,
                  held + (d_dets, d_counts, d_tiles, d_first, d_work))


def evaluate(network, images, ground_truths, fmt="bgr", conf_iou=0.5, iou_threshold=None, size=56, dtype="int8", device=None,
             tile=None, stride=None, whole=True, fit="stretch", pad=114, interp="linear"):
    """Average precision of the network's boxes against labelled ones: what evaluate_model (yolov3_train_tf.py:809-869) reports, for the
    batch `detect` takes.  `ground_truths`: one [k, 4] array (x1, y1, x2, y2) per image, in that image's pixels.  The records are decoded as
    by `detect` (fmt, size, dtype as there; iou_threshold=None scores every record, a float suppresses first, as evaluate_model does),
    matched at IoU `conf_iou` (match_device) and scored (average_precision_device) on the same stream; only the 32-byte result and the
    per-image status come back.  tile=None scores the untiled records; with a tile (and `stride`, `whole`: `detect_tiled`) the records are
    those of the tiles merged per image (at most 1200 per image; more raises ImagesError).  An image (a tile) the library refused (status 1;
    `pack_images` produces none) raises ImagesError.  fit, pad: as in `detect` -- the tool to score both preprocessings on labelled pictures.
    Returns {"ap", "detections", "ground_truths", "true_positives", "precision", "recall"}; the last two are the end of the curve:
    true_positives / (detections + 1e-16) and true_positives / max(1, ground_truths)."""
    if tile is not None:
        _packed_code(fmt, "evaluate(tile=...)")
    n = len(images)
    if len(ground_truths) != n:
        raise ValueError(f"{n} images, {len(ground_truths)} lists of ground truths")
    gt, gt_counts = pack_ground_truths(ground_truths)
    if n == 0:
        return {"ap": 0.0, "detections": 0, "ground_truths": 0, "true_positives": 0, "precision": 0.0, "recall": 0.0}
    b = _stage(network, images, fmt, None, device, iou_threshold, size, dtype, tile, stride, whole, fit=fit, pad=pad, interp=interp)
    import torch
    dev, cap, gt_cap, s = b.device, b.cap, gt.shape[1], b.stream.cuda_stream
    d_gt = torch.from_numpy(gt.view(np.float64).reshape(n, gt_cap, 4)).to(dev)
    d_gt_counts = torch.from_numpy(gt_counts).to(dev)
    d_tp = torch.empty((n, cap), dtype=torch.uint8, device=dev)
    work_bytes = average_precision_workspace(n, cap)
    d_work = torch.empty(work_bytes, dtype=torch.uint8, device=dev)
    d_result = torch.empty(4, dtype=torch.float64, device=dev)
    match_device(b.d_dets.data_ptr(), b.d_counts.data_ptr(), n, cap, d_gt.data_ptr(), d_gt_counts.data_ptr(), gt_cap, conf_iou,
                 d_tp.data_ptr(), stream=s)
    average_precision_device(b.d_dets.data_ptr(), b.d_counts.data_ptr(), d_tp.data_ptr(), n, cap, d_gt_counts.data_ptr(), gt_cap,
                             d_work.data_ptr(), work_bytes, d_result.data_ptr(), stream=s)
    b.stream.synchronize()
    bad = np.nonzero(b.d_status.cpu().numpy())[0]
    if bad.size:
        raise ImagesError(f"evaluate: the library refused image(s) {bad.tolist()} (status 1): their frames hold no picture")
    b.check_totals("evaluate")
    res = d_result.cpu().numpy().view(EVAL_RESULT_DTYPE)[0]
    m, num_gt, tp = int(res["detections"]), int(res["ground_truths"]), int(res["true_positives"])
    return {"ap": float(res["ap"]), "detections": m, "ground_truths": num_gt, "true_positives": tp,
            "precision": tp / (m + 1e-16), "recall": tp / max(1, num_gt)}


def _code(table, value, what):
    """`value` as a code of `table` (name -> code): one of its names in any letter case, or one of its codes as a number (not a bool);
    anything else is refused with `what`, a text with one place for the value"""
    if isinstance(value, str):
        if value.lower() in table:
            return table[value.lower()]
    elif not isinstance(value, bool) and value in table.values():
        return int(value)
    raise ValueError(what.format(value))


def _permille(margin):
    """a share of a box's side, 0 to 1 -> permille, as the crop and redact entries take it"""
    permille = int(round(float(margin) * 1000))
    if not 0 <= permille <= 1000:
        raise ValueError(f"margin {margin!r}: 0 to 1")
    return permille


def crop_records_device(d_pixels, pixels_bytes, fmt, d_images, d_dets, d_counts, n, cap, out_h, out_w, d_chips, chips_cap, d_first, d_info,
                        order="rgb", margin_permille=0, square=False, stream=None):
    """Face chips of the records of a batch of packed pictures (yf_images_crop_records_device): d_images IMAGE_DTYPE[n], d_dets
    yf_det[n][cap], d_counts int32[n] -> d_chips uint8 [chips_cap, out_h, out_w, 3] in `order`, d_first int32[n + 1] (chip first[i] + s is
    slot s of frame i; first[n] the true total), d_info CHIP_DTYPE[chips_cap].  The region rule: csrc/yf_images_crop.h, ptq.crop_region."""
    _call("crop_records_device", n, d_pixels, pixels_bytes, _packed_code(fmt, "crop_records_device"), d_images, d_dets, d_counts, n, cap,
          out_h, out_w, _code(ORDERS, order, ORDER_WHAT), margin_permille, YF_CROP_SQUARE if square else 0, d_chips, chips_cap, d_first, d_info,
          stream)


def crop_records_yuv_device(d_pixels, pixels_bytes, fmt, d_images, d_dets, d_counts, n, cap, out_h, out_w, d_chips, chips_cap, d_first, d_info,
                            order="rgb", margin_permille=0, square=False, stream=None):
    """`crop_records_device` for NV12 / NV21 surfaces, read where they lie (yf_images_crop_records_yuv_device): d_images
    YUV_IMAGE_DTYPE[n]; a chip is the chip of the converted picture."""
    _call("crop_records_yuv_device", n, d_pixels, pixels_bytes, _yuv_code(fmt), d_images, d_dets, d_counts, n, cap, out_h, out_w,
          _code(ORDERS, order, ORDER_WHAT), margin_permille, YF_CROP_SQUARE if square else 0, d_chips, chips_cap, d_first, d_info, stream)


def detect_chips(network, images, out=(112, 112), margin=0.0, square=False, order="rgb", fmt="bgr", cap=None, iou_threshold=0.4, size=56,
                 dtype="int8", device=None, tile=None, stride=None, whole=True, chips_cap=None, fit="stretch", pad=114, interp="linear"):
    """`detect` (with `tile`: `detect_tiled`, whose `tile`, `stride`, `whole` these are), and every kept box cut out of its picture and
    resized to `out` = (out_h, out_w) (an int: square chips; multiples of 16 in 16..256) on the GPU, on the same stream, from the pixels
    that are already there: what a recogniser, a landmark model or a blur filter takes next.  `margin`: the box grows by this share of
    its width and height on every side (0..1, rounded to permille); `square`: the grown box is made square about its centre before it is
    clamped to the picture (it is not squared again afterwards: csrc/yf_images_crop.h, `ptq.crop_region`); `order`: the chips' byte
    order, "rgb" or "bgr".  fmt, cap, iou_threshold, size, dtype, device as in `detect` (NV12 / NV21 surfaces are cut where they lie;
    with `tile`, cap is `detect_tiled`'s out_cap and the chips are cut from the parent pictures; fit, pad as in `detect`).
    The chips are sized from a read-back of the counts; with chips_cap= nothing is read back before the crop, and a batch with more
    boxes raises ImagesError.
    Returns (boxes, chips, info): per image the int32 [k, 4] array `detect` returns, a uint8 [k, out_h, out_w, 3] array of its chips in
    the same order, and the CHIP_DTYPE [k] rows (the region actually sampled; status 1: the box has no pixel in the picture, the chip is
    zeros)."""
    out_h, out_w = _pair(out, "out")
    permille = _permille(margin)
    order_code = _code(ORDERS, order, ORDER_WHAT)
    n = len(images)
    if n == 0:
        return [], [], []
    import torch
    if tile is not None:
        _packed_code(fmt, "detect_chips(tile=...)")
    b = _stage(network, images, fmt, cap, device, iou_threshold, size, dtype, tile, stride, whole, out_cap=cap, fit=fit, pad=pad, interp=interp)
    if chips_cap is None:
        b.stream.synchronize()
        room = int(np.clip(b.d_counts.cpu().numpy(), 0, b.cap).sum())
    else:
        room = int(chips_cap)
    d_chips = torch.empty((max(room, 1), out_h, out_w, 3), dtype=torch.uint8, device=b.device)
    d_info = torch.empty((max(room, 1), CHIP_DTYPE.itemsize), dtype=torch.uint8, device=b.device)
    d_first = torch.empty(n + 1, dtype=torch.int32, device=b.device)
    crop = crop_records_yuv_device if is_yuv(fmt) else crop_records_device
    crop(b.d_px.data_ptr(), b.nbytes, fmt, b.d_pictures.data_ptr(), b.d_dets.data_ptr(), b.d_counts.data_ptr(), n, b.cap, out_h, out_w,
         d_chips.data_ptr(), room, d_first.data_ptr(), d_info.data_ptr(), order=order_code, margin_permille=permille, square=square,
         stream=b.stream.cuda_stream)
    b.stream.synchronize()
    b.check_totals("detect_chips")
    first = d_first.cpu().numpy()
    if int(first[n]) > room:
        raise ImagesError(f"detect_chips: {int(first[n])} boxes in the batch, chips_cap holds {room}")
    chips = d_chips.cpu().numpy()
    info = d_info.cpu().numpy().view(CHIP_DTYPE).reshape(-1)
    return b.boxes(np.diff(first)), [chips[a:z] for a, z in zip(first, first[1:])], [info[a:z] for a, z in zip(first, first[1:])]


def _colour_code(colour):
    """(R, G, B) -- for NV12 / NV21 surfaces (Y, U, V) -- or the integer 0x00RRGGBB -> that integer"""
    if isinstance(colour, (tuple, list, np.ndarray)):
        c = [int(v) for v in colour]
        if len(c) != 3 or not all(0 <= v <= 255 for v in c):
            raise ValueError(f"colour {colour!r}: three bytes")
        return c[0] << 16 | c[1] << 8 | c[2]
    if not 0 <= int(colour) <= 0xFFFFFF:
        raise ValueError(f"colour {colour!r}: 0x00RRGGBB")
    return int(colour)


def redact_records_device(d_pixels, pixels_bytes, fmt, d_images, d_dets, d_counts, n, cap, d_first, d_status, mode="mosaic", block=8, colour=0,
                          margin_permille=0, square=False, stream=None):
    """The regions of the records of a batch of packed pictures pixelated or filled IN PLACE (yf_images_redact_records_device): d_images
    IMAGE_DTYPE[n], d_dets yf_det[n][cap], d_counts int32[n]; d_pixels is written.  mode "mosaic": block 4, 8, 16, 32 or 64, a grid
    anchored at each picture's pixel (0, 0); mode "fill": block 0, colour 0x00RRGGBB or (R, G, B).  d_first int32[n + 1] and d_status
    int32[n] (1: the picture's descriptor is invalid, the picture untouched) are written.  For the mosaic the pictures of different frames
    must not share bytes.  The definition: csrc/yf_images_redact.h, ptq.redact_u8."""
    _call("redact_records_device", n, d_pixels, pixels_bytes, _packed_code(fmt, "redact_records_device"), d_images, d_dets, d_counts, n, cap,
          _code(REDACT_MODES, mode, MODE_WHAT), block, _colour_code(colour), margin_permille, YF_CROP_SQUARE if square else 0, d_first, d_status,
          stream)


def redact_records_yuv_device(d_pixels, pixels_bytes, fmt, d_images, d_dets, d_counts, n, cap, d_first, d_status, mode="mosaic", block=8,
                              colour=0, margin_permille=0, square=False, stream=None):
    """`redact_records_device` for NV12 / NV21 surfaces, redacted where they lie (yf_images_redact_records_yuv_device): d_images
    YUV_IMAGE_DTYPE[n]; colour 0x00YYUUVV or (Y, U, V).  ptq.redact_yuv420sp."""
    _call("redact_records_yuv_device", n, d_pixels, pixels_bytes, _yuv_code(fmt), d_images, d_dets, d_counts, n, cap,
          _code(REDACT_MODES, mode, MODE_WHAT), block, _colour_code(colour), margin_permille, YF_CROP_SQUARE if square else 0, d_first, d_status,
          stream)


def _strided(buf, offset, rows, row_bytes, pitch):
    return np.lib.stride_tricks.as_strided(buf[offset:], shape=(rows, row_bytes), strides=(pitch, 1))


def _pictures_back(b, fmt):
    """the pictures of a staged batch as they lie on the device now, in the caller's shapes: new arrays (NV12 / NV21: (y, uv) pairs);
    after a synchronise"""
    yuv = is_yuv(fmt)
    buf = b.d_px.cpu().numpy()
    desc = b.d_pictures.cpu().numpy().view(YUV_IMAGE_DTYPE if yuv else IMAGE_DTYPE).reshape(-1)
    pictures = []
    for e in desc:
        h, w = int(e["height"]), int(e["width"])
        if yuv:
            pictures.append((_strided(buf, int(e["offset_y"]), h, w, int(e["stride_y"])).copy(),
                             _strided(buf, int(e["offset_uv"]), h // 2, w, int(e["stride_uv"])).copy()))
        else:
            C = CHANNELS[format_code(fmt)]
            pictures.append(_strided(buf, int(e["offset"]), h, w * C, int(e["row_stride"])).copy().reshape(h, w, C))
    return pictures


def _tracker_steps(tracker, n, steps, layout, iou_threshold):
    """the checks of a `detect_*` call's tracker arguments -> steps (None: as many as the n images make)"""
    steps = n // tracker.streams if steps is None else int(steps)
    if steps < 0 or n != tracker.streams * steps:
        raise ValueError(f"{n} images: {tracker.streams} streams x {steps} steps")
    if iou_threshold is None:
        raise ValueError("iou_threshold None: the tracker takes suppressed records")
    _code(TRACK_LAYOUTS, layout, LAYOUT_WHAT)
    return steps


def detect_redacted(network, images, mode="mosaic", block=8, colour=(0, 0, 0), margin=0.0, square=False, fmt="bgr", cap=None,
                    iou_threshold=0.4, size=56, dtype="int8", tile=None, stride=None, device=None, fit="stretch", pad=114, interp="linear",
                    tracker=None, steps=None, layout="time"):
    """`detect` (with `tile`: `detect_tiled`, whose `tile` and `stride` these are; fit, pad as in `detect`), and every kept box hidden in its picture on the GPU,
    on the same stream, in the pixels that are already there: mode "mosaic" pixelates the blocks of `block` x `block` pixels (4, 8, 16,
    32 or 64; the grid starts at the picture's pixel (0, 0)) that the box touches, each block to its mean; mode "fill" writes `colour`,
    (R, G, B) whatever the byte order of `fmt` -- for NV12 / NV21 surfaces (Y, U, V) -- into the box, and `block` is not used.  `margin`
    and `square` grow the box as in `detect_chips` (csrc/yf_images_crop.h, `ptq.crop_region`).  fmt, cap, iou_threshold, size, dtype,
    device as in `detect`; with `tile`, cap is `detect_tiled`'s out_cap and the parent pictures are redacted.
    With `tracker` (a `Tracker`; `images` are its next `steps` frames in `layout`, as in `detect_drawn`) the tracker is updated with the
    kept boxes on the same stream and the REPORTED TRACKS are hidden, held-over ones included: a face the detector misses for a few
    frames stays hidden -- with `Tracker(motion=...)` where its filter says it has moved to.
    Returns (pictures, boxes): the redacted pictures in the caller's shapes, new arrays (NV12 / NV21: (y, uv) pairs) -- the caller's
    arrays are not changed --, and per image the int32 [k, 4] array `detect` returns; with a tracker (pictures, tracks),
    `detect_tracked`'s tuples.  The definition is the library's own: csrc/yf_images_redact.h, restated as `ptq.redact_u8` and
    `ptq.redact_yuv420sp`."""
    mode_code = _code(REDACT_MODES, mode, MODE_WHAT)
    block = 0 if mode_code == YF_REDACT_FILL else int(block)
    if mode_code == YF_REDACT_MOSAIC and block not in (4, 8, 16, 32, 64):
        raise ValueError(f"block {block!r}: 4, 8, 16, 32 or 64")
    colour_code = _colour_code(colour)
    permille = _permille(margin)
    n = len(images)
    if tracker is not None:
        steps = _tracker_steps(tracker, n, steps, layout, iou_threshold)
        device = tracker.device.index
    if n == 0:
        return [], []
    import torch
    yuv = is_yuv(fmt)
    if tile is not None:
        _packed_code(fmt, "detect_redacted(tile=...)")
    b = _stage(network, images, fmt, cap, device, iou_threshold, size, dtype, tile, stride, True, out_cap=cap, fit=fit, pad=pad, interp=interp)
    d_first = torch.empty(n + 1, dtype=torch.int32, device=b.device)
    d_status = torch.empty(n, dtype=torch.int32, device=b.device)      # the redaction's own: the staging's status does not raise here
    redact = redact_records_yuv_device if yuv else redact_records_device
    d_dets, d_counts, rec_cap = b.d_dets, b.d_counts, b.cap
    if tracker is not None:
        d_dets, d_info, d_counts, _ = tracker.update(b.d_dets, b.d_counts, steps, layout, cap=b.cap, stream=b.stream.cuda_stream)
        rec_cap = d_dets.shape[1]
    redact(b.d_px.data_ptr(), b.nbytes, fmt, b.d_pictures.data_ptr(), d_dets.data_ptr(), d_counts.data_ptr(), n, rec_cap,
           d_first.data_ptr(), d_status.data_ptr(), mode=mode_code, block=block, colour=colour_code, margin_permille=permille, square=square,
           stream=b.stream.cuda_stream)
    b.stream.synchronize()
    b.check_totals("detect_redacted")
    bad = np.nonzero(d_status.cpu().numpy())[0]
    if bad.size:
        raise ImagesError(f"detect_redacted: the descriptor of image {int(bad[0])} is invalid")
    if tracker is not None:
        return _pictures_back(b, fmt), _track_tuples(d_dets, d_info, d_counts, n)
    return _pictures_back(b, fmt), b.boxes(np.diff(d_first.cpu().numpy()))


def blur_workspace(records_cap, grid):
    """The bytes of the workspace of a blur of at most `records_cap` records at `grid` (yf_images_blur_workspace): records_cap * grid *
    grid * 4 rounded up to 16; 0 for arguments the call refuses."""
    return int(load().yf_images_blur_workspace(records_cap, grid))


def blur_records_device(d_pixels, pixels_bytes, fmt, d_images, d_dets, d_counts, n, cap, d_work, work_bytes, records_cap, d_first, d_status,
                        grid=8, colour=0, margin_permille=0, square=False, stream=None):
    """The regions of the records of a batch of packed pictures blurred IN PLACE (yf_images_blur_records_device): every region becomes a
    grid of at most grid x grid means of its own pixels (no cell narrower than 4 pixels), resized back to the region as cv2.resize does.
    d_images IMAGE_DTYPE[n], d_dets yf_det[n][cap], d_counts int32[n]; d_pixels is read and written.  d_work: `blur_workspace(records_cap,
    grid)` bytes, 16-byte aligned; record k = first[f] + s keeps its grid in slot k, and a record with k >= records_cap is filled with
    colour (0x00RRGGBB or (R, G, B)) instead.  d_first int32[n + 1] and d_status int32[n] are written: bit 0 the picture's descriptor is
    invalid (the picture untouched), bit 1 a record of the frame was filled for lack of a slot.  A pixel in several regions gets the value of
    the lowest slot; a second call blurs the blur.  The pictures of different frames must not share bytes.  The definition:
    csrc/yf_images_blur.h, ptq.blur_u8."""
    _call("blur_records_device", n, d_pixels, pixels_bytes, _packed_code(fmt, "blur_records_device"), d_images, d_dets, d_counts, n, cap,
          grid, _colour_code(colour), margin_permille, YF_CROP_SQUARE if square else 0, d_work, work_bytes, records_cap, d_first, d_status, stream)


def blur_records_yuv_device(d_pixels, pixels_bytes, fmt, d_images, d_dets, d_counts, n, cap, d_work, work_bytes, records_cap, d_first,
                            d_status, grid=8, colour=0, margin_permille=0, square=False, stream=None):
    """`blur_records_device` for NV12 / NV21 surfaces, blurred where they lie (yf_images_blur_records_yuv_device): d_images
    YUV_IMAGE_DTYPE[n]; the Y plane and the chroma plane each get a grid of their own; colour 0x00YYUUVV or (Y, U, V).
    ptq.blur_yuv420sp."""
    _call("blur_records_yuv_device", n, d_pixels, pixels_bytes, _yuv_code(fmt), d_images, d_dets, d_counts, n, cap, grid, _colour_code(colour),
          margin_permille, YF_CROP_SQUARE if square else 0, d_work, work_bytes, records_cap, d_first, d_status, stream)


def detect_blurred(network, images, grid=8, colour=(0, 0, 0), margin=0.0, square=False, fmt="bgr", cap=None, iou_threshold=0.4, size=56,
                   dtype="int8", tile=None, stride=None, device=None, fit="stretch", pad=114, interp="linear", tracker=None, steps=None,
                   layout="time"):
    """`detect` (with `tile`: `detect_tiled`, whose `tile` and `stride` these are; fit, pad as in `detect`), and every kept box blurred in its picture on the GPU, on
    the same stream, in the pixels that are already there: the box becomes a grid of at most `grid` x `grid` (1 to 16) means of its own
    pixels, resized back to the box -- every face gets the same number of cells, so a large face is hidden as well as a small one.
    `margin` and `square` grow the box as in `detect_chips`.  The workspace is sized for every record the batch can hold, so no box is
    ever filled with `colour` for lack of room.  fmt, cap, iou_threshold, size, dtype, device as in `detect`; with `tile`, cap is
    `detect_tiled`'s out_cap and the parent pictures are blurred.  `tracker`, `steps`, `layout` as in `detect_redacted`: the reported
    tracks are blurred, held-over ones included.
    Returns (pictures, boxes) as `detect_redacted` does; with a tracker (pictures, tracks).  The definition is the library's own: csrc/yf_images_blur.h, restated as
    `ptq.blur_u8` and `ptq.blur_yuv420sp`."""
    grid = int(grid)
    if not 1 <= grid <= BLUR_MAX_GRID:
        raise ValueError(f"grid {grid!r}: 1 to {BLUR_MAX_GRID}")
    colour_code = _colour_code(colour)
    permille = _permille(margin)
    n = len(images)
    if tracker is not None:
        steps = _tracker_steps(tracker, n, steps, layout, iou_threshold)
        device = tracker.device.index
    if n == 0:
        return [], []
    import torch
    yuv = is_yuv(fmt)
    if tile is not None:
        _packed_code(fmt, "detect_blurred(tile=...)")
    b = _stage(network, images, fmt, cap, device, iou_threshold, size, dtype, tile, stride, True, out_cap=cap, fit=fit, pad=pad, interp=interp)
    d_dets, d_counts, rec_cap = b.d_dets, b.d_counts, b.cap
    if tracker is not None:
        d_dets, d_info, d_counts, _ = tracker.update(b.d_dets, b.d_counts, steps, layout, cap=b.cap, stream=b.stream.cuda_stream)
        rec_cap = d_dets.shape[1]
    records_cap = n * rec_cap
    room = blur_workspace(records_cap, grid)
    d_work = torch.empty(room, dtype=torch.uint8, device=b.device)
    d_first = torch.empty(n + 1, dtype=torch.int32, device=b.device)
    d_status = torch.empty(n, dtype=torch.int32, device=b.device)
    blur = blur_records_yuv_device if yuv else blur_records_device
    blur(b.d_px.data_ptr(), b.nbytes, fmt, b.d_pictures.data_ptr(), d_dets.data_ptr(), d_counts.data_ptr(), n, rec_cap, d_work.data_ptr(),
         room, records_cap, d_first.data_ptr(), d_status.data_ptr(), grid=grid, colour=colour_code, margin_permille=permille, square=square,
         stream=b.stream.cuda_stream)
    b.stream.synchronize()
    b.check_totals("detect_blurred")
    bad = np.nonzero(d_status.cpu().numpy() & 1)[0]
    if bad.size:
        raise ImagesError(f"detect_blurred: the descriptor of image {int(bad[0])} is invalid")
    if tracker is not None:
        return _pictures_back(b, fmt), _track_tuples(d_dets, d_info, d_counts, n)
    return _pictures_back(b, fmt), b.boxes(np.diff(d_first.cpu().numpy()))


def track_state_bytes(streams):
    """The bytes of the track state of `streams` streams (yf_images_track_state_bytes): 2824 each.  All zero is the empty state."""
    return int(load().yf_images_track_state_bytes(streams))


def track_device(d_dets, d_counts, streams, steps, layout, cap, params, d_state, d_out, d_info, d_out_counts, out_cap, d_status=None,
                 stream=None):
    """The records of streams * steps frames associated with the track state of their streams (yf_images_track_device): d_dets
    yf_det[n][cap], d_counts int32[n], frame t * streams + s (layout "time") or s * steps + t ("stream"); params = (match_iou, min_hits,
    max_misses); d_state the streams' state (`track_state_bytes`, read and written); d_out yf_det[n][out_cap], d_info
    TRACK_INFO_DTYPE[n][out_cap], d_out_counts int32[n], d_status int32[n] or None are written.  The definition: csrc/yf_images_track.h,
    ptq.track_step.  Returns n."""
    lib = load()
    p = YfTrackParams(float(params[0]), int(params[1]), int(params[2]))
    rc = lib.yf_images_track_device(d_dets, d_counts, streams, steps, _code(TRACK_LAYOUTS, layout, LAYOUT_WHAT), cap, ctypes.byref(p), d_state,
                                    d_out, d_info, d_out_counts, out_cap, d_status, stream)
    if rc != streams * steps or rc < 0:
        raise ImagesError(f"yf_images_track_device: {(lib.yf_images_last_error_text() or b'').decode()} (returned {rc})")
    return rc


def track_motion_state_bytes(streams):
    """The bytes of the state of `streams` streams of the tracker with a motion model (yf_images_track_motion_state_bytes): 7176 each.
    All zero is the empty state.  Not the format of `track_state_bytes`: neither state may be passed to the other entry."""
    return int(load().yf_images_track_motion_state_bytes(streams))


def track_motion_device(d_dets, d_counts, streams, steps, layout, cap, params, d_state, d_out, d_info, d_out_counts, out_cap, d_status=None,
                        stream=None):
    """`track_device` with a motion model (yf_images_track_motion_device): params = (match_iou, min_hits, max_misses, alpha, beta, damp,
    smooth), the gains of the constant-velocity filter in [0, 256] (1/256), smooth 0 or 1; d_state the streams' state of
    `track_motion_state_bytes` (read and written).  A held-over track is written with the box the filter moved on; with smooth 1 a matched
    track with its filtered box.  The definition: csrc/yf_images_motion.h, ptq.track_motion_step.  Returns n."""
    lib = load()
    p = YfTrackMotionParams(YfTrackParams(float(params[0]), int(params[1]), int(params[2])), *(int(v) for v in params[3:7]))
    rc = lib.yf_images_track_motion_device(d_dets, d_counts, streams, steps, _code(TRACK_LAYOUTS, layout, LAYOUT_WHAT), cap, ctypes.byref(p),
                                           d_state, d_out, d_info, d_out_counts, out_cap, d_status, stream)
    if rc != streams * steps or rc < 0:
        raise ImagesError(f"yf_images_track_motion_device: {(lib.yf_images_last_error_text() or b'').decode()} (returned {rc})")
    return rc


def track_motion_assign_device(d_dets, d_counts, streams, steps, layout, cap, params, assign, d_state, d_out, d_info, d_out_counts, out_cap,
                               d_status=None, stream=None):
    """`track_motion_device` with a choice of the match (yf_images_track_motion_assign_device): assign "greedy", that entry under another
    name; "optimal", the maximum-weight assignment over the eligible pairs -- maximum total IoU at 2^-30 resolution, its ties settled
    by one prescribed procedure -- in the place of the greedy match, so that two faces passing each other keep their ids where greedy
    strands one detection.  The state is `track_motion_state_bytes`' (7176 bytes per stream).  The definition:
    csrc/yf_images_assign.h, ptq.track_assign_match, ptq.track_motion_step(assign="optimal").  Returns n."""
    lib = load()
    p = YfTrackMotionParams(YfTrackParams(float(params[0]), int(params[1]), int(params[2])), *(int(v) for v in params[3:7]))
    code = _code(ASSIGNS, assign, ASSIGN_WHAT)
    rc = lib.yf_images_track_motion_assign_device(d_dets, d_counts, streams, steps, _code(TRACK_LAYOUTS, layout, LAYOUT_WHAT), cap, ctypes.byref(p),
                                                  code, d_state, d_out, d_info, d_out_counts, out_cap, d_status, stream)
    if rc != streams * steps or rc < 0:
        raise ImagesError(f"yf_images_track_motion_assign_device: {(lib.yf_images_last_error_text() or b'').decode()} (returned {rc})")
    return rc


class Tracker:
    """The track state of `streams` video streams on the device, and the parameters of their association.  match_iou=0.3, min_hits=1,
    max_misses=5 are the library's choice for faces at a video rate -- a box that moved by less than about half its side still matches,
    every detection is reported at once, a face is held over for five frames -- not something the reference states or a measurement.
    `update` takes the records of the next steps; `reset` empties every stream (an all-zero state is the empty state).
    `motion`: None, the tracker as it is -- a held-over box stays where it was last seen (`track_device`, 2824 bytes per stream); True, a
    constant-velocity filter per edge at the suggested gains `MOTION_GAINS` (a choice, not a measurement), or a triple (alpha, beta,
    damp) in 1/256 -- a held-over box moves on and the match is taken against the predicted box (`track_motion_device`, 7176 bytes per
    stream).  `smooth` (with motion): a matched track reports its filtered box, not its detection.
    `assign`: "greedy", the match as it is; "optimal", the maximum-weight assignment of csrc/yf_images_assign.h in its place
    (`track_motion_assign_device`): two faces that pass each other keep their ids where greedy strands a detection.  With motion=None
    it runs on the motion state at gains (256, 0, 256, 0) -- the plain tracker's results with the other match -- SO THE STATE IS THEN 7176
    BYTES PER STREAM, not 2824 (`self.motion` stays None)."""

    def __init__(self, streams, match_iou=0.3, min_hits=1, max_misses=5, device=None, motion=None, smooth=False, assign="greedy"):
        import torch
        if int(streams) < 1:
            raise ValueError(f"streams {streams!r}: at least 1")
        self.params = (float(match_iou), int(min_hits), int(max_misses))
        self.assign = ASSIGN_NAMES[_code(ASSIGNS, assign, ASSIGN_WHAT)]
        if motion is None or motion is False:
            if smooth:
                raise ValueError("smooth: only with motion")
            self.motion = None
        else:
            gains = MOTION_GAINS if motion is True else tuple(int(v) for v in motion)
            if len(gains) != 3 or not all(0 <= g <= 256 for g in gains):
                raise ValueError(f"motion {motion!r}: True or (alpha, beta, damp), each 0..256")
            self.motion = gains + (1 if smooth else 0,)
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self.reset(streams)

    def reset(self, streams=None):
        """every stream empty again; with `streams`, a new number of them"""
        import torch
        if streams is not None:
            self.streams = int(streams)
            state_bytes = TRACK_STATE_BYTES if self.motion is None and self.assign == "greedy" else TRACK_MOTION_STATE_BYTES
            self.d_state = torch.zeros((self.streams, state_bytes), dtype=torch.uint8, device=self.device)
        else:
            self.d_state.zero_()

    def update(self, d_dets, d_counts, steps, layout="time", cap=None, out_cap=TRACK_SLOTS, stream=None):
        """The next `steps` frames of every stream: d_dets uint8 [streams * steps, cap, 28] and d_counts int32 [streams * steps], tensors on
        the tracker's device (the output of a suppression).  -> (d_out uint8 [n, out_cap, 28], d_info uint8 [n, out_cap, 16], d_out_counts
        int32 [n], d_status int32 [n]) on the stream given (default: the device's current one), not synchronised."""
        import torch
        n = self.streams * int(steps)
        cap = d_dets.shape[1] if cap is None else cap
        d_out = torch.empty((n, out_cap, binding.DET_DTYPE.itemsize), dtype=torch.uint8, device=self.device)
        d_info = torch.empty((n, out_cap, TRACK_INFO_DTYPE.itemsize), dtype=torch.uint8, device=self.device)
        d_out_counts = torch.empty(n, dtype=torch.int32, device=self.device)
        d_status = torch.empty(n, dtype=torch.int32, device=self.device)
        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        if self.assign == "optimal":
            track_motion_assign_device(d_dets.data_ptr(), d_counts.data_ptr(), self.streams, int(steps), layout, cap,
                                       self.params + ((256, 0, 256, 0) if self.motion is None else self.motion), "optimal",
                                       self.d_state.data_ptr(), d_out.data_ptr(), d_info.data_ptr(), d_out_counts.data_ptr(), out_cap,
                                       d_status.data_ptr(), stream)
        elif self.motion is None:
            track_device(d_dets.data_ptr(), d_counts.data_ptr(), self.streams, int(steps), layout, cap, self.params, self.d_state.data_ptr(),
                         d_out.data_ptr(), d_info.data_ptr(), d_out_counts.data_ptr(), out_cap, d_status.data_ptr(), stream)
        else:
            track_motion_device(d_dets.data_ptr(), d_counts.data_ptr(), self.streams, int(steps), layout, cap, self.params + self.motion,
                                self.d_state.data_ptr(), d_out.data_ptr(), d_info.data_ptr(), d_out_counts.data_ptr(), out_cap,
                                d_status.data_ptr(), stream)
        return d_out, d_info, d_out_counts, d_status


def describe_records_device(d_pixels, pixels_bytes, fmt, d_images, d_dets, d_counts, n, cap, d_desc, d_first, d_status, margin_permille=0,
                            square=False, stream=None):
    """An appearance descriptor per record of a batch of packed pictures (yf_images_describe_records_device): d_images IMAGE_DTYPE[n],
    d_dets yf_det[n][cap], d_counts int32[n]; d_pixels is only read.  d_desc FACE_DESC_DTYPE[n][cap] is written in the slots of the first
    min(max(count, 0), cap) records of each frame: flags 1 and the 8 x 8 grid of the region's mean luma, or 68 zero bytes for a record
    without a region, with a region narrower or lower than 8 pixels, or in an invalid picture.  d_first int32[n + 1] and d_status
    int32[n] (1: the picture's descriptor is invalid) are written.  A tiny template, not a learned embedding.  The definition:
    csrc/yf_images_describe.h, ptq.describe_u8."""
    _call("describe_records_device", n, d_pixels, pixels_bytes, _packed_code(fmt, "describe_records_device"), d_images, d_dets, d_counts, n,
          cap, margin_permille, YF_CROP_SQUARE if square else 0, d_desc, d_first, d_status, stream)


def describe_records_yuv_device(d_pixels, pixels_bytes, fmt, d_images, d_dets, d_counts, n, cap, d_desc, d_first, d_status, margin_permille=0,
                                square=False, stream=None):
    """`describe_records_device` for NV12 / NV21 surfaces (yf_images_describe_records_yuv_device): d_images YUV_IMAGE_DTYPE[n]; only the
    Y plane is read.  ptq.describe_yuv420sp."""
    _call("describe_records_yuv_device", n, d_pixels, pixels_bytes, _yuv_code(fmt), d_images, d_dets, d_counts, n, cap, margin_permille,
          YF_CROP_SQUARE if square else 0, d_desc, d_first, d_status, stream)


def reid_state_bytes(streams):
    """The bytes of the re-identification state of `streams` streams (yf_images_reid_state_bytes): 5128 each.  All zero is the empty
    state."""
    return int(load().yf_images_reid_state_bytes(streams))


def reid_device(d_info, d_out_counts, d_desc, out_cap, streams, steps, layout, params, d_state, d_info_out, d_what=None, d_status=None,
                stream=None):
    """The ids of a tracker's output rewritten by appearance (yf_images_reid_device): d_info TRACK_INFO_DTYPE[n][out_cap] and d_out_counts
    int32[n] as a tracker wrote them, d_desc FACE_DESC_DTYPE[n][out_cap] the descriptors of its boxes, n = streams * steps frames in
    `layout`; params = (max_distance, max_age, blend); d_state the streams' state (`reid_state_bytes`, read and written).  d_info_out
    (may be d_info) gets every record with its id replaced: a track born while a lost one that looks the same (distance <=
    max_distance, lost for at most max_age steps) is in the table reports the lost one's id.  The records keep the tracker's order.
    d_what int32[n][out_cap] or None: 0 void, 1 known, 2 re-identified, 3 born; d_status int32[n] or None.  The definition:
    csrc/yf_images_reid.h, ptq.reid_step.  Returns n."""
    lib = load()
    p = YfReidParams(int(params[0]), int(params[1]), int(params[2]))
    rc = lib.yf_images_reid_device(d_info, d_out_counts, d_desc, out_cap, streams, steps, _code(TRACK_LAYOUTS, layout, LAYOUT_WHAT),
                                   ctypes.byref(p), d_state, d_info_out, d_what, d_status, stream)
    if rc != streams * steps or rc < 0:
        raise ImagesError(f"yf_images_reid_device: {(lib.yf_images_last_error_text() or b'').decode()} (returned {rc})")
    return rc


class ReId:
    """The re-identification state of `streams` video streams on the device (csrc/yf_images_reid.h): the stage behind a `Tracker` that
    lets a lost track keep its id.  `update` describes the tracker's reported boxes from the pictures where they lie and rewrites the
    ids on the same stream; `reset` empties every stream (an all-zero state is the empty state); `states` downloads them.
    max_distance: the largest distance (mean-removed sum of absolute differences of two 8 x 8 luma grids, times 64) at which a new
    track takes over a lost identity -- the default `REID_MAX_DISTANCE` is a choice made on synthetic textures
    (profiles/reid_bench.txt), not a figure from labelled video.  max_age: the steps a lost identity is remembered.  blend: how much of
    a new descriptor enters the stored one per frame, in 1/256.  margin, square: the region of a box, as in `detect_chips`."""

    def __init__(self, streams, max_distance=None, max_age=REID_MAX_AGE, blend=REID_BLEND, margin=0.0, square=False, device=None):
        import torch
        if int(streams) < 1:
            raise ValueError(f"streams {streams!r}: at least 1")
        max_distance = REID_MAX_DISTANCE if max_distance is None else int(max_distance)
        if max_distance < 0 or int(max_age) < 0 or not 0 <= int(blend) <= 256:
            raise ValueError(f"max_distance {max_distance!r}, max_age {max_age!r}: at least 0; blend {blend!r}: 0 to 256")
        self.streams, self.params = int(streams), (max_distance, int(max_age), int(blend))
        self.permille, self.square = _permille(margin), bool(square)
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self.d_state = torch.zeros((self.streams, REID_STATE_BYTES), dtype=torch.uint8, device=self.device)

    def reset(self):
        """every stream empty again"""
        self.d_state.zero_()

    def update(self, d_px, nbytes, fmt, d_pictures, d_out, d_info, d_out_counts, steps, layout="time", with_what=False, stream=None):
        """The next `steps` frames of every stream: d_px / nbytes / d_pictures the pictures and their descriptors on the device as the
        crop entries take them, d_out, d_info, d_out_counts a `Tracker.update`'s output for them.  d_info is REWRITTEN in place.  ->
        (d_desc uint8 [n, out_cap, 68], d_what int32 [n, out_cap] or None, d_status int32 [n]: the describe's) on the stream given
        (default: the device's current one), not synchronised."""
        import torch
        n, out_cap = self.streams * int(steps), d_out.shape[1]
        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        d_desc = torch.empty((n, out_cap, FACE_DESC_DTYPE.itemsize), dtype=torch.uint8, device=self.device)
        d_first = torch.empty(n + 1, dtype=torch.int32, device=self.device)
        d_status = torch.empty(n, dtype=torch.int32, device=self.device)
        d_what = torch.empty((n, out_cap), dtype=torch.int32, device=self.device) if with_what else None
        describe = describe_records_yuv_device if is_yuv(fmt) else describe_records_device
        describe(d_px.data_ptr(), nbytes, fmt, d_pictures.data_ptr(), d_out.data_ptr(), d_out_counts.data_ptr(), n, out_cap, d_desc.data_ptr(),
                 d_first.data_ptr(), d_status.data_ptr(), margin_permille=self.permille, square=self.square, stream=stream)
        reid_device(d_info.data_ptr(), d_out_counts.data_ptr(), d_desc.data_ptr(), out_cap, self.streams, int(steps), layout, self.params,
                    self.d_state.data_ptr(), d_info.data_ptr(), None if d_what is None else d_what.data_ptr(), None, stream)
        return d_desc, d_what, d_status

    def states(self):
        """-> REID_STATE_DTYPE [streams], after a synchronise (the download)"""
        return self.d_state.cpu().numpy().view(REID_STATE_DTYPE).reshape(self.streams)


def _reid_after(reid, tracker, b, fmt, d_out, d_info, d_out_counts, steps, layout):
    """`reid` (a `ReId` or None) behind `tracker` on the staged batch b: the tracker's output described from the pictures where they lie
    and its ids rewritten in d_info, on b's stream"""
    if reid is None:
        return
    _check_reid(reid, tracker)
    reid.update(b.d_px, b.nbytes, fmt, b.d_pictures, d_out, d_info, d_out_counts, steps, layout, stream=b.stream.cuda_stream)


def _check_reid(reid, tracker):
    if reid is not None and (reid.streams != tracker.streams or reid.device != tracker.device):
        raise ValueError(f"reid: {reid.streams} streams on {reid.device}, the tracker has {tracker.streams} on {tracker.device}")


def _track_tuples(d_out, d_info, d_out_counts, n):
    """a tracker's output of n frames -> per frame the list of (id, x1, y1, x2, y2, conf, hits, misses); after a synchronise"""
    out = d_out.cpu().numpy().view(binding.DET_DTYPE).reshape(n, -1)
    info = d_info.cpu().numpy().view(TRACK_INFO_DTYPE).reshape(n, -1)
    counts = d_out_counts.cpu().numpy()
    return [[(int(i["id"]), int(d["x1"]), int(d["y1"]), int(d["x2"]), int(d["y2"]), float(d["conf"]), int(i["hits"]), int(i["misses"]))
             for d, i in zip(out[f, :counts[f]], info[f, :counts[f]])] for f in range(n)]


def detect_tracked(network, images, tracker, steps, layout="time", fmt="bgr", iou_threshold=0.4, size=56, dtype="int8", fit="stretch", pad=114, interp="linear",
                   reid=None):
    """`detect` with the suppression for the next `steps` frames of the `tracker`'s streams, and the kept boxes associated with its track
    state on the same stream: `images` holds tracker.streams * steps pictures, frame t of stream s at index t * streams + s (layout
    "time": one frame of every camera per step) or s * steps + t ("stream": a clip per stream).  fmt, iou_threshold (not None: the tracker
    takes a frame's records in descending confidence), size, dtype, fit, pad as in `detect`; the tracker's device is used.
    Returns per frame a list of (id, x1, y1, x2, y2, conf, hits, misses) in ascending id: the tracks reported for that frame, a held-over
    one (misses > 0) with the box it was last seen at -- with a `Tracker(motion=...)`, the box its filter moved on.  The tracker carries on from there at the next call.  The definition is the
    library's own: csrc/yf_images_track.h, restated as `ptq.track_step`.
    `reid`: a `ReId` of the tracker's streams and device; the reported boxes are then described from the pictures where they lie and the
    ids rewritten on the same stream (csrc/yf_images_reid.h): a face that returns after its track died reports its old id.  The tuples
    carry the rewritten ids and keep the tracker's order, so they are then no longer in ascending id."""
    steps = int(steps)
    if steps < 0 or len(images) != tracker.streams * steps:
        raise ValueError(f"{len(images)} images: {tracker.streams} streams x {steps} steps")
    if iou_threshold is None:
        raise ValueError("iou_threshold None: the tracker takes suppressed records")
    _code(TRACK_LAYOUTS, layout, LAYOUT_WHAT)
    _check_reid(reid, tracker)
    n = len(images)
    if n == 0:
        return []
    b = _stage(network, images, fmt, None, tracker.device.index, iou_threshold, size, dtype, fit=fit, pad=pad, interp=interp)
    d_out, d_info, d_out_counts, d_status = tracker.update(b.d_dets, b.d_counts, steps, layout, stream=b.stream.cuda_stream)
    _reid_after(reid, tracker, b, fmt, d_out, d_info, d_out_counts, steps, layout)
    b.stream.synchronize()
    return _track_tuples(d_out, d_info, d_out_counts, n)


def score_state_bytes(streams):
    """The bytes of the score state of `streams` streams (yf_images_score_state_bytes): 3136 each.  All zero is the empty state."""
    return int(load().yf_images_score_state_bytes(streams))


def score_tracks_device(d_out, d_info, d_out_counts, out_cap, d_gt, d_gt_counts, gt_cap, streams, steps, layout, score_iou, d_state,
                        d_match=None, d_status=None, stream=None):
    """The CLEAR-MOT score of a tracker's output against labelled identities (yf_images_score_tracks_device): d_out yf_det[n][out_cap],
    d_info TRACK_INFO_DTYPE[n][out_cap], d_out_counts int32[n] as `track_device` and its siblings wrote them; d_gt
    GT_TRACK_DTYPE[n][gt_cap], d_gt_counts int32[n] (`pack_track_truth`); frame t * streams + s (layout "time") or s * steps + t
    ("stream"); d_state the streams' state (`score_state_bytes`, read and written: the counters and the per-object tables go on from call
    to call); d_match int32[n][gt_cap] or None: per labelled row the column of its hypothesis or -1; d_status int32[n] or None.  The
    definition: csrc/yf_images_score.h, ptq.track_score_step.  Returns n."""
    lib = load()
    rc = lib.yf_images_score_tracks_device(d_out, d_info, d_out_counts, out_cap, d_gt, d_gt_counts, gt_cap, streams, steps,
                                           _code(TRACK_LAYOUTS, layout, LAYOUT_WHAT), float(score_iou), d_state, d_match, d_status, stream)
    if rc != streams * steps or rc < 0:
        raise ImagesError(f"yf_images_score_tracks_device: {(lib.yf_images_last_error_text() or b'').decode()} (returned {rc})")
    return rc


def score_summary(states):
    """yf_images_score_summary of downloaded states (bytes, or an array of SCORE_STATE_BYTES per stream; host memory, no GPU call) -> a
    dict of yf_score_summary's fields: the eight counters summed over the streams, objects, mostly_tracked, mostly_lost, mota, motp."""
    lib = load()
    raw = np.ascontiguousarray(np.frombuffer(states, np.uint8) if isinstance(states, (bytes, bytearray)) else np.asarray(states)).view(np.uint8).reshape(-1)
    if raw.size % SCORE_STATE_BYTES:
        raise ValueError(f"{raw.size} bytes of state: {SCORE_STATE_BYTES} per stream")
    out = np.zeros(1, SCORE_SUMMARY_DTYPE)
    if lib.yf_images_score_summary(raw.ctypes.data if raw.size else None, raw.size // SCORE_STATE_BYTES, out.ctypes.data) != 0:
        raise ImagesError(f"yf_images_score_summary: {(lib.yf_images_last_error_text() or b'').decode()}")
    return {name: (float if name in ("mota", "motp") else int)(out[0][name]) for name in SCORE_SUMMARY_DTYPE.names}


def pack_track_truth(ground_truths, gt_cap=None):
    """per frame a list of (id, x1, y1, x2, y2) -- a labelled object's id (1 .. 256, one object per stream) and its box, edges inclusive
    pixels -- -> (GT_TRACK_DTYPE [n, gt_cap], int32 [n]); gt_cap None: the largest number of a frame (at least 1)"""
    rows = [[tuple(int(v) for v in t) for t in g] for g in ground_truths]
    gt_cap = max([1] + [len(r) for r in rows]) if gt_cap is None else int(gt_cap)
    if not 1 <= gt_cap <= SCORE_MAX_GT or any(len(r) > gt_cap for r in rows):
        raise ValueError(f"gt_cap {gt_cap}, {max([0] + [len(r) for r in rows])} labelled objects in one frame: at most {SCORE_MAX_GT}, and gt_cap holds every frame's")
    packed = np.zeros((len(rows), gt_cap), GT_TRACK_DTYPE)
    for f, r in enumerate(rows):
        if any(len(t) != 5 for t in r):
            raise ValueError(f"frame {f}: every labelled object is (id, x1, y1, x2, y2)")
        packed[f, :len(r)] = r
    return packed, np.array([len(r) for r in rows], np.int32)


class TrackScore:
    """The CLEAR-MOT score of `streams` video streams on the device (csrc/yf_images_score.h): misses, false positives, identity switches,
    MOTA and MOTP of what a `Tracker` reported against labelled identities, at IoU `score_iou`.  `update` scores the next steps, the
    records staying on the device; `summary` synchronises and downloads the states; `reset` empties every stream."""

    def __init__(self, streams, score_iou=0.5, device=None):
        import torch
        if int(streams) < 1:
            raise ValueError(f"streams {streams!r}: at least 1")
        if score_iou != score_iou:
            raise ValueError("score_iou is NaN")
        self.streams, self.score_iou = int(streams), float(score_iou)
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self.d_state = torch.zeros((self.streams, SCORE_STATE_BYTES), dtype=torch.uint8, device=self.device)

    def reset(self):
        """every stream's counters and per-object tables empty again"""
        self.d_state.zero_()

    def update(self, d_out, d_info, d_out_counts, d_gt, d_gt_counts, steps, layout="time", out_cap=None, gt_cap=None, with_match=False,
               stream=None):
        """The next `steps` frames of every stream: d_out, d_info, d_out_counts as `Tracker.update` returned them, d_gt uint8
        [n, gt_cap, 20] and d_gt_counts int32 [n] the uploaded arrays of `pack_track_truth`, tensors on this device.  -> (d_match int32
        [n, gt_cap] or None without `with_match`, d_status int32 [n]) on the stream given (default: the device's current one), not
        synchronised."""
        import torch
        n = self.streams * int(steps)
        out_cap = d_out.shape[1] if out_cap is None else out_cap
        gt_cap = d_gt.shape[1] if gt_cap is None else gt_cap
        d_match = torch.full((n, gt_cap), -1, dtype=torch.int32, device=self.device) if with_match else None
        d_status = torch.empty(n, dtype=torch.int32, device=self.device)
        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        score_tracks_device(d_out.data_ptr(), d_info.data_ptr(), d_out_counts.data_ptr(), out_cap, d_gt.data_ptr(), d_gt_counts.data_ptr(), gt_cap,
                            self.streams, int(steps), layout, self.score_iou, self.d_state.data_ptr(),
                            None if d_match is None else d_match.data_ptr(), d_status.data_ptr(), stream)
        return d_match, d_status

    def states(self):
        """the states as they are on the device, SCORE_STATE_DTYPE [streams]; synchronises"""
        return self.d_state.cpu().numpy().view(SCORE_STATE_DTYPE).reshape(self.streams)

    def summary(self):
        """-> `score_summary` of the states, after a synchronise (the download)"""
        return score_summary(self.states())


def evaluate_tracking(network, images, ground_truths, tracker, steps, layout="time", score_iou=0.5, score=None, fmt="bgr", iou_threshold=0.4,
                      size=56, dtype="int8", fit="stretch", pad=114, interp="linear", reid=None):
    """`detect_tracked` scored against labelled identities: the next `steps` frames of the `tracker`'s streams are detected, suppressed
    and associated as there (`images`, `layout`, fmt, iou_threshold, size, dtype, fit, pad, interp: as there), and what the tracker
    reports is scored on the same stream against `ground_truths` -- per frame, indexed as `images`, a list of (id, x1, y1, x2, y2) in that
    picture's pixels (`pack_track_truth`) -- without the records leaving the device; one synchronise at the end.  `score`: a `TrackScore`
    of the tracker's streams and device that carries the score across calls (its score_iou is used); None scores this call alone at
    `score_iou`.  Returns the summary (`TrackScore.summary`): the counters, objects, mostly_tracked, mostly_lost, mota, motp.  The
    definition: csrc/yf_images_score.h, restated as `ptq.track_score_step`.  `reid`: as in `detect_tracked`; the rewritten ids are
    scored."""
    steps = int(steps)
    if steps < 0 or len(images) != tracker.streams * steps:
        raise ValueError(f"{len(images)} images: {tracker.streams} streams x {steps} steps")
    if len(ground_truths) != len(images):
        raise ValueError(f"{len(images)} images, {len(ground_truths)} lists of labelled objects")
    if iou_threshold is None:
        raise ValueError("iou_threshold None: the tracker takes suppressed records")
    _code(TRACK_LAYOUTS, layout, LAYOUT_WHAT)
    _check_reid(reid, tracker)
    if score is None:
        score = TrackScore(tracker.streams, score_iou, tracker.device.index)
    elif score.streams != tracker.streams or score.device != tracker.device:
        raise ValueError(f"score: {score.streams} streams on {score.device}, the tracker has {tracker.streams} on {tracker.device}")
    gt, gt_counts = pack_track_truth(ground_truths)
    n = len(images)
    if n == 0:
        return score.summary()
    import torch
    b = _stage(network, images, fmt, None, tracker.device.index, iou_threshold, size, dtype, fit=fit, pad=pad, interp=interp)
    s = b.stream.cuda_stream
    with torch.cuda.stream(b.stream):
        d_gt = torch.from_numpy(gt.view(np.uint8).reshape(n, gt.shape[1], GT_TRACK_DTYPE.itemsize)).to(b.device)
        d_gt_counts = torch.from_numpy(gt_counts).to(b.device)
    d_out, d_info, d_out_counts, d_status = tracker.update(b.d_dets, b.d_counts, steps, layout, stream=s)
    _reid_after(reid, tracker, b, fmt, d_out, d_info, d_out_counts, steps, layout)
    score.update(d_out, d_info, d_out_counts, d_gt, d_gt_counts, steps, layout, stream=s)
    b.stream.synchronize()
    return score.summary()


# the colours of `detect_drawn`'s tracks, (R, G, B): sixteen that are easy to tell apart; a track has colour id % 16
TRACK_PALETTE = ((230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200), (245, 130, 48), (145, 30, 180), (70, 240, 240), (240, 50, 230),
                 (210, 245, 60), (250, 190, 212), (0, 128, 128), (220, 190, 255), (170, 110, 40), (255, 250, 200), (128, 0, 0), (170, 255, 195))
DRAW_MAX_HALF, DRAW_MAX_PALETTE = 3, 256


def _draw(name, fmt_code, d_pixels, pixels_bytes, d_images, d_dets, d_counts, n, cap, d_first, d_status, half, colour, d_keys, key_stride,
          d_palette, palette_n, stream):
    if d_keys is None:
        colour, key_stride, d_palette, palette_n = _colour_code(colour), 0, None, 0
    else:
        colour = 0
    _call(name, n, d_pixels, pixels_bytes, fmt_code, d_images, d_dets, d_counts, n, cap, int(half), colour, d_keys, key_stride, d_palette,
          palette_n, d_first, d_status, stream)


def draw_records_device(d_pixels, pixels_bytes, fmt, d_images, d_dets, d_counts, n, cap, d_first, d_status, half=1, colour=0xFF0000, d_keys=None,
                        key_stride=4, d_palette=None, palette_n=0, stream=None):
    """The outlines of the records of a batch of packed pictures drawn IN PLACE (yf_images_draw_records_device): d_images IMAGE_DTYPE[n],
    d_dets yf_det[n][cap], d_counts int32[n]; d_pixels is written.  half 0..3: 0 the one-pixel outline, 1 the script's thickness 2.
    d_keys None: every record in `colour`, 0x00RRGGBB or (R, G, B).  d_keys given: the record in slot s of frame f in
    d_palette[key % palette_n], key the uint32 at d_keys + (f * cap + s) * key_stride (the d_info of a tracker: stride 16), d_palette
    uint32 0x00RRGGBB [palette_n] on the device, and `colour` is not used.  Where records overlap the highest slot shows.  d_first
    int32[n + 1] and d_status int32[n] (1: the picture's descriptor is invalid, the picture untouched) are written.  With keys the
    pictures of different frames must not share bytes.  The definition: csrc/yf_images_draw.h, ptq.draw_rectangles_u8."""
    _draw("draw_records_device", _packed_code(fmt, "draw_records_device"), d_pixels, pixels_bytes, d_images, d_dets, d_counts, n, cap, d_first,
          d_status, half, colour, d_keys, key_stride, d_palette, palette_n, stream)


def draw_records_yuv_device(d_pixels, pixels_bytes, fmt, d_images, d_dets, d_counts, n, cap, d_first, d_status, half=1, colour=0x515AF0,
                            d_keys=None, key_stride=4, d_palette=None, palette_n=0, stream=None):
    """`draw_records_device` for NV12 / NV21 surfaces, drawn where they lie (yf_images_draw_records_yuv_device): d_images
    YUV_IMAGE_DTYPE[n]; colours 0x00YYUUVV or (Y, U, V).  A chroma pair is written when one of its four luma pixels is drawn.
    ptq.draw_rectangles_yuv420sp."""
    _draw("draw_records_yuv_device", _yuv_code(fmt), d_pixels, pixels_bytes, d_images, d_dets, d_counts, n, cap, d_first, d_status, half,
          colour, d_keys, key_stride, d_palette, palette_n, stream)


def detect_drawn(network, images, half=1, colour=(255, 0, 0), fmt="bgr", cap=None, iou_threshold=0.4, size=56, dtype="int8", tile=None,
                 stride=None, device=None, tracker=None, steps=None, layout="time", palette=None, fit="stretch", pad=114, interp="linear",
                 reid=None):
    """`detect` (with `tile`: `detect_tiled`, whose `tile` and `stride` these are), and the outline of every kept box drawn into its picture
    on the GPU, on the same stream, in the pixels that are already there -- the last line of the reference's scripts,
    cv2.rectangle(img, (x1, y1), (x2, y2), (0, 0, 255), 2), which the defaults reproduce: `colour` (R, G, B) whatever the byte order of
    `fmt` (for NV12 / NV21 surfaces (Y, U, V)), red; `half` = 1, the band of three pixels that thickness 2 is read to draw (half 0..3:
    csrc/yf_images_draw.h; the reading of OpenCV's thickness 2 is not pinned against a real cv2).  fmt, cap, iou_threshold, size, dtype,
    device, fit, pad as in `detect`.
    With `tracker` (a `Tracker`; then `images` are its next `steps` frames in `layout`, as `detect_tracked` takes them; steps=None: as
    many as the images make; iou_threshold must not be None and the tracker's device is used) the tracker is updated with the kept boxes
    and the REPORTED TRACKS are drawn, held-over ones included, each in palette[id % len(palette)]: a face keeps its colour over the
    frames.  `palette`: up to 256 (R, G, B) -- (Y, U, V) -- triples; None: `TRACK_PALETTE`.  Where outlines overlap, the later record
    (the higher track id) shows.  `reid` (with a tracker): as in `detect_tracked`; the descriptors are taken from the pictures before
    anything is drawn into them, and the colours follow the rewritten ids.
    Returns (pictures, boxes) as `detect_redacted` does: the pictures in the caller's shapes, new arrays, and `detect`'s boxes; with a
    tracker (pictures, tracks), `detect_tracked`'s tuples."""
    half = int(half)
    if not 0 <= half <= DRAW_MAX_HALF:
        raise ValueError(f"half {half!r}: 0 to {DRAW_MAX_HALF}")
    colour_code = _colour_code(colour)
    n = len(images)
    if tracker is not None:
        steps = _tracker_steps(tracker, n, steps, layout, iou_threshold)
        table = [_colour_code(c) for c in (TRACK_PALETTE if palette is None else palette)]
        if not 1 <= len(table) <= DRAW_MAX_PALETTE:
            raise ValueError(f"palette: 1 to {DRAW_MAX_PALETTE} colours")
        device = tracker.device.index
        _check_reid(reid, tracker)
    elif reid is not None:
        raise ValueError("reid: only with a tracker")
    if n == 0:
        return [], []
    import torch
    yuv = is_yuv(fmt)
    if tile is not None:
        _packed_code(fmt, "detect_drawn(tile=...)")
    b = _stage(network, images, fmt, cap, device, iou_threshold, size, dtype, tile, stride, True, out_cap=cap, fit=fit, pad=pad, interp=interp)
    d_first = torch.empty(n + 1, dtype=torch.int32, device=b.device)
    d_status = torch.empty(n, dtype=torch.int32, device=b.device)      # the drawing's own: the staging's status does not raise here
    draw = draw_records_yuv_device if yuv else draw_records_device
    s = b.stream.cuda_stream
    if tracker is None:
        draw(b.d_px.data_ptr(), b.nbytes, fmt, b.d_pictures.data_ptr(), b.d_dets.data_ptr(), b.d_counts.data_ptr(), n, b.cap,
             d_first.data_ptr(), d_status.data_ptr(), half=half, colour=colour_code, stream=s)
    else:
        d_out, d_info, d_out_counts, _ = tracker.update(b.d_dets, b.d_counts, steps, layout, cap=b.cap, stream=s)
        _reid_after(reid, tracker, b, fmt, d_out, d_info, d_out_counts, steps, layout)
        d_palette = torch.tensor(table, dtype=torch.int32).to(b.device)
        # the keys are the id fields of the info rows, as they lie: TRACK_INFO_DTYPE's first field, one row per output slot
        draw(b.d_px.data_ptr(), b.nbytes, fmt, b.d_pictures.data_ptr(), d_out.data_ptr(), d_out_counts.data_ptr(), n, d_out.shape[1],
             d_first.data_ptr(), d_status.data_ptr(), half=half, d_keys=d_info.data_ptr(), key_stride=TRACK_INFO_DTYPE.itemsize,
             d_palette=d_palette.data_ptr(), palette_n=len(table), stream=s)
    b.stream.synchronize()
    b.check_totals("detect_drawn")
    bad = np.nonzero(d_status.cpu().numpy())[0]
    if bad.size:
        raise ImagesError(f"detect_drawn: the descriptor of image {int(bad[0])} is invalid")
    pictures = _pictures_back(b, fmt)
    if tracker is None:
        return pictures, b.boxes(np.diff(d_first.cpu().numpy()))
    return pictures, _track_tuples(d_out, d_info, d_out_counts, n)


def detect_tiled(network, images, tile, stride=None, whole=True, fmt="bgr", out_cap=1200, device=None, iou_threshold=0.4, size=56, dtype="int8",
                 fit="stretch", pad=114, interp="linear"):
    """`detect` for pictures larger than the faces in them: every image is cut into tiles (`plan_tiles`: `tile`, `stride` an int or (y, x),
    stride=None no overlap; `whole` adds the whole image as a tile of its own), every tile is one frame of the network at `size` and `dtype`
    (as in `detect`), and the tiles' records are merged per image on the GPU, translated to the image's own pixels (`gather_tiles_device`)
    and suppressed across the tile borders, where overlapping tiles report one face twice (`nms_wide_device`, in place) -- all on one
    stream.  Returns one int32 [k, 4] array (x1, y1, x2, y2) per image: with iou_threshold=None the merged records in tile order, each
    tile's in decode order; with a float the kept ones in keep order.  out_cap: the merged records an image can hold (at most 1200); an
    image with more raises ImagesError naming the image and its total.  fit="letterbox" (and pad): every tile, and the whole-image tile, keeps
    its aspect in its frame, as in `detect`; a square tile is the same frame either way."""
    _packed_code(fmt, "detect_tiled")
    n = len(images)
    if n == 0:
        return []
    b = _stage(network, images, fmt, None, device, iou_threshold, size, dtype, tile, stride, whole, out_cap, fit=fit, pad=pad, interp=interp)
    b.stream.synchronize()
    b.check_totals("detect_tiled")
    return b.boxes(np.minimum(b.d_counts.cpu().numpy(), b.cap))


def detect(network, images, fmt="bgr", cap=None, device=None, iou_threshold=None, size=56, dtype="int8", fit="stretch", pad=114, interp="linear"):
    """Boxes per image, in that image's own pixels: a list of int32 [k, 4] arrays (x1, y1, x2, y2), one per image -- what
    tflite_prediction.py:29-61 computes for each photo, for the whole batch in one ragged launch sequence.  `images`: uint8 [H, W, C] arrays
    of any sizes (cv2.imread gives BGR: fmt="bgr"); `network`: an initialised Network.  iou_threshold=None returns every record above the
    confidence threshold in decode order; a float (yoloface_test.py uses 0.4) suppresses them in place on the same stream (nms_device) and
    returns the kept boxes in keep order, highest confidence first.  size: the side of the network's frames, 56 (7x7 heads) or 160 (20x20
    heads, which find smaller faces; suppression through nms_wide_device); cap=None holds every candidate: 147 / 1200.
    dtype: "int8" (the quantised network) or "fp16" -- the fp16 network, which makes this h5_predition.py:29-73 for the batch: fp16 frames
    of pixel / 255., float32 logits, the float32 decode (`run_decode_f16_ragged_device`).  Call `network.fp16_init()` first, as for
    `fp16_run_device`: detect does not do it.  The fp16 network exists at 56 only.
    fmt="nv12" / "nv21": `images` are surfaces as `pack_yuv_images` takes them; the sequence is the YUV prepare, the network's device run
    and the ragged decode of that size and dtype, on one stream, and the boxes are in the Y plane's pixels -- those of
    cv2.cvtColor(yuv, cv2.COLOR_YUV2BGR_NV12) under fmt="bgr".
    fit="stretch": every picture is resized onto the whole frame, as the reference does.  fit="letterbox": its aspect is kept, the rest
    of the frame is the grey `pad` (0..255; the trainers' 114), and the boxes are mapped back through the same rectangle
    (`run_decode_fit_ragged_device`; the definition: csrc/yf_images_fit.h, `ptq.letterbox_u8`) -- what a model trained by a letterboxing
    trainer expects.  The shipped model was trained on stretched pictures; what letterboxing does to its accuracy has not been measured
    (`evaluate` scores either on labelled pictures).  Any other `fit` raises ValueError.
    interp="linear": the resize is cv2.resize's INTER_LINEAR, as the reference's.  interp="area": every source pixel of the picture is
    averaged into its frame (`prepare_area_*`, then the network and the decode of the fit; the definition: csrc/yf_images_area.h,
    `ptq.resize_area_u8`), with either fit, any fmt, size and dtype.  The shipped model was trained on linearly resized pictures; what
    the filter does to its accuracy has not been measured.  Any other `interp` raises ValueError."""
    _check_frames(size, dtype)                          # before the empty batch is returned, and before torch, the network or the library
    if fit not in FITS:
        raise ValueError(FIT_WHAT.format(fit))
    if interp not in INTERPS:
        raise ValueError(INTERP_WHAT.format(interp))
    if len(images) == 0:
        return []
    b = _stage(network, images, fmt, cap, device, iou_threshold, size, dtype, fit=fit, pad=pad, interp=interp)
    b.stream.synchronize()
    return b.boxes(np.minimum(b.d_counts.cpu().numpy(), b.cap))
