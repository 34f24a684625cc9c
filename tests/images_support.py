"""What the tests of libyf_images share (test_images_*, test_nms_*, test_boxes160_*): the restatement of the reference's suppression and the
check of a suppressed batch against it, the reference's image sizes and the real images at those sizes, the expected frame of an image, a
ragged batch on the device at either frame size, the host build of the library's arithmetic, the seeded synthetic heads, and the fixtures.

`nms_restated` is the project's statement of YoloFaceDetector.non_max_suppression (yoloface/tensorflow/yoloface_test.py:165-190): a literal
copy with one change, a stable sort (ties later record first).  `nms_reference_literal` keeps the reference's default argsort."""
import ctypes
import importlib
import os

import numpy as np
import pytest

from conftest import ROOT
from host_libs import host_library

PKG = os.path.join(ROOT, "stm32h7-yolo_amd")

# the reference's 27 sample images (yoloface/small_dataset, sorted by name), (width, height)
REF_SIZES = [(410, 362), (389, 450), (410, 356), (299, 410), (331, 410), (327, 410), (410, 391), (410, 330), (301, 410), (410, 450),
             (410, 283), (410, 281), (274, 410), (282, 410), (406, 450), (410, 312), (327, 410), (410, 273), (410, 295), (410, 297),
             (305, 409), (410, 344), (306, 450), (278, 410), (410, 301), (253, 409), (410, 295)]
FMT_CH = {0: 3, 1: 3, 2: 4, 3: 4}
BGR = {0: True, 1: False, 2: True, 3: False}


# ---- fixtures (imported into the test modules by name) ----
@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def images():
    return importlib.import_module("stm32h7-yolo_amd.images")


@pytest.fixture(scope="module", name="images")
def images_after_network(network):
    """`images` of the GPU tests: the network (and with it torch's HIP context) is up before libyf_images.so is loaded"""
    return importlib.import_module("stm32h7-yolo_amd.images")


@pytest.fixture(scope="module")
def ptq():
    return importlib.import_module("stm32h7-yolo_amd.ptq")


@pytest.fixture(scope="module")
def host():
    return host_lib()


# ---- the host build of the library's arithmetic ----
def host_lib(build=True):
    """libyf_images_host.so (csrc/yf_images_host.c) with every prototype set; build=False: the file as it is, without make"""
    lib = host_library("libyf_images_host.so") if build else ctypes.CDLL(os.path.join(PKG, "lib", "libyf_images_host.so"))
    lib.yfi_resize_host.restype = ctypes.c_int
    lib.yfi_resize_host.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_long, ctypes.c_int, ctypes.c_int,
                                    ctypes.c_void_p]
    lib.yfi_tap_host.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.yfi_image_ok_host.restype = ctypes.c_int
    lib.yfi_image_ok_host.argtypes = [ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_uint64]
    lib.yfi_nms_pairs_host.restype = None
    lib.yfi_nms_pairs_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]
    for key in (lib.yfi_nms_key_host, lib.yfi_nms_key_wide_host):
        key.restype = ctypes.c_uint64
        key.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    lib.yfi_decode160_host.restype = ctypes.c_int
    lib.yfi_decode160_host.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_float, ctypes.c_float, ctypes.c_void_p, ctypes.c_int]
    lib.yfi_decode160_q_threshold_host.restype = ctypes.c_int
    return lib


def last_error(lib):
    """the text libyf_images.so left for the call that has just failed"""
    return (lib.yf_images_last_error_text() or b"").decode()


# ---- the suppression, restated ----
def _boxes(recs):
    """records (DET_DTYPE rows or tuples (frame, anchor, row, col, q_conf, conf, x1, y1, x2, y2)) -> the reference's boxes list"""
    return [[int(r[6]), int(r[7]), int(r[8]), int(r[9]), float(r[5])] for r in recs]


def nms_reference_literal(boxes, iou_threshold):
    """yoloface_test.py:165-190 as written (numpy's default argsort); returns `keep`, the indices boxes[keep] is taken with"""
    if len(boxes) == 0:
        return []
    boxes = np.array(boxes)
    x1 = boxes[:, 0]
    y1 = boxes[:, 1]
    x2 = boxes[:, 2]
    y2 = boxes[:, 3]
    conf = boxes[:, 4]
    area = (x2 - x1 + 1) * (y2 - y1 + 1)
    order = conf.argsort()[::-1]
    keep = []
    while order.size > 0:
        i = order[0]
        keep.append(i)
        xx1 = np.maximum(x1[i], x1[order[1:]])
        yy1 = np.maximum(y1[i], y1[order[1:]])
        xx2 = np.minimum(x2[i], x2[order[1:]])
        yy2 = np.minimum(y2[i], y2[order[1:]])
        w = np.maximum(0.0, xx2 - xx1 + 1)
        h = np.maximum(0.0, yy2 - yy1 + 1)
        intersection = w * h
        union = area[i] + area[order[1:]] - intersection
        with np.errstate(divide="ignore", invalid="ignore"):
            iou = intersection / union
        inds = np.where(iou <= iou_threshold)[0]
        order = order[inds + 1]
    return [int(k) for k in keep]


def nms_restated(boxes, iou_threshold):
    """the same with the pinned order: np.argsort(conf, kind="stable")[::-1] (descending conf, ties later record first)"""
    if len(boxes) == 0:
        return []
    boxes = np.array(boxes)
    x1 = boxes[:, 0]
    y1 = boxes[:, 1]
    x2 = boxes[:, 2]
    y2 = boxes[:, 3]
    conf = boxes[:, 4]
    area = (x2 - x1 + 1) * (y2 - y1 + 1)
    order = np.argsort(conf, kind="stable")[::-1]
    keep = []
    while order.size > 0:
        i = order[0]
        keep.append(i)
        xx1 = np.maximum(x1[i], x1[order[1:]])
        yy1 = np.maximum(y1[i], y1[order[1:]])
        xx2 = np.minimum(x2[i], x2[order[1:]])
        yy2 = np.minimum(y2[i], y2[order[1:]])
        w = np.maximum(0.0, xx2 - xx1 + 1)
        h = np.maximum(0.0, yy2 - yy1 + 1)
        intersection = w * h
        union = area[i] + area[order[1:]] - intersection
        with np.errstate(divide="ignore", invalid="ignore"):
            iou = intersection / union
        inds = np.where(iou <= iou_threshold)[0]
        order = order[inds + 1]
    return [int(k) for k in keep]


def suppress(recs, iou_threshold):
    """the kept records of one frame, in keep order"""
    return [recs[k] for k in nms_restated(_boxes(recs), iou_threshold)]


def expect_kept(rows, count, cap, thr):
    """the kept rows of one frame: the restatement over its first min(max(count, 0), cap) records"""
    m = min(max(int(count), 0), cap)
    r = rows[:m]
    boxes = np.stack([r["x1"], r["y1"], r["x2"], r["y2"], r["conf"]], axis=1).astype(np.float64)      # what np.array(boxes) makes
    return r[nms_restated(boxes, thr)]


# ---- device buffers and their host views ----
def sentinels(torch, n, cap):
    """d_dets, d_counts that show what was written: every record byte 0xA5, every count -7"""
    return torch.full((max(n, 1), cap, 28), 0xA5, dtype=torch.uint8, device="cuda"), torch.full((max(n, 1),), -7, dtype=torch.int32, device="cuda")


def to_host(yf, d_dets, d_counts, cap):
    """device records and counts -> DET_DTYPE [n, cap], int32 [n], after a synchronize"""
    import torch
    torch.cuda.synchronize()
    return d_dets.cpu().numpy().view(yf.DET_DTYPE).reshape(-1, cap), d_counts.cpu().numpy()


def tuples(rows):
    return [tuple(v.item() for v in r) for r in rows]


def check_nms(yf, dets_in, counts_in, d_out, d_oc, cap, thr, frames=None):
    """every frame's output (written into `sentinels`) equals the restatement, byte for byte and in keep order, and slots beyond the kept
    count keep their sentinel; returns the number of records the suppression removed"""
    out, oc = to_host(yf, d_out, d_oc, cap)
    raw = out.view(np.uint8).reshape(out.shape[0], cap, 28)
    lost = 0
    for f in (range(dets_in.shape[0]) if frames is None else frames):
        want = expect_kept(dets_in[f], counts_in[f], cap, thr)
        assert oc[f] == want.shape[0], (f, thr, oc[f], want.shape[0])
        assert out[f, :want.shape[0]].tobytes() == want.tobytes(), (f, thr)
        assert (raw[f, want.shape[0]:] == 0xA5).all(), (f, thr)
        lost += min(max(int(counts_in[f]), 0), cap) - want.shape[0]
    return lost


# ---- images, frames and batches ----
def expect_frame(ptq, img, fmt, out):
    """the restatement: RGB order, cv2.resize, minus 128, int8"""
    rgb = img[..., :3][..., ::-1] if BGR[fmt] else img[..., :3]
    return (ptq.resize_linear_u8(np.ascontiguousarray(rgb), out, out).astype(np.int16) - 128).astype(np.int8)


def real_images(ptq):
    """the 27 real frames (+128, RGB) upscaled by the restatement to the reference sizes, stored as BGR as cv2.imread gives them"""
    real = np.fromfile(os.path.join(ROOT, "tests", "golden", "real_frames_56.bin"), np.int8).reshape(-1, 56, 56, 3)
    rgb56 = (real.astype(np.int16) + 128).astype(np.uint8)
    return [np.ascontiguousarray(ptq.resize_linear_u8(rgb56[i], w, h)[..., ::-1]) for i, (w, h) in enumerate(REF_SIZES)]


class Batch:
    """a packed ragged batch on the device with its workspaces, for frames of `out` x `out` (56: 7x7 heads, 160: 20x20 heads).  cap=None
    holds every candidate.  Frames are filled with 77, status with -7, records and counts with `sentinels`."""

    def __init__(self, torch, images, imgs, fmt, out=56, cap=None, desc=None, buf=None):
        if desc is None:
            buf, desc = images.pack_images(imgs, fmt)
        grid = out // 8
        self.n, self.buf, self.desc, self.fmt, self.out, self.cap = desc.shape[0], buf, desc, fmt, out, 3 * grid * grid if cap is None else cap
        self.d_px = torch.from_numpy(buf).cuda()
        self.d_desc = torch.from_numpy(desc.view(np.uint8).copy()).cuda()
        n = max(self.n, 1)
        self.d_frames = torch.full((n, out, out, 3), 77, dtype=torch.int8, device="cuda")
        self.d_heads = torch.zeros((n, grid, grid, 18), dtype=torch.int8, device="cuda")
        self.d_dets, self.d_counts = sentinels(torch, n, self.cap)
        self.d_status = torch.full((n,), -7, dtype=torch.int32, device="cuda")

    def prepare(self, images):
        images.prepare_ragged_device(self.d_px.data_ptr(), self.buf.nbytes, self.fmt, self.d_desc.data_ptr(), self.n, self.out,
                                     self.d_frames.data_ptr(), self.d_status.data_ptr())

    def run_decode(self, images, network):
        run = images.run_decode_ragged_device if self.out == 56 else images.run_decode160_ragged_device
        run(network, self.d_px.data_ptr(), self.buf.nbytes, self.fmt, self.d_desc.data_ptr(), self.n, self.d_frames.data_ptr(),
            self.d_heads.data_ptr(), self.d_dets.data_ptr(), self.d_counts.data_ptr(), self.cap, self.d_status.data_ptr())

    def records(self, yf):
        dets, counts = to_host(yf, self.d_dets, self.d_counts, self.cap)
        return [tuples(dets[i, :min(int(counts[i]), self.cap)]) for i in range(self.n)], counts


# ---- seeded heads ----
def synthetic_heads(rng, n):
    """seeded heads: random bytes (about half the candidates fire: q_conf >= -9), every third frame sparse, every 64th frame all 147
    candidates at one shared q_conf"""
    heads = rng.integers(-128, 128, (n, 7, 7, 18), dtype=np.int16)
    heads[1::3, ..., 4::6] = rng.integers(-128, 0, heads[1::3, ..., 4::6].shape)
    for f in range(0, n, 64):
        heads[f, ..., 4::6] = 96 + (f // 64) % 32
    return heads.astype(np.int8)


def synthetic_heads160(rng, n):
    """seeded 20x20 heads: random bytes (about half the 1200 candidates fire), every third frame sparse, every 64th frame all 1200
    candidates at one shared q_conf"""
    heads = rng.integers(-128, 128, (n, 20, 20, 18), dtype=np.int16)
    sparse = heads[1::3, ..., 4::6]
    heads[1::3, ..., 4::6] = np.where(rng.random(sparse.shape) < 0.01, sparse, rng.integers(-128, -20, sparse.shape))
    for f in range(0, n, 64):
        heads[f, ..., 4::6] = 96 + (f // 64) % 32
    return heads.astype(np.int8)
