"""What the tests of the face chips share (test_crops_*): the seeded pictures and the designed records, the pictures in each packed format,
the host build's prototypes, and the expected chips, info rows and prefix of a batch -- `ptq.crop_region` and `ptq.crop_resize_u8`, the
plain-Python statement of csrc/yf_images_crop.h, computed once per (picture, region, size) and shared by every format and byte order.

The designed records, per picture of W x H: a box well inside, the whole picture, a 1 x 1 box, boxes overhanging each of the four sides, a
box overhanging a corner, a box wholly outside, x1 > x2, y1 > y2, and INT32_MIN / INT32_MAX edges.  The batch: one frame per picture with
those 13 records, then a frame with count 0, a frame whose count is above cap (all cap records exist) and a frame with a negative count."""
import ctypes
import functools
import importlib

import numpy as np

from images_support import host_lib

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
PICTURES = [(37, 53), (64, 48), (1, 1), (410, 362)]             # (W, H)
CAP = 15
FRAME_PICTURE = [0, 1, 2, 3, 1, 0, 3]                           # the picture of each frame of the designed batch
OUTS = [(16, 16), (112, 112), (32, 48)]                         # (out_h, out_w)
GRID = [(m, s) for m in (0, 250) for s in (False, True)]        # (margin_permille, square)
ORDER_CODE = {"rgb": 1, "bgr": 0}


def _mod(name):
    return importlib.import_module("stm32h7-yolo_amd." + name)


DET = _mod("binding").DET_DTYPE
CHIP = _mod("images").CHIP_DTYPE


@functools.lru_cache(maxsize=None)
def picture(k):
    """the seeded picture k, uint8 [H, W, 3] in RGB order, read-only"""
    w, h = PICTURES[k]
    img = np.random.default_rng(4200 + k).integers(0, 256, (h, w, 3), dtype=np.uint8)
    img.setflags(write=False)
    return img


def in_format(rgb, fmt):
    """the RGB picture as format code `fmt` stores it (0 BGR, 1 RGB, 2 BGRA, 3 RGBA; the alpha byte is seeded noise)"""
    img = rgb[..., ::-1] if fmt in (0, 2) else rgb
    if fmt in (2, 3):
        alpha = np.random.default_rng(77).integers(0, 256, rgb.shape[:2] + (1,), dtype=np.uint8)
        img = np.concatenate([img, alpha], axis=2)
    return np.ascontiguousarray(img)


def designed_boxes(w, h):
    return [
        (w // 4, h // 4, 3 * w // 4, 3 * h // 4),               # well inside
        (0, 0, w - 1, h - 1),                                   # the whole picture
        (w // 2, h // 2, w // 2, h // 2),                       # 1 x 1
        (-w // 3 - 2, h // 4, w // 2, h // 2),                  # overhangs the left side
        (w // 2, h // 4, w + 5, h // 2),                        # ... the right
        (w // 4, -7, w // 2, h // 2),                           # ... the top
        (w // 4, h // 2, w // 2, h + 9),                        # ... the bottom
        (-5, -6, w // 3, h // 3),                               # a corner
        (w + 3, h + 3, w + 10, h + 12),                         # wholly outside
        (w // 2, 0, w // 2 - 1, h - 1),                         # x1 > x2
        (0, h // 2, w - 1, h // 2 - 2),                         # y1 > y2
        (I32_MIN, I32_MIN, I32_MAX, I32_MAX),
        (I32_MIN, h // 4, w // 2, I32_MAX),
    ]


@functools.lru_cache(maxsize=None)
def designed():
    """-> (dets DET [7, CAP], counts int32 [7]); slots that hold no record are 0xA5 bytes"""
    n = len(FRAME_PICTURE)
    dets = np.frombuffer(bytes([0xA5]) * (n * CAP * 28), DET).reshape(n, CAP).copy()
    counts = np.zeros(n, np.int32)
    rng = np.random.default_rng(4300)
    for f, k in enumerate(FRAME_PICTURE):
        w, h = PICTURES[k]
        boxes = designed_boxes(w, h)
        while len(boxes) < CAP:                                 # seeded boxes about the picture fill the frame whose count exceeds cap
            x1, y1 = int(rng.integers(-4, w)), int(rng.integers(-4, h))
            boxes.append((x1, y1, x1 + int(rng.integers(0, w + 4)), y1 + int(rng.integers(0, h + 4))))
        m = {4: 0, 5: CAP + 84, 6: -3}.get(f, 13)
        counts[f] = m
        for s in range(CAP if f == 5 else max(m, 0)):
            dets[f, s] = (f, s % 3, 1, 2, 5, 0.75 + s / 64, *boxes[s])
    dets.setflags(write=False)
    counts.setflags(write=False)
    return dets, counts


def clamp(count, cap):
    return min(max(int(count), 0), cap)


@functools.lru_cache(maxsize=4096)
def _chip_rgb(key, region, out_h, out_w):
    """the chip of `region` = (x0, y0, w, h) of the picture registered under `key`, RGB order; read-only"""
    x0, y0, w, h = region
    chip = _mod("ptq").resize_linear_u8(_PICTURES[key][y0:y0 + h, x0:x0 + w], out_w, out_h)
    chip.setflags(write=False)
    return chip


_PICTURES = {}


def register(key, rgb):
    """make an RGB picture known to the expected-chip cache under a hashable key"""
    _PICTURES[key] = rgb
    return key


def expected(dets, counts, cap, keys, out_h, out_w, margin, square, order, chips_cap=None, invalid=()):
    """-> (chips uint8 [total, out_h, out_w, 3], info CHIP [total], first int32 [n + 1]) of a batch whose frame i shows the registered
    picture keys[i]; chips_cap cuts chips and info (not first).  Frames in `invalid` have status 2."""
    ptq = _mod("ptq")
    chips, info, first = [], [], [0]
    for i in range(dets.shape[0]):
        rgb = _PICTURES[keys[i]]
        for s in range(clamp(counts[i], cap)):
            d = dets[i, s]
            region = None if i in invalid else ptq.crop_region((d["x1"], d["y1"], d["x2"], d["y2"]), rgb.shape[1], rgb.shape[0], margin, square)
            if region is None:
                chips.append(np.zeros((out_h, out_w, 3), np.uint8))
                info.append((i, s, 0, 0, 0, 0, 2 if i in invalid else 1))
            else:
                chip = _chip_rgb(keys[i], region, out_h, out_w)
                chips.append(chip if order == "rgb" else chip[..., ::-1])
                info.append((i, s) + region + (0,))
        first.append(len(chips))
    k = len(chips) if chips_cap is None else min(len(chips), chips_cap)
    return (np.stack(chips[:k]) if k else np.zeros((0, out_h, out_w, 3), np.uint8)), np.array(info[:k], CHIP).reshape(-1), np.array(first, np.int32)


@functools.lru_cache(maxsize=None)
def crops_host():
    """libyf_images_host.so with the prototypes of csrc/yf_images_crop.h's host build added"""
    lib = host_lib()
    vp, ci, cl = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    for fn in (lib.yfi_crop_records_host, lib.yfi_crop_records_yuv_host):
        fn.restype = cl
        fn.argtypes = [vp, ctypes.c_uint64, ci, vp, vp, vp, cl, ci, ci, ci, ci, ci, ci, vp, cl, vp, vp]
    lib.yfi_crop_region_host.restype = None
    lib.yfi_crop_region_host.argtypes = [ctypes.c_int32] * 6 + [ci, ci, vp]
    return lib


def host_crop(buf, fmt, desc, dets, counts, cap, out_h, out_w, margin, square, order, chips_cap, nbytes=None):
    """the host build on a batch -> (rc, chips uint8 [chips_cap, ...], info CHIP [chips_cap], first int32 [n + 1]), written into buffers
    filled with 0xA5"""
    lib = crops_host()
    n = dets.shape[0]
    room = max(chips_cap, 1)
    chips = np.full((room, out_h, out_w, 3), 0xA5, np.uint8)
    info = np.frombuffer(bytes([0xA5]) * (room * 28), CHIP).copy()
    first = np.full(n + 1, np.int32(-1515870811), np.int32)           # 0xA5A5A5A5
    dets, counts, desc = np.ascontiguousarray(dets), np.ascontiguousarray(counts), np.ascontiguousarray(desc)
    fn = lib.yfi_crop_records_yuv_host if fmt in (4, 5) else lib.yfi_crop_records_host
    rc = fn(buf.ctypes.data, buf.nbytes if nbytes is None else nbytes, fmt, desc.ctypes.data, dets.ctypes.data, counts.ctypes.data, n, cap,
            out_h, out_w, ORDER_CODE[order], margin, int(square), chips.ctypes.data, chips_cap, first.ctypes.data, info.ctypes.data)
    return rc, chips, info, first


def designed_batch(fmt):
    """the designed batch in packed format `fmt` -> (buf, desc, dets, counts, keys)"""
    images = _mod("images")
    dets, counts = designed()
    buf, desc = images.pack_images([in_format(picture(k), fmt) for k in FRAME_PICTURE], fmt)
    keys = [register(("designed", k), picture(k)) for k in FRAME_PICTURE]
    return buf, desc, dets, counts, keys
