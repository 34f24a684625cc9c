"""What the tests of the NV12 / NV21 path share (test_images_yuv_*): the host build's new prototypes, the shape list, seeded surfaces and the
buffer they are laid out in, the expected frame of a surface (the restated conversion under `images_support.expect_frame`), and the real
images as surfaces.

The yardstick of a frame: `expect_frame(ptq, ptq.yuv420sp_to_rgb_u8(y, uv, v_first)[..., ::-1], BGR, out)` -- the frame of
cv2.cvtColor(yuv, cv2.COLOR_YUV2BGR_NV12) under the BGR path that exists."""
import ctypes
import functools
import importlib

import numpy as np

from images_support import expect_frame, host_lib, real_images

# (h, w): the minimum; taps whose two columns or rows share / do not share a chroma pair; upscaling; the identity size and both sides of
# it; the reference's sizes; the maximum side
SHAPES = [(2, 2), (2, 4), (4, 2), (6, 10), (54, 58), (56, 56), (58, 54), (112, 112), (362, 410), (450, 306), (2, 16384), (16384, 2)]
GAP = 0x5B            # the filler between rows and planes: no value of the clamp pictures, and as a sample it changes a random picture


class YfImageYuv(ctypes.Structure):
    _fields_ = [("offset_y", ctypes.c_uint64), ("offset_uv", ctypes.c_uint64), ("height", ctypes.c_int32), ("width", ctypes.c_int32),
                ("stride_y", ctypes.c_int64), ("stride_uv", ctypes.c_int64)]


@functools.lru_cache(maxsize=None)
def yuv_host_lib():
    """libyf_images_host.so with the prototypes of csrc/yf_images_yuv.h's host build added"""
    lib = host_lib()
    lib.yfi_yuv_rgb_host.restype = None
    lib.yfi_yuv_rgb_host.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p]
    lib.yfi_yuv_image_ok_host.restype = ctypes.c_int
    lib.yfi_yuv_image_ok_host.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                          ctypes.c_uint64]
    lib.yfi_prepare_yuv_host.restype = ctypes.c_int
    lib.yfi_prepare_yuv_host.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_void_p]
    return lib


def _ptq():
    return importlib.import_module("stm32h7-yolo_amd.ptq")


def f16_table():
    out = np.zeros(256, np.uint16)
    yuv_host_lib().yfi_f16_of_u8_host(out.ctypes.data_as(ctypes.c_void_p))
    return out


@functools.lru_cache(maxsize=None)
def surface(k, clamp):
    """the seeded surface of SHAPES[k]: (y [h, w], uv [h / 2, w]), read-only.  clamp: built from Y in {0, 16, 235, 255} and U, V in
    {0, 128, 255} only, so every clamp of the conversion fires"""
    h, w = SHAPES[k]
    rng = np.random.default_rng(1000 + 2 * k + int(clamp))
    if clamp:
        y = rng.choice(np.array([0, 16, 235, 255], np.uint8), (h, w))
        uv = rng.choice(np.array([0, 128, 255], np.uint8), (h // 2, w))
    else:
        y = rng.integers(0, 256, (h, w), dtype=np.uint8)
        uv = rng.integers(0, 256, (h // 2, w), dtype=np.uint8)
    y.setflags(write=False)
    uv.setflags(write=False)
    return y, uv


def all_surfaces():
    """[(shape index, clamp)] in batch order: per shape the random picture, then the clamp picture"""
    return [(k, c) for k in range(len(SHAPES)) for c in (False, True)]


@functools.lru_cache(maxsize=None)
def restated_rgb(k, clamp, v_first, out):
    """uint8 [out, out, 3]: the resized bytes of the converted surface, RGB order.  Computed once, read-only."""
    y, uv = surface(k, clamp)
    ptq = _ptq()
    bgr = np.ascontiguousarray(ptq.yuv420sp_to_rgb_u8(y, uv, v_first)[..., ::-1])
    frame = expect_frame(ptq, bgr, 0, out)
    rgb = (frame.astype(np.int16) + 128).astype(np.uint8)
    rgb.setflags(write=False)
    return rgb


def expected_frame(k, clamp, v_first, out):
    return (restated_rgb(k, clamp, v_first, out).astype(np.int16) - 128).astype(np.int8)


def lay_out(surfaces, tail=0):
    """Surfaces [(y, uv)] -> (buffer uint8, descriptors YUV_IMAGE_DTYPE) with pitches stride_y = w + 3 and stride_uv = w + 6, every second
    surface's UV plane before its Y plane, nothing aligned, and every byte that is no sample equal to GAP.  The last plane ends with the
    buffer (plus `tail` bytes of GAP)."""
    images = importlib.import_module("stm32h7-yolo_amd.images")
    desc = np.zeros(len(surfaces), images.YUV_IMAGE_DTYPE)
    parts, off = [], 1
    for i, (y, uv) in enumerate(surfaces):
        h, w = y.shape
        sy, suv = w + 3, w + 6
        ext_y, ext_uv = (h - 1) * sy + w, (h // 2 - 1) * suv + w
        if i % 2:
            off_uv, off_y = off, off + ext_uv + 5
            off = off_y + ext_y + 3
        else:
            off_y, off_uv = off, off + ext_y + 7
            off = off_uv + ext_uv + 3
        desc[i] = (off_y, off_uv, h, w, sy, suv)
        parts.append((off_y, sy, y))
        parts.append((off_uv, suv, uv))
    last = max(o + (p.shape[0] - 1) * s + p.shape[1] for o, s, p in parts)
    buf = np.full(last + tail, GAP, np.uint8)
    for o, s, p in parts:
        rows, w = p.shape
        np.lib.stride_tricks.as_strided(buf[o:], shape=(rows, w), strides=(s, 1))[:] = p
    return buf, desc


def host_frame(buf, d, v_first, out, f16=False):
    """yfi_prepare_yuv_host on one descriptor (a YUV_IMAGE_DTYPE record) of `buf` -> (status, frame)"""
    lib = yuv_host_lib()
    frame = np.full((out, out, 3), 0x1111 if f16 else 17, np.uint16 if f16 else np.int8)
    im = YfImageYuv(int(d["offset_y"]), int(d["offset_uv"]), int(d["height"]), int(d["width"]), int(d["stride_y"]), int(d["stride_uv"]))
    st = lib.yfi_prepare_yuv_host(buf.ctypes.data, buf.nbytes, ctypes.byref(im), int(v_first), out, int(f16), frame.ctypes.data)
    return st, frame


# ---- real content ----
def bgr_to_nv12(bgr):
    """A float BT.601 limited-range forward conversion with 2x2 chroma averaging: it only generates input (nothing is exact about it).
    uint8 [H, W, 3] BGR with even sides -> (y [H, W], uv [H / 2, W]) as NV12."""
    b, g, r = (bgr[..., c].astype(np.float64) for c in range(3))
    y = 16 + (65.481 * r + 128.553 * g + 24.966 * b) / 255
    u = 128 + (-37.797 * r - 74.203 * g + 112.0 * b) / 255
    v = 128 + (112.0 * r - 93.786 * g - 18.214 * b) / 255
    h, w = y.shape
    u2 = u.reshape(h // 2, 2, w // 2, 2).mean(axis=(1, 3))
    v2 = v.reshape(h // 2, 2, w // 2, 2).mean(axis=(1, 3))
    uv = np.stack([u2, v2], axis=-1).reshape(h // 2, w)
    return np.clip(np.rint(y), 0, 255).astype(np.uint8), np.clip(np.rint(uv), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def real_surfaces():
    """the 27 real images cropped to even sides as NV12 -> (nv12 [(y, uv)], nv21 [(y, vu)], bgr [the restated BGR of those surfaces])"""
    ptq = _ptq()
    nv12, nv21, bgr = [], [], []
    for img in real_images(ptq):
        h, w = img.shape[0] & ~1, img.shape[1] & ~1
        y, uv = bgr_to_nv12(img[:h, :w])
        vu = np.ascontiguousarray(uv.reshape(h // 2, w // 2, 2)[..., ::-1]).reshape(h // 2, w)
        nv12.append((y, uv))
        nv21.append((y, vu))
        bgr.append(np.ascontiguousarray(ptq.yuv420sp_to_rgb_u8(y, uv)[..., ::-1]))
    return nv12, nv21, bgr
