"""What the tests of the area-averaged frames share (test_area_host, test_area_gpu): the prototypes of the host build's area functions
(csrc/yf_images_area.h through csrc/yf_images_host.c), the expected frame of a picture (`ptq.resize_area_u8` / `ptq.letterbox_u8(...,
interp="area")` under the minus 128 or the halves of the frame's element), each computed once per (picture, size, fit, pad), and the
pictures the tests build: a picture in a buffer of exactly its extent, surfaces with odd pitches."""
import ctypes
import functools
import importlib

import numpy as np

from fit_support import YfImage, YfImageYuv, fit_host, halves

STRETCH, LETTERBOX = 0, 1


def _ptq():
    return importlib.import_module("stm32h7-yolo_amd.ptq")


@functools.lru_cache(maxsize=None)
def area_host():
    """libyf_images_host.so with the prototypes of the area functions added"""
    lib = fit_host()
    vp, ci, i32, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int32, ctypes.c_uint64
    lib.yfi_area_weight_host.restype = None
    lib.yfi_area_weight_host.argtypes = [i32, i32, i32, i32, vp]
    lib.yfi_area_bands_host.restype = ci
    lib.yfi_area_bands_host.argtypes = [ctypes.c_long, ci]
    lib.yfi_prepare_area_host.restype = ci
    lib.yfi_prepare_area_host.argtypes = [vp, u64, ci, vp, ci, ci, ci, ci, vp]
    lib.yfi_prepare_area_yuv_host.restype = ci
    lib.yfi_prepare_area_yuv_host.argtypes = [vp, u64, vp, ci, ci, ci, ci, ci, vp]
    lib.yfi_area_check_host.restype = ci
    lib.yfi_area_check_host.argtypes = [ci, ci, vp, ci, vp, ctypes.c_long, ci, ci, ci, vp, vp, vp, ci]
    return lib


def host_weight(d, s, n_in, n_out):
    """(a(d, s), first source of d, last source of d) as the host build computes them"""
    out = np.zeros(3, np.int32)
    area_host().yfi_area_weight_host(d, s, n_in, n_out, out.ctypes.data)
    return tuple(int(v) for v in out)


@functools.lru_cache(maxsize=4096)
def _area_cached(shape, data, S, fit, pad):
    rgb = np.frombuffer(data, np.uint8).reshape(shape)
    out = _ptq().letterbox_u8(rgb, S, pad, interp="area") if fit == LETTERBOX else _ptq().resize_area_u8(rgb, S, S)
    out.setflags(write=False)
    return out


def expect_u8(rgb, S, fit=STRETCH, pad=114):
    """the restatement's bytes of an RGB picture, computed once per (picture, S, fit, pad): uint8 [S, S, 3]"""
    return _area_cached(rgb.shape, rgb.tobytes(), S, fit, pad if fit == LETTERBOX else 0)


def as_frame(u8, f16=False):
    return halves()[u8] if f16 else (u8.astype(np.int16) - 128).astype(np.int8)


def expect_frame_area(rgb, S, fit=STRETCH, pad=114, f16=False):
    return as_frame(expect_u8(rgb, S, fit, pad), f16)


def exact_buffer(img, row_stride=None):
    """a picture [h, w, C] stored with `row_stride` (None: packed rows; the gap bytes are 0x5B) in a buffer of exactly its extent"""
    h, w, C = img.shape
    rs = w * C if row_stride is None else row_stride
    buf = np.full((h - 1) * rs + w * C, 0x5B, np.uint8)
    np.lib.stride_tricks.as_strided(buf, shape=(h, w * C), strides=(rs, 1))[:] = img.reshape(h, w * C)
    return buf, rs


def host_area_packed(img, fmt, S, fit=STRETCH, pad=114, f16=False, row_stride=None):
    """yfi_prepare_area_host on one picture in a buffer of exactly its extent -> (status, frame)"""
    buf, rs = exact_buffer(img, row_stride)
    frame = np.full((S, S, 3), 0x1111 if f16 else 17, np.uint16 if f16 else np.int8)
    im = YfImage(0, img.shape[0], img.shape[1], rs)
    st = area_host().yfi_prepare_area_host(buf.ctypes.data, buf.nbytes, fmt, ctypes.byref(im), S, fit, pad, int(f16), frame.ctypes.data)
    return st, frame


def host_area_yuv(buf, d, v_first, S, fit=STRETCH, pad=114, f16=False):
    """yfi_prepare_area_yuv_host on one descriptor (a YUV_IMAGE_DTYPE record) of `buf` -> (status, frame)"""
    frame = np.full((S, S, 3), 0x1111 if f16 else 17, np.uint16 if f16 else np.int8)
    im = YfImageYuv(int(d["offset_y"]), int(d["offset_uv"]), int(d["height"]), int(d["width"]), int(d["stride_y"]), int(d["stride_uv"]))
    st = area_host().yfi_prepare_area_yuv_host(buf.ctypes.data, buf.nbytes, ctypes.byref(im), int(v_first), S, fit, pad, int(f16),
                                               frame.ctypes.data)
    return st, frame


def host_linear_frame(img, fmt, S):
    """the linear prepare's host frame of a packed picture, int8 [S, S, 3]: yfi_resize_host under the channel order and the minus 128"""
    from images_support import BGR
    h, w, C = img.shape
    src = np.ascontiguousarray(img)
    dst = np.zeros((S, S, C), np.uint8)
    assert area_host().yfi_resize_host(src.ctypes.data, h, w, C, w * C, S, S, dst.ctypes.data) == 0
    rgb = dst[..., :3][..., ::-1] if BGR[fmt] else dst[..., :3]
    return (rgb.astype(np.int16) - 128).astype(np.int8)


def checkerboard(side, shift=0):
    """squares of one pixel, 0 and 255, as an RGB picture [side, side, 3]; shift=1: the same board moved by one pixel"""
    y, x = np.mgrid[0:side, 0:side]
    return np.repeat((((y + x + shift) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)


def lay_out_packed(imgs, image_dtype, slack=5):
    """Packed pictures [h, w, C] -> (buffer uint8, descriptors): the first at offset 1, odd gaps between them, rows `slack` bytes longer
    than their pixels, every byte that is no pixel 0x5B, and the buffer ends with the last picture's last pixel: an allocation of exactly
    the pictures' extent"""
    desc = np.zeros(len(imgs), image_dtype)
    parts, off = [], 1
    for i, img in enumerate(imgs):
        h, w, C = img.shape
        rs = w * C + slack
        desc[i] = (off, h, w, rs)
        parts.append((off, rs, img.reshape(h, w * C)))
        off += (h - 1) * rs + w * C + 3 + 2 * (i % 2)
    last = max(o + (p.shape[0] - 1) * s + p.shape[1] for o, s, p in parts)
    buf = np.full(last, 0x5B, np.uint8)
    for o, s, p in parts:
        np.lib.stride_tricks.as_strided(buf[o:], shape=p.shape, strides=(s, 1))[:] = p
    return buf, desc
