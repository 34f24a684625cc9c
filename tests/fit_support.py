"""What the tests of the letterboxed frames share (test_fit_host, test_fit_gpu): the prototypes of the host build's letterbox functions
(csrc/yf_images_fit.h through csrc/yf_images_host.c), the shapes and seeded pictures, the expected frame of a picture (`ptq.letterbox_u8`
under the channel order and the minus 128 of `images_support.expect_frame`), and the project's own statement, in numpy float32, of the
decode with the letterbox tail -- one IEEE operation per numpy operation, in the order csrc/yf_images_fit.h gives:

    x_scale = float32(W / width), y_scale = float32(H / height)                   (float64 division, rounded once)
    cx = (sx + col) * 8, cy = (sy + row) * 8, bw = ew * anchor_w, bh = eh * anchor_h
    x1 = cx - bw / 2, ...                                                          (the edges in frame pixels)
    x = (x - float32(x0)) * x_scale, y = (y - float32(y0)) * y_scale               (THE change against YF_DECODE_PY)
    int32: truncation, out of range and NaN -> INT32_MIN

with (x0, y0, width, height) = ptq.letterbox_fit(H, W, S).  The reference has no letterbox; the definition is the library's own."""
import ctypes
import functools
import importlib

import numpy as np

from float_support import exp_rounded, to_int32
from images_support import BGR, FMT_CH, host_lib, real_images

DET = np.dtype([("frame", "<i4"), ("anchor", "u1"), ("row", "u1"), ("col", "u1"), ("q_conf", "i1"),
                ("conf", "<f4"), ("x1", "<i4"), ("y1", "<i4"), ("x2", "<i4"), ("y2", "<i4")])
ANCHOR_W, ANCHOR_H = np.float32([9, 12, 22]), np.float32([14, 17, 21])
PADS = (0, 114, 255)
# (h, w): the smallest; one off the square on either side; the thinnest; strips whose short side rounds to 1 or 2 frame pixels
SMALL_SHAPES = [(1, 1), (57, 56), (56, 57), (2, 1), (1, 2), (3, 200), (200, 3)]
# NV12 / NV21: the smallest surface, the thinnest, one off the square
YUV_SHAPES = [(2, 2), (2, 400), (400, 2), (58, 56), (56, 58), (362, 410)]
# mixed aspects for the decodes: landscape, portrait, square, the exact-half case, strips, the extremes
DECODE_SIDES = [(1080, 1920), (1920, 1080), (300, 300), (362, 410), (57, 56), (1, 16384), (16384, 1), (16384, 16384), (3, 200), (56, 56), (1, 1)]


class YfImage(ctypes.Structure):
    _fields_ = [("offset", ctypes.c_uint64), ("height", ctypes.c_int32), ("width", ctypes.c_int32), ("row_stride", ctypes.c_int64)]


class YfImageYuv(ctypes.Structure):
    _fields_ = [("offset_y", ctypes.c_uint64), ("offset_uv", ctypes.c_uint64), ("height", ctypes.c_int32), ("width", ctypes.c_int32),
                ("stride_y", ctypes.c_int64), ("stride_uv", ctypes.c_int64)]


def _ptq():
    return importlib.import_module("stm32h7-yolo_amd.ptq")


@functools.lru_cache(maxsize=None)
def fit_host():
    """libyf_images_host.so with the prototypes of the letterbox functions added"""
    lib = host_lib()
    vp, ci, i32, i64, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64
    lib.yfi_fit_host.restype = None
    lib.yfi_fit_host.argtypes = [i64, i64, i64, vp]
    lib.yfi_prepare_fit_host.restype = ci
    lib.yfi_prepare_fit_host.argtypes = [vp, u64, ci, vp, ci, ci, ci, vp]
    lib.yfi_prepare_fit_yuv_host.restype = ci
    lib.yfi_prepare_fit_yuv_host.argtypes = [vp, u64, vp, ci, ci, ci, ci, vp]
    lib.yfi_decode_fit_host.restype = ci
    lib.yfi_decode_fit_host.argtypes = [vp, i32, i32, i32, i32, ci, vp, ci]
    lib.yfi_decode_f32_fit_host.restype = ci
    lib.yfi_decode_f32_fit_host.argtypes = [vp, i32, i32, i32, i32, vp, ci]
    lib.yfi_decode_f32_host.restype = ci
    lib.yfi_decode_f32_host.argtypes = [vp, i32, ctypes.c_float, ctypes.c_float, vp, ci]
    lib.yfi_fit_check_host.restype = ci
    lib.yfi_fit_check_host.argtypes = [ci, ci, ci, vp, ci, vp, ctypes.c_long, ci, ci, vp, vp, vp, ci, vp, ci]
    lib.yfi_f16_of_u8_host.restype = None
    lib.yfi_f16_of_u8_host.argtypes = [vp]
    return lib


def host_fit(h, w, S):
    out = np.zeros(4, np.int32)
    fit_host().yfi_fit_host(h, w, S, out.ctypes.data)
    return tuple(int(v) for v in out)


@functools.lru_cache(maxsize=None)
def halves():
    out = np.zeros(256, np.uint16)
    fit_host().yfi_f16_of_u8_host(out.ctypes.data)
    out.setflags(write=False)
    return out


# ---- pictures ----
@functools.lru_cache(maxsize=None)
def seeded_rgb(h, w):
    """the seeded picture of a shape, uint8 [h, w, 3] in RGB order, read-only"""
    img = np.random.default_rng(7000 + 31 * h + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def real_rgb():
    """the 27 real pictures at the reference sizes, RGB order, read-only"""
    out = [np.ascontiguousarray(img[..., ::-1]) for img in real_images(_ptq())]
    for a in out:
        a.setflags(write=False)
    return tuple(out)


def in_format(rgb, fmt):
    """an RGB picture as format `fmt` stores it (the alpha of the 4-byte formats: a seeded byte that no frame may show)"""
    img = rgb[..., ::-1] if BGR[fmt] else rgb
    if FMT_CH[fmt] == 4:
        alpha = np.random.default_rng(rgb.shape[0] * 7 + rgb.shape[1]).integers(0, 256, rgb.shape[:2] + (1,), dtype=np.uint8)
        img = np.concatenate([img, alpha], axis=2)
    return np.ascontiguousarray(img)


def _key(rgb):
    return rgb.shape, rgb.tobytes()


@functools.lru_cache(maxsize=4096)
def _letterbox_cached(shape, data, S, pad):
    out = _ptq().letterbox_u8(np.frombuffer(data, np.uint8).reshape(shape), S, pad)
    out.setflags(write=False)
    return out


def expect_u8(rgb, S, pad):
    """ptq.letterbox_u8 of an RGB picture, computed once per (picture, S, pad): uint8 [S, S, 3]"""
    return _letterbox_cached(*_key(rgb), S, pad)


def expect_frame_fit(rgb, S, pad, f16=False):
    """the frame of an RGB picture: the bytes of `expect_u8` minus 128 as int8, or their halves as fp16 bits"""
    u8 = expect_u8(rgb, S, pad)
    return halves()[u8] if f16 else (u8.astype(np.int16) - 128).astype(np.int8)


def host_frame_packed(img, fmt, S, pad, f16=False, row_stride=None):
    """yfi_prepare_fit_host on one picture stored with `row_stride` (None: packed rows; the gap bytes are 0x5B) in a buffer of exactly
    its extent -> (status, frame)"""
    h, w, C = img.shape
    rs = w * C if row_stride is None else row_stride
    buf = np.full((h - 1) * rs + w * C, 0x5B, np.uint8)
    np.lib.stride_tricks.as_strided(buf, shape=(h, w * C), strides=(rs, 1))[:] = img.reshape(h, w * C)
    frame = np.full((S, S, 3), 0x1111 if f16 else 17, np.uint16 if f16 else np.int8)
    im = YfImage(0, h, w, rs)
    st = fit_host().yfi_prepare_fit_host(buf.ctypes.data, buf.nbytes, fmt, ctypes.byref(im), S, pad, int(f16), frame.ctypes.data)
    return st, frame


def host_frame_yuv(buf, d, v_first, S, pad, f16=False):
    """yfi_prepare_fit_yuv_host on one descriptor (a YUV_IMAGE_DTYPE record) of `buf` -> (status, frame)"""
    frame = np.full((S, S, 3), 0x1111 if f16 else 17, np.uint16 if f16 else np.int8)
    im = YfImageYuv(int(d["offset_y"]), int(d["offset_uv"]), int(d["height"]), int(d["width"]), int(d["stride_y"]), int(d["stride_uv"]))
    st = fit_host().yfi_prepare_fit_yuv_host(buf.ctypes.data, buf.nbytes, ctypes.byref(im), int(v_first), S, pad, int(f16), frame.ctypes.data)
    return st, frame


@functools.lru_cache(maxsize=None)
def seeded_surface(h, w):
    rng = np.random.default_rng(9000 + 17 * h + w)
    y, uv = rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w), dtype=np.uint8)
    y.setflags(write=False)
    uv.setflags(write=False)
    return y, uv


def surface_rgb(y, uv, v_first):
    rgb = _ptq().yuv420sp_to_rgb_u8(y, uv, v_first)
    rgb.setflags(write=False)
    return rgb


# ---- the decode, restated ----
def fit_scales(h, w, S):
    """(x0, y0, x_scale, y_scale) as float32, from ptq.letterbox_fit"""
    x0, y0, fw, fh = _ptq().letterbox_fit(h, w, S)
    return np.float32(x0), np.float32(y0), np.float32(np.float64(w) / np.float64(fw)), np.float32(np.float64(h) / np.float64(fh))


def boxes_restated(sx, sy, ew, eh, a, row, col, h, w, S):
    """float32 arrays of the four transcendental values and the candidates' (anchor, row, col) -> int32 [k, 4] edges in the picture's pixels"""
    x0, y0, xs, ys = fit_scales(h, w, S)
    eight, two = np.float32(8), np.float32(2)
    with np.errstate(over="ignore", invalid="ignore"):
        cx, cy = (sx + col.astype(np.float32)) * eight, (sy + row.astype(np.float32)) * eight
        bw, bh = ew * ANCHOR_W[a], eh * ANCHOR_H[a]
        x1, y1, x2, y2 = cx - bw / two, cy - bh / two, cx + bw / two, cy + bh / two
        x1, x2 = (x1 - x0) * xs, (x2 - x0) * xs
        y1, y2 = (y1 - y0) * ys, (y2 - y0) * ys
    for v in (x1, y1, x2, y2):
        assert v.dtype == np.float32
    return np.stack([to_int32(x1), to_int32(y1), to_int32(x2), to_int32(y2)], axis=1).reshape(-1, 4)


def _records(frame, keep, G, q_conf, conf, edges):
    recs = np.zeros(keep.shape[0], DET)
    recs["frame"] = frame
    recs["anchor"], recs["row"], recs["col"] = keep // (G * G), keep % (G * G) // G, keep % G
    recs["q_conf"], recs["conf"] = q_conf, conf
    recs["x1"], recs["y1"], recs["x2"], recs["y2"] = edges[:, 0], edges[:, 1], edges[:, 2], edges[:, 3]
    return recs


def decode_int8_restated(head, frame, h, w, S, sig, ex):
    """all records of one int8 head [G, G, 18] (G = S / 8) of a picture of h x w, in the order (anchor, row, col), as a DET array;
    sig, ex: the two float32 tables indexed by byte + 128"""
    G = S // 8
    c = np.asarray(head, np.int8).reshape(G, G, 3, 6).transpose(2, 0, 1, 3).reshape(-1, 6).astype(np.int64) + 128
    conf = sig[c[:, 4]]
    keep = np.nonzero(conf > np.float32(0.7))[0]
    k = c[keep]
    a, row, col = keep // (G * G), keep % (G * G) // G, keep % G
    edges = boxes_restated(sig[k[:, 0]], sig[k[:, 1]], ex[k[:, 2]], ex[k[:, 3]], a, row, col, h, w, S)
    return _records(frame, keep, G, (k[:, 4] - 128).astype(np.int8), conf[keep], edges)


def decode_f32_restated(logits, frame, h, w):
    """... of one frame's float32 logits [7, 7, 18]: sigmoid(x) = 1 / (1 + E(-x)), E = float_support.exp_rounded"""
    one = np.float32(1)
    t = np.asarray(logits, np.float32).reshape(7, 7, 3, 6).transpose(2, 0, 1, 3).reshape(-1, 6)

    def sigmoid(x):
        with np.errstate(over="ignore", invalid="ignore"):
            return one / (one + exp_rounded(-x))

    conf = sigmoid(t[:, 4])
    keep = np.nonzero(conf > np.float32(0.7))[0]
    k = t[keep]
    a, row, col = keep // 49, keep % 49 // 7, keep % 7
    edges = boxes_restated(sigmoid(k[:, 0]), sigmoid(k[:, 1]), exp_rounded(k[:, 2]), exp_rounded(k[:, 3]), a, row, col, h, w, 56)
    return _records(frame, keep, 7, 0, conf[keep], edges)


def host_decode_int8(head, frame, h, w, S, cap, status=0):
    """(true count, the records written) of yfi_decode_fit_host; slots beyond min(count, cap) must keep 0xA5"""
    hd = np.ascontiguousarray(head, np.int8)
    recs = np.frombuffer(bytes([0xA5]) * (28 * cap), DET).copy()
    count = fit_host().yfi_decode_fit_host(hd.ctypes.data, frame, h, w, status, S, recs.ctypes.data, cap)
    k = min(count, cap)
    assert (recs[k:].view(np.uint8) == 0xA5).all()
    return count, recs[:k]


def host_decode_f32(logits, frame, h, w, cap, status=0):
    t = np.ascontiguousarray(logits, np.float32)
    recs = np.frombuffer(bytes([0xA5]) * (28 * cap), DET).copy()
    count = fit_host().yfi_decode_f32_fit_host(t.ctypes.data, frame, h, w, status, recs.ctypes.data, cap)
    k = min(count, cap)
    assert (recs[k:].view(np.uint8) == 0xA5).all()
    return count, recs[:k]


def sizes_desc(sides):
    """[(h, w)] -> IMAGE_DTYPE[n] as the decodes read it (only the sides count; offset and stride carry bytes they must not read)"""
    images = importlib.import_module("stm32h7-yolo_amd.images")
    desc = np.zeros(len(sides), images.IMAGE_DTYPE)
    for i, (h, w) in enumerate(sides):
        desc[i] = (0xDEADBEEF00 + i, h, w, -5)
    return desc

