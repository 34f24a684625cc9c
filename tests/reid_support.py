"""What the tests of the appearance descriptors and the re-identification share (test_reid_*): the descriptor, entry and state layouts
as numpy dtypes, the expectations of a call -- `ptq.describe_u8` / `ptq.describe_yuv420sp` and `ptq.reid_step`, the plain-Python
statements of csrc/yf_images_describe.h and csrc/yf_images_reid.h --, the host build's prototypes with runners that put guard bytes in
front of and behind every array a call may write, the designed cases, the seeded random ones and the textured clips of the behavioural
test.  The record and info layouts, the guards and the layouts of a call are tests/track_support.py's.

A descriptor batch is a `Batch`: pictures (uint8 [H, W, C] arrays, or (y, uv) pairs), per picture the boxes (x1, y1, x2, y2) and the
count (None: their number).  A re-identification scene is `frames[s][t] = (records, descs, count)`: the tracker's info rows (id, hits,
misses, age) of stream s at step t in the order they lie, per record its 64 descriptor bytes or None, and the count (None: the
length); the places of a row that hold nothing are 0xA5 bytes."""
import ctypes
import functools
import os
import re
from collections import namedtuple

import numpy as np

import track_support as ts
from conftest import ROOT
from images_support import host_lib

DESC = np.dtype([("flags", "<u4"), ("v", "u1", (64,))])
ENTRY = np.dtype([("id", "<u4"), ("alias", "<u4"), ("seen", "<u4"), ("flags", "<u4"), ("v", "u1", (64,))])
STATE = np.dtype([("clock", "<u4"), ("reserved", "<u4"), ("entry", ENTRY, (64,))])
IMAGE = np.dtype([("offset", "<u8"), ("height", "<i4"), ("width", "<i4"), ("row_stride", "<i8")])
YUV_IMAGE = np.dtype([("offset_y", "<u8"), ("offset_uv", "<u8"), ("height", "<i4"), ("width", "<i4"), ("stride_y", "<i8"), ("stride_uv", "<i8")])
assert (DESC.itemsize, ENTRY.itemsize, STATE.itemsize, IMAGE.itemsize, YUV_IMAGE.itemsize) == (68, 80, 5128, 24, 40)
CLIPPED, VOID = 1, 2
KNOWN, REIDENTIFIED, BORN = 1, 2, 3
U32MAX = 2 ** 32 - 1
FORMATS = {"bgr": 0, "rgb": 1, "bgra": 2, "rgba": 3, "nv12": 4, "nv21": 5}
MAX_DISTANCE = 64 * 64 * 255


class Params(ctypes.Structure):
    _fields_ = [("max_distance", ctypes.c_int32), ("max_age", ctypes.c_int32), ("blend", ctypes.c_int32)]


@functools.lru_cache(maxsize=None)
def reid_host():
    """libyf_images_host.so with the prototypes of the host build of csrc/yf_images_describe.h and csrc/yf_images_reid.h added"""
    lib = host_lib()
    vp, ci, cl, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_uint64
    for name in ("yfi_describe_records_host", "yfi_describe_records_yuv_host"):
        getattr(lib, name).restype = cl
        getattr(lib, name).argtypes = [vp, u64, ci, vp, vp, vp, cl, ci, ci, ci, vp, vp, vp]
    lib.yfi_describe_check_host.restype = ci
    lib.yfi_describe_check_host.argtypes = [vp, vp, vp, vp, cl, ci, ci, ci, vp, vp, vp, ctypes.c_char_p, ci]
    lib.yf_images_reid_host.restype = cl
    lib.yf_images_reid_host.argtypes = [vp, vp, vp, ci, cl, cl, ci, vp, vp, vp, vp, vp, vp]
    lib.yfi_reid_check_host.restype = ci
    lib.yfi_reid_check_host.argtypes = [vp, vp, vp, ci, cl, cl, ci, vp, vp, vp, vp, vp, ctypes.c_char_p, ci]
    lib.yf_images_reid_state_bytes_host.restype = ctypes.c_size_t
    lib.yf_images_reid_state_bytes_host.argtypes = [cl]
    lib.yfi_reid_distance_host.restype = ctypes.c_int32
    lib.yfi_reid_distance_host.argtypes = [vp, vp]
    return lib


def ptq():
    return ts._mod("ptq")


# ================================================================ descriptors ================================================================
Batch = namedtuple("Batch", "name fmt pictures boxes counts cap margin square pad bad")
Batch.__new__.__defaults__ = (0, False, 0, ())
DescResult = namedtuple("DescResult", "rc desc first status")


def texture(rng, h, w, c=3):
    """a random smooth texture uint8 [h, w, c]: noise on a 4 x 4 lattice, stretched"""
    coarse = rng.integers(0, 256, (4, 4, c)).astype(np.float64)
    ys, xs = np.linspace(0, 3, h), np.linspace(0, 3, w)
    y0, x0 = np.minimum(ys.astype(int), 2), np.minimum(xs.astype(int), 2)
    fy, fx = (ys - y0)[:, None, None], (xs - x0)[None, :, None]
    out = (coarse[y0][:, x0] * (1 - fy) * (1 - fx) + coarse[y0][:, x0 + 1] * (1 - fy) * fx + coarse[y0 + 1][:, x0] * fy * (1 - fx)
           + coarse[y0 + 1][:, x0 + 1] * fy * fx)
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def noise(rng, h, w, c):
    return rng.integers(0, 256, (h, w, c) if c else (h, w), dtype=np.uint8)


def surface(rng, h, w):
    """an NV12 / NV21 surface of random bytes: (y [h, w], uv [h / 2, w])"""
    return noise(rng, h, w, 0), noise(rng, h // 2, w, 0)


def pack(batch):
    """-> (buf uint8, descriptors IMAGE / YUV_IMAGE [n], dets RAW [n, cap], counts int32 [n]); every row is `pad` bytes longer than its
    pixels (odd strides), 0xEE between the pictures; the descriptors in batch.bad get a height that does not fit the buffer"""
    yuv = batch.fmt in ("nv12", "nv21")
    n = len(batch.pictures)
    desc = np.zeros(max(n, 1), YUV_IMAGE if yuv else IMAGE)
    parts, at = [], 5
    parts.append(np.full(5, 0xEE, np.uint8))

    def place(plane):
        nonlocal at
        rows, row_bytes = plane.shape[0], int(np.prod(plane.shape[1:]))
        stride = row_bytes + batch.pad
        block = np.full(rows * stride + 3, 0xEE, np.uint8)
        for r in range(rows):
            block[r * stride:r * stride + row_bytes] = plane[r].reshape(-1)
        parts.append(block)
        start, at = at, at + block.size
        return start, stride
    for i, pic in enumerate(batch.pictures):
        if yuv:
            y, uv = pic
            oy, sy = place(y)
            ouv, suv = place(uv)
            desc[i] = (oy, ouv, y.shape[0], y.shape[1], sy, suv)
        else:
            o, s = place(pic)
            desc[i] = (o, pic.shape[0], pic.shape[1], s)
    for i in batch.bad:
        desc[i]["height"] = 16384
    buf = np.concatenate(parts)
    dets = np.frombuffer(bytes([0xA5]) * (max(n, 1) * batch.cap * 28), ts.RAW).reshape(max(n, 1), batch.cap).copy()
    counts = np.zeros(max(n, 1), np.int32)
    for i in range(n):
        counts[i] = len(batch.boxes[i]) if batch.counts is None or batch.counts[i] is None else batch.counts[i]
        for j, box in enumerate(batch.boxes[i][:batch.cap]):
            dets[i, j] = (i, 0, 0, j % 7, 5, ts.conf_bits(j), *box)
    return buf, desc, dets, counts


def desc_sentinels(n, cap):
    n = max(n, 1)
    return (np.frombuffer(bytes([0xA5]) * (n * cap * 68), DESC).reshape(n, cap).copy(), np.full(n + 1, ts.SENTINEL32, np.int32),
            np.full(n, ts.SENTINEL32, np.int32))


def describe_expected(batch):
    """the call by the Python statement -> DescResult"""
    p = ptq()
    n = len(batch.pictures)
    buf, descs, dets, counts = pack(batch)
    desc, first, status = desc_sentinels(n, batch.cap)
    total = 0
    yuv = batch.fmt in ("nv12", "nv21")
    for i in range(n):
        m = min(max(int(counts[i]), 0), batch.cap)
        # a surface with an odd side is no valid picture (yfi_yuv_image_ok)
        bad = i in batch.bad or (yuv and (batch.pictures[i][0].shape[0] % 2 != 0 or batch.pictures[i][0].shape[1] % 2 != 0))
        first[i], status[i] = total, 1 if bad else 0
        total += m
        for s in range(m):
            box = tuple(int(dets[i, s][k]) for k in ("x1", "y1", "x2", "y2"))
            if bad:
                v = None
            elif batch.fmt in ("nv12", "nv21"):
                v = p.describe_yuv420sp(batch.pictures[i][0], box, batch.margin, batch.square)
            else:
                v = p.describe_u8(batch.pictures[i], box, batch.fmt, batch.margin, batch.square)
            desc[i, s] = (0, np.zeros(64, np.uint8)) if v is None else (1, np.array(v, np.uint8))
    if n:
        first[n] = total
    return DescResult(n, desc, first, status)


def describe_run_with(fn, batch, upload=None, download=None, n=None):
    """`fn(pixels, bytes, format, images, dets, counts, n, cap, margin, flags, desc, first, status)` on addresses, every written array
    between guard bytes -> DescResult"""
    n = len(batch.pictures) if n is None else n
    buf, descs, dets, counts = pack(batch)
    arrays = list(desc_sentinels(len(batch.pictures), batch.cap))
    bufs = [ts.guarded(a)[0] for a in arrays]
    ins = [buf, descs.view(np.uint8).reshape(-1), dets.view(np.uint8).reshape(-1), counts.view(np.uint8).reshape(-1)]
    if upload is not None:
        bufs, ins = [upload(b) for b in bufs], [upload(a) for a in ins]
        addr = lambda b: b.data_ptr()
    else:
        ins = [np.ascontiguousarray(a) for a in ins]
        addr = lambda b: b.ctypes.data
    p = [addr(b) + ts.GUARD for b in bufs]
    rc = fn(addr(ins[0]), buf.size, FORMATS[batch.fmt], addr(ins[1]), addr(ins[2]), addr(ins[3]), n, batch.cap, batch.margin,
            1 if batch.square else 0, p[0], p[1], p[2])
    if download is not None:
        bufs = [download(b) for b in bufs]
    assert all(ts.guards_intact(b) for b in bufs), "a byte outside an array was written"
    got = [b[ts.GUARD:-ts.GUARD].view(a.dtype).reshape(a.shape) for a, b in zip(arrays, bufs)]
    return DescResult(rc, *got)


def describe_host_run(batch, n=None):
    lib = reid_host()
    fn = lib.yfi_describe_records_yuv_host if batch.fmt in ("nv12", "nv21") else lib.yfi_describe_records_host
    return describe_run_with(fn, batch, n=n)


def same_desc(a, b):
    return a.rc == b.rc and all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:]))


def _picture(rng, fmt, h, w):
    if fmt in ("nv12", "nv21"):
        return surface(rng, h, w)
    return noise(rng, h, w, 4 if fmt.endswith("a") else 3)


@functools.lru_cache(maxsize=None)
def describe_batches():
    """the designed descriptor batches -> [Batch]"""
    rng = np.random.default_rng(9100)
    out = []
    # the region sizes: 8 x 8 the smallest valid, 7 x 8 and 8 x 7 invalid, 9 x 13 uneven cells, 64 x 40; a record without a region (an
    # inverted box, a box outside the picture); an odd origin; in every format, with odd row strides
    sized = [(3, 5, 10, 12), (3, 5, 9, 12), (3, 5, 10, 11), (1, 1, 9, 13), (7, 3, 70, 42), (20, 20, 10, 30), (200, 5, 230, 40), (5, 7, 33, 29)]
    for fmt in FORMATS:
        out.append(Batch("sizes_" + fmt, fmt, [_picture(rng, fmt, 50, 82)], [sized], None, 8, pad=3 if fmt not in ("nv12", "nv21") else 1))
    # a region clipped at each picture border, and one that covers the picture
    clipped = [(-5, 10, 12, 30), (60, 10, 200, 30), (10, -9, 40, 11), (10, 40, 40, 90), (-100, -100, 500, 500)]
    out.append(Batch("borders", "rgb", [noise(rng, 50, 82, 3)], [clipped], None, 5, pad=1))
    out.append(Batch("borders_nv12", "nv12", [surface(rng, 50, 82)], [clipped], None, 5, pad=5))
    # margin and square, which move the region
    out.append(Batch("margin", "bgr", [noise(rng, 61, 97, 3)], [[(30, 20, 50, 33), (2, 2, 20, 11)]], None, 2, margin=250, square=True, pad=2))
    # 0, 1 and cap records; a count above cap and a negative one; an invalid picture between valid ones
    boxes = [[], [(0, 0, 7, 7)], [(0, 0, 7, 7), (1, 1, 20, 20), (4, 4, 30, 19)], [(0, 0, 11, 11), (3, 3, 12, 12), (2, 2, 22, 22)], [(0, 0, 9, 9)],
             [(0, 0, 8, 8), (5, 5, 15, 15)]]
    pics = [noise(rng, 8, 8, 3), noise(rng, 8, 8, 3), noise(rng, 40, 33, 3), noise(rng, 61, 97, 3), noise(rng, 24, 24, 3), noise(rng, 24, 24, 3)]
    out.append(Batch("counts", "bgr", pics, boxes, [None, None, None, 7, -3, None], 3, pad=1, bad=(5,)))
    # a constant region: 64 equal bytes (grey 93 has luma 93; the surface's Y plane is 201)
    flat = np.full((30, 30, 3), 93, np.uint8)
    out.append(Batch("constant", "rgba", [np.concatenate([flat, noise(rng, 30, 30, 1)], axis=2)], [[(2, 3, 25, 19)]], None, 1))
    out.append(Batch("constant_nv21", "nv21", [(np.full((30, 30), 201, np.uint8), noise(rng, 15, 30, 0))], [[(2, 3, 25, 19)]], None, 1))
    return out


def gpu_describe_batches():
    """a batch with 0, 1 and cap records per frame over pictures of 8 x 8 up to 97 x 61, packed and NV12 (where the 97 x 61 surface,
    with its odd sides, is an invalid picture: its records get zero descriptors; a 96 x 60 one follows it)"""
    rng = np.random.default_rng(9150)
    out = []
    for fmt in ("bgr", "rgba", "nv12"):
        sizes = [(8, 8), (20, 32), (61, 97), (34, 50), (60, 96)]
        pics = [_picture(rng, fmt, h, w) for h, w in sizes]
        many = [(int(x), int(y), int(x + w), int(y + h)) for x, y, w, h in zip(rng.integers(-5, 70, 6), rng.integers(-5, 40, 6), rng.integers(5, 60, 6),
                                                                              rng.integers(5, 50, 6))]
        boxes = [[], [(0, 0, 7, 7)], many, [(3, 3, 40, 30)], many]
        out.append(Batch("ragged_" + fmt, fmt, pics, boxes, None, 6, pad=1))
    return out


D_VALID = dict(pixels=8, images=8, dets=8, counts=8, n=2, cap=4, margin=0, flags=0, desc=8, first=8, status=8)
D_NAMES = tuple(D_VALID)
D_FAULTS = [(dict(n=-1), "n must"), (dict(n=2 ** 31 - 1), "n must"), (dict(cap=0), "cap must"), (dict(cap=1201), "cap must"),
            (dict(n=2 ** 22, cap=1024), "n * cap"), (dict(margin=-1), "margin_permille"), (dict(margin=1001), "margin_permille"), (dict(flags=2), "flags"),
            (dict(dets=0), "is NULL"), (dict(counts=0), "is NULL"), (dict(desc=0), "is NULL"), (dict(first=0), "is NULL"), (dict(status=0), "is NULL"),
            (dict(dets=6), "4-byte aligned"), (dict(counts=5), "4-byte aligned"), (dict(desc=10), "4-byte aligned"), (dict(first=7), "4-byte aligned"),
            (dict(status=9), "4-byte aligned"), (dict(pixels=0), "d_pixels is NULL"), (dict(images=0), "d_images"), (dict(images=12), "d_images")]


def describe_host_check(**kw):
    a = dict(D_VALID, **kw)
    text = ctypes.create_string_buffer(256)
    rc = reid_host().yfi_describe_check_host(*(a[k] for k in D_NAMES), text, 256)
    assert rc == (text.value != b"")
    return text.value.decode()


# ============================================================= re-identification =============================================================
Case = namedtuple("Case", "name frames out_cap params state0")
Result = namedtuple("Result", "rc state info what status")


def same(a, b):
    return a.rc == b.rc and all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:]))


def lay_out(frames, out_cap, layout):
    """frames[s][t] = (records, descs, count) -> (info INFO [n, out_cap], counts int32 [n], desc DESC [n, out_cap]) of a call in `layout`"""
    streams, steps = len(frames), len(frames[0]) if frames else 0
    n = max(streams * steps, 1)
    info = np.frombuffer(bytes([0xA5]) * (n * out_cap * 16), ts.INFO).reshape(n, out_cap).copy()
    desc = np.frombuffer(bytes([0xA5]) * (n * out_cap * 68), DESC).reshape(n, out_cap).copy()
    counts = np.zeros(n, np.int32)
    for s in range(streams):
        assert len(frames[s]) == steps
        for t in range(steps):
            records, descs, count = frames[s][t]
            f = ts.frame_of(s, t, streams, steps, layout)
            assert len(records) <= out_cap and len(descs) == len(records)
            counts[f] = len(records) if count is None else count
            for j, (row, d) in enumerate(zip(records, descs)):
                info[f, j] = row
                # an invalid descriptor as the describe entry writes it, or -- every third -- with junk behind a flags word whose bit 0 is clear
                desc[f, j] = (1, np.array(d, np.uint8)) if d is not None else ((0, np.zeros(64, np.uint8)) if j % 3 else (0xA5A5A5A4, np.full(64, 0xA5, np.uint8)))
    return info, counts, desc


def empty_state(streams):
    return np.zeros(max(streams, 1), STATE)


def state_to_py(rec):
    return {"clock": int(rec["clock"]), "reserved": int(rec["reserved"]),
            "entries": [{"id": int(e["id"]), "alias": int(e["alias"]), "seen": int(e["seen"]), "flags": int(e["flags"]), "v": e["v"].tolist()}
                        for e in rec["entry"]]}


def py_to_state(st):
    rec = np.zeros((), STATE)
    rec["clock"], rec["reserved"] = st["clock"], st["reserved"]
    for k, e in enumerate(st["entries"]):
        rec["entry"][k] = (e["id"], e["alias"], e["seen"], e["flags"], np.array(e["v"], np.uint8))
    return rec


def sentinels(n, out_cap):
    n = max(n, 1)
    return (np.frombuffer(bytes([0xA5]) * (n * out_cap * 16), ts.INFO).reshape(n, out_cap).copy(), np.full((n, out_cap), ts.SENTINEL32, np.int32),
            np.full(n, ts.SENTINEL32, np.int32))


def expected(call, streams, steps, layout, out_cap, params, state0, in_place=False):
    """the call by the Python statement -> Result; nothing of the inputs is changed"""
    p = ptq()
    info, counts, desc = call
    n = streams * steps
    info_out, what, status = sentinels(n, out_cap)
    if in_place:
        info_out = info.copy()
    state = state0[:max(streams, 1)].copy()
    for s in range(streams):
        st = state_to_py(state[s])
        for t in range(steps):
            f = ts.frame_of(s, t, streams, steps, layout)
            m = min(max(int(counts[f]), 0), out_cap, 64)
            records = [tuple(int(info[f, k][name]) for name in ts.INFO.names) for k in range(m)]
            descs = [desc[f, k]["v"].tolist() if int(desc[f, k]["flags"]) & 1 else None for k in range(m)]
            st, ids, kinds, bits = p.reid_step(st, records, descs, params, count=int(counts[f]), out_cap=out_cap)
            for k in range(m):
                info_out[f, k] = (ids[k],) + records[k][1:]
                what[f, k] = kinds[k]
            for k in range(m, min(max(int(counts[f]), 0), out_cap)):
                info_out[f, k], what[f, k] = info[f, k], 0
            status[f] = bits
        state[s] = py_to_state(st)
    return Result(n, state, info_out, what, status)


def run_with(fn, call, streams, steps, layout, out_cap, params, state0, with_what=True, with_status=True, in_place=False, upload=None,
             download=None):
    """`fn(info, out_counts, desc, out_cap, streams, steps, layout, params, state, info_out, what, status)` on addresses, every written
    array between guard bytes -> Result.  in_place: d_info_out is d_info.  upload / download: the way to the device and back"""
    n = streams * steps
    info, counts, desc = call
    arrays = [state0[:max(streams, 1)].copy(), *sentinels(n, out_cap)]
    if in_place:
        arrays[1] = info.copy()
    bufs = [ts.guarded(a)[0] for a in arrays]
    ins = [np.ascontiguousarray(a).view(np.uint8).reshape(-1) for a in (info, counts, desc)]
    if upload is not None:
        bufs, ins = [upload(b) for b in bufs], [upload(a) for a in ins]
        addr = lambda b: b.data_ptr()
    else:
        addr = lambda b: b.ctypes.data
    p = [addr(b) + ts.GUARD for b in bufs]
    par = None if params is None else ctypes.byref(Params(*params))
    rc = fn(p[1] if in_place else addr(ins[0]), addr(ins[1]), addr(ins[2]), out_cap, streams, steps, layout, par, p[0], p[1], p[2] if with_what else None,
            p[3] if with_status else None)
    if download is not None:
        bufs = [download(b) for b in bufs]
    assert all(ts.guards_intact(b) for b in bufs), "a byte outside an array was written"
    got = [b[ts.GUARD:-ts.GUARD].view(a.dtype).reshape(a.shape) for a, b in zip(arrays, bufs)]
    return Result(rc, *got)


def host_run(call, streams, steps, layout, out_cap, params, state0, with_what=True, with_status=True, in_place=False):
    lib = reid_host()
    fn = lambda *a: lib.yf_images_reid_host(*a, None)
    return run_with(fn, call, streams, steps, layout, out_cap, params, state0, with_what, with_status, in_place)


VALID = dict(info=8, out_counts=8, desc=8, out_cap=4, streams=2, steps=3, layout=ts.TIME, params=(1000, 30, 64), state=8, info_out=8, what=8, status=0)
NAMES = tuple(VALID)
POINTERS = ("info", "out_counts", "desc", "state", "info_out", "what", "status")
FAULTS = [(dict(info=0), "is NULL"), (dict(out_counts=0), "is NULL"), (dict(desc=0), "is NULL"), (dict(params=None), "is NULL"), (dict(state=0), "is NULL"),
          (dict(info_out=0), "is NULL"), (dict(info=10), "4-byte aligned"), (dict(out_counts=5), "4-byte aligned"), (dict(desc=6), "4-byte aligned"),
          (dict(info_out=7), "4-byte aligned"), (dict(what=2), "4-byte aligned"), (dict(status=6), "4-byte aligned"), (dict(state=12), "8-byte aligned"),
          (dict(out_cap=0), "out_cap"), (dict(out_cap=-4), "out_cap"), (dict(params=(-1, 30, 64)), "max_distance"), (dict(params=(5, -1, 64)), "max_age"),
          (dict(params=(5, 30, -1)), "blend"), (dict(params=(5, 30, 257)), "blend"), (dict(layout=2), "layout"), (dict(layout=-1), "layout"),
          (dict(streams=-1), "streams and steps"), (dict(steps=-1), "streams and steps"), (dict(streams=2 ** 31, steps=1), "streams * steps"),
          (dict(streams=65536, steps=32768), "streams * steps")]


def call_args(a):
    """the arguments of a check or an entry from a dict of VALID's keys: params as a pointer (None: NULL), 0 pointers as NULL"""
    par = None if a["params"] is None else ctypes.byref(Params(*a["params"]))
    return [par if k == "params" else ((a[k] or None) if k in POINTERS else a[k]) for k in NAMES]


def host_check(**kw):
    text = ctypes.create_string_buffer(256)
    rc = reid_host().yfi_reid_check_host(*call_args(dict(VALID, **kw)), text, 256)
    assert rc == (text.value != b"")
    return text.value.decode()


# ---- the designed scenes ----
def vec(seed, offset=0):
    """a descriptor of 64 seeded random bytes in [40, 215], plus an offset: room to add and subtract without clipping"""
    return (np.random.default_rng(seed).integers(40, 216, 64) + offset).tolist()


def rec(tid, misses=0, hits=3, age=7):
    return (tid, hits, misses, age)


def crafted(entries, clock=100, reserved=0):
    """a state of one stream: entries = {index: (id, alias, seen, flags, v or None)}"""
    st = empty_state(1)
    st["clock"], st["reserved"] = clock, reserved
    for k, (eid, alias, seen, flags, v) in entries.items():
        st["entry"][0, k] = (eid, alias, seen, flags, np.zeros(64, np.uint8) if v is None else np.array(v, np.uint8))
    return st


def at_distance(a, d):
    """a descriptor at distance exactly d from a, d a multiple of 126: byte 0 raised by k changes its own term by 64 k - k and each of
    the other 63 terms by k, the sum having grown by k -- distance 63 k + 63 k = 126 k"""
    assert d % 126 == 0
    b = list(a)
    b[0] += d // 126
    assert 0 <= b[0] <= 255 and ptq().reid_distance(a, b) == d
    return b


def junk_state(streams, seed=9300):
    """states of random bytes; in every stream the aliases of entries 3, 9 and 40 are made equal to that of entry 1 (duplicated aliases),
    entry 5 is free, and stream 0's clock is just below 2^32"""
    rng = np.random.default_rng(seed)
    st = np.frombuffer(rng.integers(0, 256, streams * STATE.itemsize, dtype=np.uint8).tobytes(), STATE).copy()
    for k in (3, 9, 40):
        st["entry"]["alias"][:, k] = st["entry"]["alias"][:, 1]
    st["entry"]["id"][:, 5] = 0
    st["clock"][0] = U32MAX - 1
    return st


def full_state(clock=1000, n=64, with_desc=True, seed=9400):
    """a table with its first n entries taken: entry k has id 500 + k, alias 100 + k, seen clock - 1 - k % 7 (so that ages tie), a
    descriptor of its own"""
    return crafted({k: (500 + k, 100 + k, clock - 1 - k % 7, 1 if with_desc else 0, vec(seed + k) if with_desc else None) for k in range(n)}, clock)


@functools.lru_cache(maxsize=None)
def designed():
    """the designed scenes, each at the smallest size that can go wrong -> [Case]"""
    a, b, c = vec(1), vec(2), vec(3)
    cases = []
    # the hand-counted minimal case: track 7 with face a is born (entry 0), seen again, lost; track 9 is born with the same face three
    # frames later and takes identity 7; a track 11 with face b in the same frame is born as itself
    lost = [[([rec(7)], [a], None), ([rec(7)], [a], None), ([], [], None), ([], [], None), ([rec(9), rec(11)], [a, b], None),
             ([rec(11), rec(9)], [b, a], None)]]
    cases.append(Case("lost_and_found", lost, 2, (0, 10, 128), None))
    # age equal to max_age is kept, max_age + 1 is freed: entry 0 was seen at 90 and entry 1 at 89, the step's clock is 100
    aged = crafted({0: (7, 7, 90, 1, a), 1: (8, 8, 89, 1, b)}, clock=99)
    cases.append(Case("ages", [[([rec(20), rec(21)], [a, b], None)]], 2, (0, 10, 256), aged))
    # a clock just below 2^32 that wraps: entry 0 was seen at 2^32 - 3; the steps' clocks are 2^32 - 1, 0, 1, 2: ages 2 .. 5 against
    # max_age 4 -- the face that returns at clock 1 finds its entry, the one that returns at clock 2 does not
    wrap = crafted({0: (7, 7, U32MAX - 2, 1, a)}, clock=U32MAX - 1)
    cases.append(Case("wrap", [[([], [], None)] * 2 + [([rec(30)], [a], None)]], 1, (0, 4, 256), wrap))
    cases.append(Case("wrap_late", [[([], [], None)] * 3 + [([rec(30)], [a], None)]], 1, (0, 4, 256), wrap))
    # distance equal to max_distance is eligible, one step above is not (the distances of one raised byte are multiples of 126)
    near = crafted({0: (7, 7, 99, 1, a), 1: (8, 8, 99, 1, b)}, clock=100)
    cases.append(Case("threshold", [[([rec(40), rec(41)], [at_distance(a, 1260), at_distance(b, 1386)], None)]], 2, (1260, 10, 0), near))
    # a tie in distance between two records (the same face twice: the lower record wins the entry, the other is born) and between two
    # entries (the same descriptor twice: the lower entry is taken)
    cases.append(Case("tie_records", [[([rec(40), rec(41)], [at_distance(a, 126), at_distance(a, 126)], None)]], 2, (5000, 10, 64), crafted({3: (7, 7, 99, 1, a)})))
    cases.append(Case("tie_entries", [[([rec(40)], [at_distance(a, 252)], None)]], 1, (5000, 10, 64), crafted({2: (7, 7, 99, 1, a), 6: (8, 8, 99, 1, a)})))
    # the smallest distance goes first, whatever the order of the records: record 1 is nearer to entry 0 than record 0 is
    cases.append(Case("nearest_first", [[([rec(40), rec(41)], [at_distance(a, 630), at_distance(a, 126)], None)]], 2, (5000, 10, 256),
                      crafted({0: (7, 7, 99, 1, a), 1: (8, 8, 99, 1, at_distance(a, 2520))})))
    # records of id 0 (void), two records of one id (both bound to one entry, whose descriptor meets both), a held-over record (misses
    # > 0: bound, but its descriptor is not taken, and unbound it is no candidate but is born), invalid descriptors
    known = crafted({0: (7, 70, 99, 1, a), 1: (8, 80, 99, 0, None), 2: (9, 90, 99, 1, c)})
    odd = [[([rec(0), rec(70), rec(70), rec(80, misses=2), rec(80), rec(55, misses=1), rec(0, misses=3), rec(56)], [a, b, c, b, None, c, a, None], None),
            ([rec(56), rec(55), rec(80)], [a, c, b], None)]]
    cases.append(Case("odd_records", odd, 8, (3000, 10, 128), known))
    # blend 0 (the stored descriptor never moves: the face a + 9 still finds it at distance 0), 128 and 256 (it is replaced by the last
    # face seen, c, and a + 9 is born)
    for blend in (0, 128, 256):
        cases.append(Case("blend_%d" % blend, [[([rec(70)], [b], None), ([rec(70)], [c], None), ([rec(71)], [vec(1, 9)], None)]], 1, (1000, 10, blend),
                          crafted({0: (7, 70, 99, 1, a)})))
    # counts above the capacity, above 64 and below 0; a cap above 64, whose records beyond 64 are copied as they are
    many = [rec(200 + k) for k in range(70)]
    cases.append(Case("counts", [[(many[:3], [a, b, c], 9), (many[:3], [a, b, c], -2), (many[:3], [a, b, c], 0), (many[:2], [a, b], None)]], 3, (0, 10, 64), None))
    cases.append(Case("beyond_64", [[(many, [vec(100 + k) for k in range(70)], None), (many, [vec(100 + k) for k in range(70)], 69)]], 70, (0, 10, 64), None))
    # 0, 1, 2, 63 and 64 records against an empty, a half-full and a full table; with a full table the births evict the unbound entry of
    # the largest age, ties to the lowest index
    for name, st in (("empty", None), ("half", full_state(n=32)), ("full", full_state())):
        for m in (0, 1, 2, 63, 64):
            recs = [rec(100 + 2 * k if k % 3 else 900 + k) for k in range(m)]                # a third of them known (with a half or full table)
            ds = [vec(9400 + 2 * k) if k % 5 else None for k in range(m)]
            cases.append(Case("%s_%d" % (name, m), [[(recs, ds, None), (recs[::-1], ds[::-1], None)]], 64, (2000, 3, 64), st))
    # a full table without descriptors, every entry unbound and of the same age: eviction from the lowest index on
    cases.append(Case("evict", [[([rec(900 + k) for k in range(5)], [vec(k) for k in range(5)], None)]], 5, (0, 1000, 64), full_state(with_desc=False)))
    # a state of random bytes with duplicated aliases
    junk = junk_state(2)
    alias = int(junk["entry"]["alias"][0, 1])
    cases.append(Case("junk", [[([rec(alias), rec(77), rec(alias)], [a, b, c], None), ([rec(77), rec(78)], [b, a], None)],
                               [([rec(int(junk["entry"]["alias"][1, 1]))], [None], None), ([], [], None)]], 3, (300000, 2 ** 31 - 1, 77), junk))
    return cases


def laid_out(case, layout):
    """-> (call, streams, steps, state0) of a designed case"""
    streams, steps = len(case.frames), len(case.frames[0])
    return lay_out(case.frames, case.out_cap, layout), streams, steps, (empty_state(streams) if case.state0 is None else case.state0)


# ---- seeded random clips ----
@functools.lru_cache(maxsize=None)
def drift_frames(streams, steps, seed=9500):
    """`streams` x `steps` small frames for the shape sweeps (at most 6 records a frame): a handful of faces with a descriptor each that
    drifts a little; a face's track dies now and then and returns under a new tracker id; about a fifth of the records held over, a few
    void, a few without a descriptor"""
    rng = np.random.default_rng(seed + 1000 * streams + steps)
    frames = []
    for s in range(streams):
        faces = [vec(int(rng.integers(1, 10 ** 6))) for _ in range(int(rng.integers(2, 7)))]
        tids = list(range(1, len(faces) + 1))
        issued = len(faces)
        clip = []
        for t in range(steps):
            rows = []
            for k, face in enumerate(faces):
                if rng.random() < 0.15:
                    issued += 1
                    tids[k] = issued
                if rng.random() < 0.25:
                    continue
                d = [min(255, max(0, v + int(j))) for v, j in zip(face, rng.integers(-2, 3, 64))]
                rows.append((rec(0 if rng.random() < 0.05 else tids[k], misses=int(rng.random() < 0.2)), d if rng.random() > 0.1 else None))
            order = rng.permutation(len(rows))
            clip.append(([rows[int(k)][0] for k in order], [rows[int(k)][1] for k in order], None))
        frames.append(clip)
    return frames


D_CAP, D_PARAMS = 6, (9000, 2, 64)


def split_calls(run, call, streams, steps, out_cap, params, state0):
    """`steps` calls of one step each on time-major arrays, the state carried -> the Result one call of `steps` steps must give"""
    state, parts = state0, []
    for t in range(steps):
        part = tuple(a[t * streams:(t + 1) * streams] for a in call)
        r = run(part, streams, 1, ts.TIME, out_cap, params, state)
        assert r.rc == streams
        state = r.state
        parts.append(r)
    return Result(streams * steps, state, *(np.concatenate([getattr(p, name) for p in parts]) for name in ("info", "what", "status")))


def per_cu():
    """the workgroups of the kernel that a CU holds at once, the measure of the launcher's grid: the constant the launcher itself takes,
    read from csrc/yf_images_reid.hip.h"""
    text = open(os.path.join(ROOT, "stm32h7-yolo_amd", "csrc", "yf_images_reid.hip.h")).read()
    return int(re.search(r"\bkPerCuReid = (\d+)", text).group(1))


# ================================================================ textured clips ================================================================
CLIP_H, CLIP_W, FACE = 96, 160, 32
CLIP_TRACKER = (0.3, 1, 5)                       # match_iou, min_hits, max_misses
CLIP_MAX_DISTANCE = 60000                        # between the same-face and the different-face distances of these clips (asserted in the tests)


def textured_clip(kind, steps=30, seed=9700):
    """One stream of `steps` BGR pictures of noise with textured faces pasted in, the boxes a detector would report and the labelled
    identities.  Face 1 stays put on the left all the time.  kind "occlusion": face 2, on the right, is hidden for 12 steps (8 .. 19)
    and returns; "replaced": after the gap a DIFFERENT face 3 appears in its place.  Brightness drifts by a few levels over the clip and
    every reported box jitters by +- 1 pixel.  -> (pictures, boxes[t], truths[t])"""
    rng = np.random.default_rng(seed)
    tex = {k: texture(np.random.default_rng(seed + 10 * k), FACE, FACE) for k in (1, 2, 3)}
    places = {1: (20, 30), 2: (100, 40)}
    pictures, boxes, truths = [], [], []
    for t in range(steps):
        pic = noise(rng, CLIP_H, CLIP_W, 3)
        shown = [(1, 1)]
        if t < 8:
            shown.append((2, 2))
        elif t >= 20:
            shown.append((2, 2) if kind == "occlusion" else (3, 2))
        frame_boxes, frame_truth = [], []
        for face, place in shown:
            x, y = places[place]
            lit = np.clip(tex[face].astype(np.int32) + (t // 3 - 4), 0, 255).astype(np.uint8)
            pic[y:y + FACE, x:x + FACE] = lit
            jx, jy = (int(v) for v in rng.integers(-1, 2, 2))
            frame_boxes.append((x + jx, y + jy, x + jx + FACE - 1, y + jy + FACE - 1))
            frame_truth.append((face, x, y, x + FACE - 1, y + FACE - 1))
        pictures.append(pic)
        boxes.append(frame_boxes)
        truths.append(frame_truth)
    return pictures, boxes, truths


def host_chain(pictures, boxes, truths, reid_params, tracker=CLIP_TRACKER, score_iou=0.5):
    """one stream through the host builds: the tracker (yf_images_track_host), the descriptors of what it reports, the re-identification
    (reid_params None: left out) and the score -> (summary dict, the ids reported per step, the reid state or None)"""
    import score_support as sc
    steps, cap, out_cap = len(pictures), 4, 8
    dets, counts = ts.lay_out([[(b, None) for b in boxes]], cap, ts.TIME)
    tracked = ts.host_run(dets, counts, 1, steps, ts.TIME, cap, tracker, ts.empty_state(1), out_cap)
    info, state = tracked.info, None
    if reid_params is not None:
        batch = Batch("clip", "bgr", pictures, [[] for _ in pictures], None, out_cap)
        buf, descs, _, _ = pack(batch)
        lib = reid_host()
        desc, first, status = desc_sentinels(steps, out_cap)
        out = np.ascontiguousarray(tracked.out)
        assert lib.yfi_describe_records_host(buf.ctypes.data, buf.size, 0, descs.ctypes.data, out.ctypes.data, tracked.out_counts.ctypes.data, steps,
                                             out_cap, 0, 0, desc.ctypes.data, first.ctypes.data, status.ctypes.data) == steps
        r = host_run((tracked.info, tracked.out_counts, desc), 1, steps, ts.TIME, out_cap, reid_params, empty_state(1))
        info, state = r.info, r.state
    gt, gt_counts = sc.truth_arrays([truths], 4, ts.TIME)
    scored = sc.host_run((tracked.out, info, tracked.out_counts, gt, gt_counts), 1, steps, ts.TIME, 4, out_cap, score_iou, sc.empty_state(1))
    ids = [[int(info[t, k]["id"]) for k in range(int(tracked.out_counts[t]))] for t in range(steps)]
    return sc.host_summary(scored.state), ids, state, tracked
