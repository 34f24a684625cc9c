"""What the tests of the blur share (test_blur_*): the host build's prototypes and the expected buffer of a call -- `ptq.blur_u8` /
`ptq.blur_yuv420sp` on `ptq.crop_region`, the plain-numpy statement of csrc/yf_images_blur.h -- over the designed batches and layouts of
tests/redact_support.py, which is imported, not edited; the strips (pictures of 1 x W with the whole picture as the region) and the small
regions."""
import ctypes
import functools

import numpy as np

import crops_support as cs
import redact_support as rs

GRIDS = [1, 3, 8, 16]
FILL = rs.FILL
SENTINEL32 = rs.SENTINEL32
INVALID, FILLED = 1, 2                                         # the bits of d_status
STRIP_WIDTHS = list(range(1, 261)) + [16384]
DET = rs.DET
_mod = rs._mod


def workspace(records_cap, grid):
    """csrc/yf_images_blur.h: records_cap * grid * grid * 4 bytes rounded up to 16"""
    return (records_cap * grid * grid * 4 + 15) // 16 * 16


def aligned(nbytes, fill=0xA5):
    """a uint8 array of nbytes (at least 1) whose first byte is 16-byte aligned"""
    raw = np.full(max(nbytes, 1) + 16, fill, np.uint8)
    at = -raw.ctypes.data % 16
    return raw[at:at + max(nbytes, 1)]


def filled_slots(first, counts, cap, f, records_cap):
    """the slots of frame f whose record k = first[f] + s has no slot in the workspace"""
    return {s for s in range(cs.clamp(counts[f], cap)) if int(first[f]) + s >= records_cap}


def want_status(counts, cap, records_cap, invalid=()):
    first = rs.first_of(counts, cap)
    return [(INVALID if f in invalid else 0) | (FILLED if first[f + 1] > first[f] and first[f + 1] > records_cap else 0)
            for f in range(len(counts))]


def _records_cap(records_cap, counts, cap):
    return len(counts) * cap if records_cap is None else records_cap


def expected_packed(pictures, fmt, dets, counts, cap, grid, margin, square, records_cap=None, invalid=()):
    """the buffer `rs.lay_out_packed(pictures)` after the call, by the restatement; frames in `invalid` keep their pictures"""
    ptq = _mod("ptq")
    first, records_cap = rs.first_of(counts, cap), _records_cap(records_cap, counts, cap)
    out = []
    for f, p in enumerate(pictures):
        regions = [] if f in invalid else rs.regions_of(dets, counts, cap, f, p.shape[1], p.shape[0], margin, square)
        out.append(ptq.blur_u8(p, regions, grid, rs.fill_bytes(fmt), filled_slots(first, counts, cap, f, records_cap)))
    return rs.lay_out_packed(out)[0]


def expected_yuv(surfaces, fmt, dets, counts, cap, grid, margin, square, records_cap=None, invalid=()):
    from images_yuv_support import lay_out
    ptq = _mod("ptq")
    first, records_cap = rs.first_of(counts, cap), _records_cap(records_cap, counts, cap)
    out = []
    for f, (y, uv) in enumerate(surfaces):
        regions = [] if f in invalid else rs.regions_of(dets, counts, cap, f, y.shape[1], y.shape[0], margin, square)
        out.append(ptq.blur_yuv420sp(y, uv, regions, grid, (FILL >> 16 & 255, FILL >> 8 & 255, FILL & 255),
                                     filled_slots(first, counts, cap, f, records_cap), fmt == 5))
    return lay_out(out)[0]


@functools.lru_cache(maxsize=None)
def blur_host():
    """libyf_images_host.so with the prototypes of csrc/yf_images_blur.h's host build added"""
    lib = rs.redact_host()
    vp, ci, cl, cs_ = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_size_t
    for fn in (lib.yfi_blur_records_host, lib.yfi_blur_records_yuv_host):
        fn.restype = cl
        fn.argtypes = [vp, ctypes.c_uint64, ci, vp, vp, vp, cl, ci, ci, ctypes.c_uint32, ci, ci, vp, cs_, cl, vp, vp]
    lib.yfi_blur_workspace_host.restype = cs_
    lib.yfi_blur_workspace_host.argtypes = [cl, ci]
    lib.yfi_blur_check_host.restype = ci
    lib.yfi_blur_check_host.argtypes = [cl, ci, ci, ctypes.c_uint32, ci, ci, vp, cs_, cl, ctypes.c_char_p, ci]
    return lib


def host_check(n=4, cap=rs.CAP, grid=8, colour=0, margin=0, flags=0, work=16, work_bytes=1 << 30, records_cap=4):
    """yfi_blur_check -> the text of the first fault, '' for none (`work` is an address that is only looked at)"""
    text = ctypes.create_string_buffer(256)
    rc = blur_host().yfi_blur_check_host(n, cap, grid, colour, margin, flags, work, work_bytes, records_cap, text, 256)
    assert rc == (text.value != b"")
    return text.value.decode()


def host_blur(buf, fmt, desc, dets, counts, cap, grid, margin, square, records_cap=None, colour=FILL, nbytes=None, work_bytes=None):
    """the host build on a copy of `buf` with a workspace of exactly its size -> (rc, buffer, first int32 [n + 1], status int32 [n]);
    first and status start as 0xA5 bytes"""
    lib = blur_host()
    n = dets.shape[0]
    records_cap = _records_cap(records_cap, counts, cap)
    out = buf.copy()
    first = np.full(n + 1, SENTINEL32, np.int32)
    status = np.full(max(n, 1), SENTINEL32, np.int32)
    dets, counts, desc = np.ascontiguousarray(dets), np.ascontiguousarray(counts), np.ascontiguousarray(desc)
    room = int(lib.yfi_blur_workspace_host(records_cap, grid)) if work_bytes is None else work_bytes
    work = aligned(room)
    fn = lib.yfi_blur_records_yuv_host if fmt in (4, 5) else lib.yfi_blur_records_host
    rc = fn(out.ctypes.data, out.nbytes if nbytes is None else nbytes, fmt, desc.ctypes.data, dets.ctypes.data, counts.ctypes.data, n, cap,
            grid, colour, margin, int(square), work.ctypes.data, room, records_cap, first.ctypes.data, status.ctypes.data)
    return rc, out, first, status[:n]


# ---- the strips: pictures of 1 x W, the whole picture the region ----
@functools.lru_cache(maxsize=None)
def strips():
    """-> (buf, desc, pictures uint8 [1, W, 3], dets, counts): one frame per width of STRIP_WIDTHS, cap 1, in format 1 (RGB)"""
    rng = np.random.default_rng(6100)
    pictures = [rng.integers(0, 256, (1, w, 3), dtype=np.uint8) for w in STRIP_WIDTHS]
    buf, desc = rs.lay_out_packed(pictures)
    dets = np.zeros((len(pictures), 1), DET)
    for f, w in enumerate(STRIP_WIDTHS):
        dets[f, 0] = (f, 0, 0, 0, 0, 0.5, 0, 0, w - 1, 0)
    counts = np.ones(len(pictures), np.int32)
    for a in (buf, dets, counts):
        a.setflags(write=False)
    return buf, desc, pictures, dets, counts


@functools.lru_cache(maxsize=None)
def strips_expected(grid):
    _, _, pictures, dets, counts = strips()
    out = expected_packed(pictures, 1, dets, counts, 1, grid, 0, False)
    out.setflags(write=False)
    return out


# ---- small regions of one random picture ----
SMALL = [((3, 3), (1, 1)), ((4, 4), (1, 1)), ((7, 8), (1, 2)), ((16, 16), (4, 4)), ((33, 15), (8, 3))]      # (width, height) -> (gx, gy) at g = 8


@functools.lru_cache(maxsize=None)
def small_batch():
    """one frame per region of SMALL on a random 40 x 40 picture, the region at (2, 3) -> (buf, desc, pictures, dets, counts), format 0"""
    pictures = [np.random.default_rng(6200 + f).integers(0, 256, (40, 40, 3), dtype=np.uint8) for f in range(len(SMALL))]
    buf, desc = rs.lay_out_packed(pictures)
    dets = np.zeros((len(SMALL), 1), DET)
    for f, ((w, h), _) in enumerate(SMALL):
        dets[f, 0] = (f, 0, 0, 0, 0, 0.5, 2, 3, 2 + w - 1, 3 + h - 1)
    return buf, desc, pictures, dets, np.ones(len(SMALL), np.int32)


# ---- one frame of pairwise disjoint records ----
@functools.lru_cache(maxsize=None)
def disjoint_batch():
    """the 64 x 48 picture with twelve records on a 4 x 3 lattice of 16 x 16 tiles, each inside its tile -> (buf, desc, pictures, dets, counts)"""
    rng = np.random.default_rng(6300)
    boxes = []
    for ty in range(3):
        for tx in range(4):
            x1, y1 = 16 * tx + int(rng.integers(0, 5)), 16 * ty + int(rng.integers(0, 5))
            boxes.append((x1, y1, int(rng.integers(x1, 16 * tx + 16)), int(rng.integers(y1, 16 * ty + 16))))
    dets, counts = rs.records([(boxes, len(boxes))])
    pictures = [cs.in_format(rs.picture(1), 3)]
    buf, desc = rs.lay_out_packed(pictures)
    return buf, desc, pictures, dets, counts


def big_surface():
    """one NV12 surface of 4128 x 4096 (W x H), every Y byte 255 and the chroma a constant pair, the whole surface one record ->
    (buf, desc, dets, counts): a Y sum of 4 311 613 440, above 2^32"""
    images = _mod("images")
    w, h = 4128, 4096
    buf = np.empty(w * h * 3 // 2, np.uint8)
    buf[:w * h] = 255
    buf[w * h:] = 77
    desc = np.zeros(1, images.YUV_IMAGE_DTYPE)
    desc[0] = (0, w * h, h, w, w, w)
    dets = np.zeros((1, 1), DET)
    dets[0, 0] = (0, 0, 0, 0, 0, 0.5, 0, 0, w - 1, h - 1)
    return buf, desc, dets, np.ones(1, np.int32)
