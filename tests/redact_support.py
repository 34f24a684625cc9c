"""What the tests of the redaction share (test_redact_*): the designed batches, laid out with padded rows and odd gaps in a buffer whose
every other byte is a sentinel, the host build's prototypes, and the expected buffer of a call -- `ptq.redact_u8` / `ptq.redact_yuv420sp`
on `ptq.crop_region`, the plain-Python statement of csrc/yf_images_redact.h, laid out the same way.

The mosaic must not be given pictures that share bytes, so `crops_support.designed_batch` (whose frames share pictures) is not reused:
here every frame has a picture of its own.  The designed batch, cap 80:
  frame 0, 37 x 53: the 13 boxes of `crops_support.designed_boxes` (overhang on every side, empty, inverted, int32 extremes)
  frame 1, 64 x 48: 70 records that all touch the same blocks, so that the kernel's list of earlier owners passes a wave's width
  frame 2, 1 x 1: the 13 designed boxes
  frame 3, 410 x 362: the overlap set, then seeded boxes; its count is above cap (all 80 records exist)
  frame 4, 64 x 48 (a copy of frame 1's picture): the overlap set alone, so that most of the picture lies outside the redacted set
  frame 5, 37 x 53 and frame 6, 64 x 48: counts 0 and -3 over slots that hold records; their pictures must stay as they are
The overlap set: two records sharing blocks; a record inside another, the inner one first; the same record twice; a chain A, B, C with
A and B, B and C overlapping and A and C apart."""
import ctypes
import functools

import numpy as np

import crops_support as cs
from images_support import host_lib

PICTURES = [(37, 53), (64, 48), (1, 1), (410, 362), (64, 48), (37, 53), (64, 48)]       # (W, H) of each frame's own picture
SEED_OF = [0, 1, 2, 3, 1, 0, 1]                                                          # frame 4 copies frame 1's picture, ...
CAP = 80
BLOCKS = [4, 8, 64]
GRID = cs.GRID                                                                           # (margin_permille, square)
FILL = 0x00C82D5A                                                                        # R 200, G 45, B 90; Y 200, U 45, V 90
GAP = 0x5B
SENTINEL32 = -1515870811                                                                 # 0xA5A5A5A5
MOSAIC, FILLED = 0, 1
DET = cs.DET
_mod = cs._mod


def overlap_set(w, h):
    ox, oy = w // 4, h // 4
    return [
        (ox, oy, ox + 9, oy + 9), (ox + 6, oy + 6, ox + 14, oy + 14),                    # two records sharing blocks
        (w // 2 + 4, oy + 4, w // 2 + 6, oy + 6), (w // 2, oy, w // 2 + 12, oy + 12),    # one inside another, the inner one first
        (3, h - 12, 10, h - 5), (3, h - 12, 10, h - 5),                                  # the same record twice
        (ox, h // 2 + 2, ox + 8, h // 2 + 8), (ox + 7, h // 2 + 2, ox + 15, h // 2 + 8), (ox + 14, h // 2 + 2, ox + 22, h // 2 + 8),
    ]


def crowd(n):
    """n records of the 64 x 48 picture that all hold pixel (24, 20), each with edges of its own"""
    return [(24 - s % 7, 20 - s % 5, 24 + s % 11, 20 + s % 3 + s // 35) for s in range(n)]


def records(frames):
    """[(boxes, count)] per frame -> (dets DET [n, cap], counts int32 [n]); slots that hold no record are 0xA5 bytes"""
    n = len(frames)
    cap = max(CAP, max(len(b) for b, _ in frames)) if frames else CAP
    dets = np.frombuffer(bytes([0xA5]) * (n * cap * 28), DET).reshape(n, cap).copy()
    counts = np.zeros(n, np.int32)
    for f, (boxes, count) in enumerate(frames):
        counts[f] = count
        for s, box in enumerate(boxes):
            dets[f, s] = (f, s % 3, 1, 2, 5, 0.75, *box)
    return dets, counts


@functools.lru_cache(maxsize=None)
def designed():
    rng = np.random.default_rng(5300)
    w3, h3 = PICTURES[3]
    seeded = overlap_set(w3, h3)
    while len(seeded) < CAP:
        x1, y1 = int(rng.integers(-6, w3)), int(rng.integers(-6, h3))
        seeded.append((x1, y1, x1 + int(rng.integers(0, 60)), y1 + int(rng.integers(0, 60))))
    frames = [(cs.designed_boxes(37, 53), 13), (crowd(70), 70), (cs.designed_boxes(1, 1), 13), (seeded, CAP + 84),
              (overlap_set(64, 48), 9), (cs.designed_boxes(37, 53), 0), (overlap_set(64, 48), -3)]
    dets, counts = records(frames)
    dets.setflags(write=False)
    counts.setflags(write=False)
    return dets, counts


@functools.lru_cache(maxsize=None)
def picture(f):
    """frame f's picture, uint8 [H, W, 3] in RGB order, read-only"""
    w, h = PICTURES[f]
    img = np.random.default_rng(5200 + SEED_OF[f]).integers(0, 256, (h, w, 3), dtype=np.uint8)
    img.setflags(write=False)
    return img


def lay_out_packed(pictures, pad=5):
    """pictures uint8 [H, W, C] -> (buffer, IMAGE_DTYPE descriptors): rows pad bytes longer than their pixels, gaps of odd sizes in front
    of every picture, nothing aligned, every byte that is no pixel equal to GAP, and the last picture ends with the buffer"""
    images = _mod("images")
    desc = np.zeros(len(pictures), images.IMAGE_DTYPE)
    off, parts = 3, []
    for i, p in enumerate(pictures):
        h, w, C = p.shape
        rs = w * C + pad
        desc[i] = (off, h, w, rs)
        parts.append((off, rs, p))
        off += (h - 1) * rs + w * C + 7 + 2 * (i % 3)
    last = max(o + (p.shape[0] - 1) * rs + p.shape[1] * p.shape[2] for o, rs, p in parts)
    buf = np.full(last, GAP, np.uint8)
    for o, rs, p in parts:
        h, w, C = p.shape
        np.lib.stride_tricks.as_strided(buf[o:], shape=(h, w * C), strides=(rs, 1))[:] = p.reshape(h, w * C)
    return buf, desc


def fill_bytes(fmt, colour=FILL):
    """the colour's three bytes in the order format `fmt` keeps them: what `ptq.redact_u8` takes"""
    rgb = (colour >> 16 & 255, colour >> 8 & 255, colour & 255)
    return rgb[::-1] if fmt in (0, 2) else rgb


def regions_of(dets, counts, cap, f, w, h, margin, square):
    ptq = _mod("ptq")
    return [ptq.crop_region((d["x1"], d["y1"], d["x2"], d["y2"]), w, h, margin, square) for d in dets[f, :cs.clamp(counts[f], cap)]]


def first_of(counts, cap):
    return np.concatenate([[0], np.cumsum([cs.clamp(c, cap) for c in counts])]).astype(np.int32)


def packed_batch(fmt, frames=None):
    """the designed batch (or the frames given, a list of frame indices) in packed format `fmt` -> (buf, desc, pictures)"""
    frames = range(len(PICTURES)) if frames is None else frames
    pictures = [cs.in_format(picture(f), fmt) for f in frames]
    buf, desc = lay_out_packed(pictures)
    return buf, desc, pictures


def expected_packed(pictures, fmt, dets, counts, cap, mode, block, margin, square, invalid=()):
    """the buffer `lay_out_packed(pictures)` after the call, by the restatement; frames in `invalid` keep their pictures"""
    ptq = _mod("ptq")
    out = []
    for f, p in enumerate(pictures):
        regions = [] if f in invalid else regions_of(dets, counts, cap, f, p.shape[1], p.shape[0], margin, square)
        out.append(ptq.redact_u8(p, regions, "mosaic" if mode == MOSAIC else "fill", block, fill_bytes(fmt)))
    return lay_out_packed(out)[0]


YUV_SHAPES = [3, 4, 8, 0]                   # images_yuv_support.SHAPES: 6 x 10, 54 x 58, 362 x 410, 2 x 2 (h x w)
YUV_CAP = 32


@functools.lru_cache(maxsize=None)
def yuv_batch():
    """surfaces laid out with odd pitches and UV before Y (images_yuv_support.lay_out); per surface the designed boxes, boxes with odd
    origins and odd sides, and the overlap set -> (buf, desc, surfaces, dets, counts)"""
    from images_yuv_support import lay_out, surface
    surfaces = [surface(k, False) for k in YUV_SHAPES]
    buf, desc = lay_out(surfaces)
    frames = []
    for i, (y, _) in enumerate(surfaces):
        h, w = y.shape
        designed = cs.designed_boxes(w, h)
        if i == 1:                                              # 54 x 58: no box holds the whole surface, most of it stays as it is
            designed = designed[2:8]
        boxes = designed + [(3, 1, 7, 7), (w - 3, h - 5, w - 1, h - 1)] + ([] if i == 1 else [(1, 1, w - 2, h - 2)]) + overlap_set(w, h)
        frames.append((boxes, len(boxes)))
    dets, counts = records(frames)
    dets = np.ascontiguousarray(dets[:, :YUV_CAP])
    for a in (buf, dets, counts):
        a.setflags(write=False)
    return buf, desc, surfaces, dets, counts


def expected_yuv(surfaces, fmt, dets, counts, cap, mode, block, margin, square, invalid=()):
    from images_yuv_support import lay_out
    ptq = _mod("ptq")
    out = []
    for f, (y, uv) in enumerate(surfaces):
        regions = [] if f in invalid else regions_of(dets, counts, cap, f, y.shape[1], y.shape[0], margin, square)
        out.append(ptq.redact_yuv420sp(y, uv, regions, "mosaic" if mode == MOSAIC else "fill", block,
                                       (FILL >> 16 & 255, FILL >> 8 & 255, FILL & 255), fmt == 5))
    return lay_out(out)[0]


@functools.lru_cache(maxsize=None)
def redact_host():
    """libyf_images_host.so with the prototypes of csrc/yf_images_redact.h's host build added"""
    lib = host_lib()
    vp, ci, cl = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    for fn in (lib.yfi_redact_records_host, lib.yfi_redact_records_yuv_host):
        fn.restype = cl
        fn.argtypes = [vp, ctypes.c_uint64, ci, vp, vp, vp, cl, ci, ci, ci, ctypes.c_uint32, ci, ci, vp, vp]
    lib.yfi_redact_check_host.restype = ci
    lib.yfi_redact_check_host.argtypes = [cl, ci, ci, ci, ctypes.c_uint32, ci, ci, ctypes.c_char_p, ci]
    return lib


def host_check(n=4, cap=CAP, mode=MOSAIC, block=8, colour=0, margin=0, flags=0):
    """yfi_redact_check -> the text of the first fault, '' for none"""
    text = ctypes.create_string_buffer(256)
    rc = redact_host().yfi_redact_check_host(n, cap, mode, block, colour, margin, flags, text, 256)
    assert rc == (text.value != b"")
    return text.value.decode()


def host_redact(buf, fmt, desc, dets, counts, cap, mode, block, margin, square, colour=FILL, nbytes=None):
    """the host build on a copy of `buf` -> (rc, buffer, first int32 [n + 1], status int32 [n]); first and status start as 0xA5 bytes"""
    lib = redact_host()
    n = dets.shape[0]
    out = buf.copy()
    first = np.full(n + 1, SENTINEL32, np.int32)
    status = np.full(max(n, 1), SENTINEL32, np.int32)
    dets, counts, desc = np.ascontiguousarray(dets), np.ascontiguousarray(counts), np.ascontiguousarray(desc)
    fn = lib.yfi_redact_records_yuv_host if fmt in (4, 5) else lib.yfi_redact_records_host
    rc = fn(out.ctypes.data, out.nbytes if nbytes is None else nbytes, fmt, desc.ctypes.data, dets.ctypes.data, counts.ctypes.data, n, cap,
            mode, block if mode == MOSAIC else 0, colour, margin, int(square), first.ctypes.data, status.ctypes.data)
    return rc, out, first, status[:n]


def cases():
    """(mode, block, margin_permille, square) of the grid: the mosaic at every block size, and the fill"""
    return [(MOSAIC, k, m, s) for k in BLOCKS for m, s in GRID] + [(FILLED, 0, m, s) for m, s in GRID]


@functools.lru_cache(maxsize=None)
def capacity_batch():
    """one frame, cap 1200, 1200 records on the 37 x 53 picture: the last slot's list of earlier owners reaches its capacity (every
    record holds pixel (18, 26), so every earlier record meets every later one)"""
    rng = np.random.default_rng(5400)
    boxes = [(18 - int(rng.integers(0, 19)), 26 - int(rng.integers(0, 27)), 18 + int(rng.integers(0, 3)), 26 + int(rng.integers(0, 3)))
             for _ in range(1200)]
    boxes.sort(key=lambda b: (b[2] - b[0]) * (b[3] - b[1]))     # small records first: the later ones own what the earlier ones left
    dets = np.zeros((1, 1200), DET)
    for s, box in enumerate(boxes):
        dets[0, s] = (0, 0, 0, 0, 0, 0.5, *box)
    dets.setflags(write=False)
    return dets, np.array([1200], np.int32)
