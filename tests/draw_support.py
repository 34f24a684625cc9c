"""What the tests of the drawing share (test_draw_*): the designed batches of small pictures, laid out with padded rows and odd offsets in
a buffer whose every other byte is a filler, the keys and palettes, the host build's prototypes, and the expected buffer of a call --
`ptq.draw_rectangles_u8` / `ptq.draw_rectangles_yuv420sp`, the plain-numpy statement of csrc/yf_images_draw.h, laid out the same way.

The records depend on `half` = h (a box at distance exactly h from the picture reaches in, one at h + 1 does not), so a batch is built
per h.  Per picture of W x H, `designed_boxes`: a box inside; a box on each border; edges beyond each side; boxes wholly outside at
distance h and h + 1 on every side; x1 > x2 and y1 > y2; a point, a horizontal and a vertical line; a box of inner size below 2h + 1;
INT32_MIN / INT32_MAX edges; boxes with odd and with even origins (on a surface their chroma pairs are shared between a drawn and an
undrawn pixel); and pairs that cross, coincide and contain each other, whose keys differ.

The packed batch, cap 48 (W x H): frame 0 1 x 1, frame 1 2 x 7, frame 2 an INVALID descriptor (its stride is below its row), frame 3
23 x 37, frame 4 64 x 48, frame 5 64 x 48 with a count above cap (all 48 records exist, seeded), frame 6 23 x 37 with a negative count
over slots that hold records.  The surfaces: 2 x 2, 22 x 34, an invalid one (odd height), 48 x 64, 48 x 64 with a count above cap,
22 x 34 with count 0.  Every frame has a picture of its own: with keys, pictures must not share bytes."""
import ctypes
import functools

import numpy as np

import crops_support as cs
import redact_support as rs
from images_support import host_lib
from images_yuv_support import lay_out

I32_MIN, I32_MAX = cs.I32_MIN, cs.I32_MAX
CAP = 48
PACKED = [(1, 1), (2, 7), (23, 37), (23, 37), (64, 48), (64, 48), (23, 37)]          # (W, H) of each frame's own picture
PACKED_INVALID = 2
SURFACES = [(2, 2), (22, 34), (22, 34), (48, 64), (48, 64), (22, 34)]
SURFACES_INVALID = 2
HALVES = [0, 1, 2, 3]
COLOUR = 0x00C82D5A                                                                   # R 200, G 45, B 90; Y 200, U 45, V 90
GAP = rs.GAP
SENTINEL32 = rs.SENTINEL32
DET = cs.DET
_mod = cs._mod


def designed_boxes(w, h, half):
    k = half
    return [
        (w // 4, h // 4, 3 * w // 4, 3 * h // 4),                                     # inside
        (0, 0, w - 1, h - 1),                                                         # on each border
        (-5, h // 3, w + 4, 2 * h // 3), (w // 3, -6, 2 * w // 3, h + 7), (-4, -4, w // 2, h // 2),      # beyond the sides
        (-k - 4, 2, -k, h - 3), (-k - 5, 1, -k - 1, h - 2),                           # left of the picture at distance h, and at h + 1
        (w - 1 + k, 1, w + 5 + k, h - 2), (w + k, 2, w + 6 + k, h - 3),               # right
        (1, -k - 3, w - 2, -k), (2, -k - 4, w - 3, -k - 1),                           # above
        (2, h - 1 + k, w - 3, h + 4 + k), (1, h + k, w - 2, h + 5 + k),               # below
        (2 * w // 3, h // 4, w // 3, h // 2), (w // 4, 2 * h // 3, w // 2, h // 3),   # x1 > x2, y1 > y2
        (w // 2, h // 2, w // 2, h // 2), (1, h // 2 + 2, w - 2, h // 2 + 2), (w // 2 + 1, 1, w // 2 + 1, h - 2),      # point, lines
        (w // 3, h // 3, w // 3 + k, h // 3 + 2 * k),                                 # thinner than 2h + 1 (one way for h >= 1)
        (I32_MIN, I32_MIN, I32_MAX, I32_MAX), (I32_MIN, h // 4, w // 2, I32_MAX),
        (1, 1, 6, 6), (2, 2, 7, 7), (3, 4, 8, 9),                                     # odd and even origins
        (2, h // 2 - 3, w - 3, h // 2 + 3), (w // 2 - 3, 2, w // 2 + 3, h - 3),       # two that cross
        (w // 5, h // 5, w // 5 + 9, h // 5 + 9), (w // 5, h // 5, w // 5 + 9, h // 5 + 9),              # two that coincide
        (5, 5, 20, 20), (6, 6, 19, 19),                                               # one that contains the next
    ]


def seeded_boxes(w, h, count, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        x1, y1 = int(rng.integers(-6, w + 3)), int(rng.integers(-6, h + 3))
        out.append((x1, y1, x1 + int(rng.integers(-3, w)), y1 + int(rng.integers(-3, h))))
    return out


def _records(frames, cap):
    """[(boxes, count)] per frame -> (dets DET [n, cap], counts int32 [n]); slots that hold no record are 0xA5 bytes"""
    n = len(frames)
    dets = np.frombuffer(bytes([0xA5]) * (n * cap * 28), DET).reshape(n, cap).copy()
    counts = np.zeros(n, np.int32)
    for f, (boxes, count) in enumerate(frames):
        counts[f] = count
        for s, box in enumerate(boxes):
            dets[f, s] = (f, s % 3, 1, 2, 5, 0.75, *box)
    dets.setflags(write=False)
    counts.setflags(write=False)
    return dets, counts


@functools.lru_cache(maxsize=None)
def packed_records(half):
    """-> (dets DET [7, CAP], counts int32 [7])"""
    frames = []
    for f, (w, h) in enumerate(PACKED):
        boxes = designed_boxes(w, h, half)
        assert len(boxes) <= CAP
        if f == 5:
            frames.append((seeded_boxes(w, h, CAP, 6100 + half), CAP + 50))
        elif f == 6:
            frames.append((boxes, -3))
        else:
            frames.append((boxes, len(boxes)))
    return _records(frames, CAP)


@functools.lru_cache(maxsize=None)
def surface_records(half):
    frames = []
    for f, (w, h) in enumerate(SURFACES):
        boxes = designed_boxes(w, h, half)
        if f == 4:
            frames.append((seeded_boxes(w, h, CAP, 6200 + half), CAP + 7))
        elif f == 5:
            frames.append((boxes, 0))
        else:
            frames.append((boxes, len(boxes)))
    return _records(frames, CAP)


@functools.lru_cache(maxsize=None)
def _rgb(f):
    w, h = PACKED[f]
    img = np.random.default_rng(6000 + f).integers(0, 256, (h, w, 3), dtype=np.uint8)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def packed_batch(fmt):
    """the packed pictures in format `fmt`, laid out with padded rows and odd gaps -> (buf, desc with frame PACKED_INVALID made invalid,
    pictures); the buffer ends with its last picture"""
    pictures = [cs.in_format(_rgb(f), fmt) for f in range(len(PACKED))]
    buf, desc = rs.lay_out_packed(pictures)
    desc["row_stride"][PACKED_INVALID] = PACKED[PACKED_INVALID][0] * pictures[0].shape[2] - 1
    buf.setflags(write=False)
    return buf, desc, pictures


@functools.lru_cache(maxsize=None)
def surface_batch():
    """-> (buf, desc with surface SURFACES_INVALID made invalid, surfaces [(y, uv)])"""
    surfaces = []
    for f, (w, h) in enumerate(SURFACES):
        rng = np.random.default_rng(6050 + f)
        surfaces.append((rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w), dtype=np.uint8)))
    buf, desc = lay_out(surfaces)
    desc["height"][SURFACES_INVALID] += 1
    buf.setflags(write=False)
    return buf, desc, surfaces


# ---- keys and palettes ----
def keys_for(n, cap, stride, seed=0):
    """a key per slot, neighbours different, many above every palette size -> uint32 [n, cap, stride / 4] whose column 0 holds the keys
    and whose other columns hold 0xA5 bytes (the other fields of a wider row)"""
    s = np.arange(n * cap, dtype=np.uint64).reshape(n, cap)
    key = ((s * 2654435761 + 977 * (seed + 1)) % (1 << 32)).astype(np.uint32)
    key[:, ::5] = key[:, ::5] % 7                                                     # some small ones too
    rows = np.full((n, cap, stride // 4), 0xA5A5A5A5, np.uint32)
    rows[..., 0] = key
    return rows


def palette(count):
    """`count` colours 0x00RRGGBB, every third entry with a top byte that must be ignored"""
    rng = np.random.default_rng(6300 + count)
    p = rng.integers(0, 1 << 24, count, dtype=np.uint32)
    p[::3] |= np.uint32(0xAB000000)
    return p


KEYED = [(4, 3), (16, 256), (4, 1), (16, 3)]                                          # (key_stride, palette_n), one per half


def colours_of(fmt, keys, pal, f, m, colour=COLOUR):
    """the colour triples of the first m records of frame f as `ptq` takes them: in the byte order of packed format `fmt`, (Y, U, V) for
    surfaces; keys None: the one colour"""
    if keys is None:
        codes = [colour] * m
    else:
        codes = [int(pal[int(keys[f, s, 0]) % len(pal)]) & 0xFFFFFF for s in range(m)]
    triples = [(c >> 16 & 255, c >> 8 & 255, c & 255) for c in codes]
    return [t[::-1] if fmt in (0, 2) else t for t in triples]


def _boxes(dets, f, m):
    return [(int(d["x1"]), int(d["y1"]), int(d["x2"]), int(d["y2"])) for d in dets[f, :m]]


def expected_packed(pictures, fmt, dets, counts, cap, half, keys=None, pal=None, invalid=(PACKED_INVALID,)):
    """the buffer `lay_out_packed(pictures)` after the call, by the restatement; frames in `invalid` keep their pictures"""
    ptq = _mod("ptq")
    out = []
    for f, p in enumerate(pictures):
        m = 0 if f in invalid else cs.clamp(counts[f], cap)
        out.append(ptq.draw_rectangles_u8(p, _boxes(dets, f, m), half, colours_of(fmt, keys, pal, f, m)) if m else p)
    return rs.lay_out_packed(out)[0]


def expected_surfaces(surfaces, fmt, dets, counts, cap, half, keys=None, pal=None, invalid=(SURFACES_INVALID,)):
    ptq = _mod("ptq")
    out = []
    for f, (y, uv) in enumerate(surfaces):
        m = 0 if f in invalid else cs.clamp(counts[f], cap)
        out.append(ptq.draw_rectangles_yuv420sp(y, uv, _boxes(dets, f, m), half, colours_of(4, keys, pal, f, m), fmt == 5) if m else (y, uv))
    return lay_out(out)[0]


def batch_of(fmt, half):
    """-> (buf, desc, pictures or surfaces, dets, counts) of the designed batch of format `fmt` at `half`"""
    if fmt in (4, 5):
        return surface_batch() + surface_records(half)
    return packed_batch(fmt) + packed_records(half)


def expected(fmt, half, keys=None, pal=None):
    buf, desc, pictures, dets, counts = batch_of(fmt, half)
    fn = expected_surfaces if fmt in (4, 5) else expected_packed
    return fn(pictures, fmt, dets, counts, CAP, half, keys, pal)


@functools.lru_cache(maxsize=None)
def capacity_batch():
    """one frame, cap 1200, 1200 seeded records with keys on a 64 x 48 picture: the first slot's list of later owners is full"""
    dets = np.zeros((1, 1200), DET)
    for s, box in enumerate(seeded_boxes(64, 48, 1200, 6400)):
        dets[0, s] = (0, 0, 0, 0, 0, 0.5, *box)
    dets.setflags(write=False)
    return dets, np.array([1200], np.int32)


# ---- the host build ----
@functools.lru_cache(maxsize=None)
def draw_host():
    """libyf_images_host.so with the prototypes of csrc/yf_images_draw.h's host build added"""
    lib = host_lib()
    vp, ci, cl, u32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_uint32
    for fn in (lib.yfi_draw_records_host, lib.yfi_draw_records_yuv_host):
        fn.restype = cl
        fn.argtypes = [vp, ctypes.c_uint64, ci, vp, vp, vp, cl, ci, ci, u32, vp, ci, vp, ci, vp, vp]
    lib.yfi_draw_check_host.restype = ci
    lib.yfi_draw_check_host.argtypes = [cl, ci, ci, u32, vp, ci, vp, ci, ctypes.c_char_p, ci]
    lib.yfi_draw_masks_host.restype = None
    lib.yfi_draw_masks_host.argtypes = [vp, cl, ci, ctypes.c_int32, ctypes.c_int32, vp]
    lib.yfi_draw_bands_host.restype = None
    lib.yfi_draw_bands_host.argtypes = [vp, cl, ci, ctypes.c_int32, ctypes.c_int32, vp]
    return lib


def host_check(n=4, cap=CAP, half=1, colour=0, keys=None, key_stride=0, palette=None, palette_n=0):
    """yfi_draw_check -> the text of the first fault, '' for none; keys and palette are addresses (or None)"""
    text = ctypes.create_string_buffer(256)
    rc = draw_host().yfi_draw_check_host(n, cap, half, colour, keys, key_stride, palette, palette_n, text, 256)
    assert rc == (text.value != b"")
    return text.value.decode()


def host_draw(buf, fmt, desc, dets, counts, cap, half, colour=COLOUR, keys=None, pal=None, nbytes=None):
    """the host build on a copy of `buf` -> (rc, buffer, first int32 [n + 1], status int32 [n]); first and status start as 0xA5 bytes.
    keys: uint32 [n, cap, stride / 4] as `keys_for` gives them, pal: uint32 [palette_n]; None: the one colour"""
    lib = draw_host()
    n = dets.shape[0]
    out = buf.copy()
    first = np.full(n + 1, SENTINEL32, np.int32)
    status = np.full(max(n, 1), SENTINEL32, np.int32)
    dets, counts, desc = np.ascontiguousarray(dets), np.ascontiguousarray(counts), np.ascontiguousarray(desc)
    fn = lib.yfi_draw_records_yuv_host if fmt in (4, 5) else lib.yfi_draw_records_host
    if keys is None:
        kp, stride, pp, pn, colour = None, 0, None, 0, colour
    else:
        keys, pal = np.ascontiguousarray(keys), np.ascontiguousarray(pal)
        kp, stride, pp, pn, colour = keys.ctypes.data, keys.shape[2] * 4, pal.ctypes.data, pal.shape[0], 0
    rc = fn(out.ctypes.data, out.nbytes if nbytes is None else nbytes, fmt, desc.ctypes.data, dets.ctypes.data, counts.ctypes.data, n, cap,
            half, colour, kp, stride, pp, pn, first.ctypes.data, status.ctypes.data)
    return rc, out, first, status[:n]


def host_masks(boxes, half, w, h):
    """yfi_draw_covers for every pixel of a w x h picture and every box of int32 [n, 4] -> bool [n, h, w]"""
    boxes = np.ascontiguousarray(boxes, np.int32)
    out = np.full((boxes.shape[0], h, w), 7, np.uint8)
    draw_host().yfi_draw_masks_host(boxes.ctypes.data, boxes.shape[0], half, w, h, out.ctypes.data)
    assert out.max(initial=0) <= 1
    return out.astype(bool)


def host_bands(boxes, half, w, h):
    """yfi_draw_bands_of per box -> int32 [n, 14]: (at, n) of top, bottom, between, across, left, right; yfi_draw_visible; 0"""
    boxes = np.ascontiguousarray(boxes, np.int32)
    out = np.full((boxes.shape[0], 14), -99, np.int32)
    draw_host().yfi_draw_bands_host(boxes.ctypes.data, boxes.shape[0], half, w, h, out.ctypes.data)
    return out


def status_of(n, invalid):
    return [1 if f == invalid else 0 for f in range(n)]
