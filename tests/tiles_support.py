"""What the tests of the tiled detection share (test_tiles_host, test_tiles_gpu): the project's own statement, in plain Python, of the
tile grid, of the translation of a tile's record to its image's pixels and of the merge (csrc/yf_images_tiles.h -- the reference has no
tiling, this is the library's definition), the prototypes of the host build, and the builders of seeded records."""
import ctypes

import numpy as np

from images_support import host_lib

TILE = np.dtype([("image", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("height", "<i4"), ("width", "<i4")])
IMAGE = np.dtype([("offset", "<u8"), ("height", "<i4"), ("width", "<i4"), ("row_stride", "<i8")])
DET = np.dtype([("frame", "<i4"), ("anchor", "u1"), ("row", "u1"), ("col", "u1"), ("q_conf", "i1"), ("conf", "<f4"),
                ("x1", "<i4"), ("y1", "<i4"), ("x2", "<i4"), ("y2", "<i4")])
CHANNELS = {0: 3, 1: 3, 2: 4, 3: 4}
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
assert TILE.itemsize == 20 and IMAGE.itemsize == 24 and DET.itemsize == 28


# ---- the statement ----
def axis_tiles(L, T, S):
    """(origin, side) of every tile along an axis of length L: tile side T >= 1, stride 1 <= S <= T"""
    if L <= T:
        return [(0, L)]
    k = (L - T + S - 1) // S + 1
    return [(i * S, T) for i in range(k - 1)] + [(L - T, T)]


def image_tiles(H, W, th, tw, sy, sx, whole):
    """(x0, y0, height, width) of an image's tiles: row-major, y outer; the whole image first when the grid has more than one tile"""
    grid = [(x0, y0, h, w) for y0, h in axis_tiles(H, th, sy) for x0, w in axis_tiles(W, tw, sx)]
    return ([(0, 0, H, W)] if whole and len(grid) > 1 else []) + grid


def plan_restated(parents, fmt, th, tw, sy, sx, whole):
    """parents IMAGE[n] -> (tiles TILE[t], tile descriptors IMAGE[t], first int32[n + 1])"""
    C = CHANNELS[fmt]
    tiles, desc, first = [], [], [0]
    for i, p in enumerate(parents):
        for x0, y0, h, w in image_tiles(int(p["height"]), int(p["width"]), th, tw, sy, sx, whole):
            tiles.append((i, x0, y0, h, w))
            desc.append((int(p["offset"]) + y0 * int(p["row_stride"]) + x0 * C, h, w, int(p["row_stride"])))
        first.append(len(tiles))
    return np.array(tiles, TILE).reshape(-1), np.array(desc, IMAGE).reshape(-1), np.array(first, np.int32)


def clamp(count, cap):
    return min(max(int(count), 0), cap)


def shift(edge, origin):
    """an edge moved by an origin: the exact sum, clamped to int32"""
    return min(max(int(edge) + int(origin), I32_MIN), I32_MAX)


def translate(recs, image, x0, y0):
    """DET records of a tile at (x0, y0) as image `image` holds them: `shift` on every edge (int64 sums, clamped), frame = image"""
    out = recs.copy()
    out["frame"] = image
    for name, origin in (("x1", x0), ("x2", x0), ("y1", y0), ("y2", y0)):
        out[name] = np.clip(recs[name].astype(np.int64) + int(origin), I32_MIN, I32_MAX)
    return out


def merge_restated(dets, counts, cap, tiles, first):
    """dets DET[t, cap], counts[t], tiles TILE[t], first[n + 1] (well formed) -> per image the DET array of its merged records (all of
    them: the caller cuts at out_cap)"""
    out = []
    for i in range(len(first) - 1):
        rows = [translate(dets[j, :clamp(counts[j], cap)], i, tiles["x0"][j], tiles["y0"][j]) for j in range(int(first[i]), int(first[i + 1]))]
        out.append(np.concatenate(rows + [np.zeros(0, DET)]))
    return out


def expect_gather(dets, counts, cap, tiles, first, out_cap, fill=0xA5):
    """-> (bytes uint8[n, out_cap, 28] with `fill` in every slot that is not written, totals int32[n])"""
    merged = merge_restated(dets, counts, cap, tiles, first)
    n = len(merged)
    raw = np.full((n, out_cap, 28), fill, np.uint8)
    for i, m in enumerate(merged):
        k = min(m.shape[0], out_cap)
        raw[i, :k] = m[:k].view(np.uint8).reshape(k, 28)
    return raw, np.array([m.shape[0] for m in merged], np.int32)


# ---- seeded records: the batch of the issue's count and edge cases ----
TILES_PER_IMAGE = [0, 1, 63, 64, 65, 255, 256, 257, 1000, 0, 3]          # the scan's wave and chunk edges; empty images between others


def seeded_tiles(rng, cap, per_image=TILES_PER_IMAGE):
    """-> (dets DET[t, cap], counts int32[t], tiles TILE[t], first int32[n + 1]).  Most tiles hold few records or none; some hold exactly
    cap, more than cap, a negative count, INT32_MIN.  Edges are random with INT32_MIN, INT32_MAX and INT32_MAX - 5 among them; origins are
    random in [0, 16383], every seventh tile at x0 = 16383."""
    first = np.concatenate([[0], np.cumsum(per_image)]).astype(np.int32)
    t = int(first[-1])
    tiles = np.zeros(t, TILE)
    tiles["image"] = -5                                   # never read: membership comes from `first`
    tiles["x0"], tiles["y0"] = rng.integers(0, 16384, t), rng.integers(0, 16384, t)
    tiles["x0"][::7] = 16383
    tiles["height"], tiles["width"] = 1, 1
    pool = [0, 0, 0, 0, 1, 2, min(3, cap), cap, cap + 1, cap + 40, -1, -3, I32_MIN, I32_MAX, max(cap // 2, 1), max(cap - 1, 0)]
    counts = rng.choice(np.array(pool, np.int64), t).astype(np.int32)
    if per_image[-1] == 3:
        counts[-3:] = [min(2, cap), min(3, cap), 1]           # the image `cuts` cuts
    dets = np.zeros((t, cap), DET)
    raw = dets.view(np.uint8).reshape(t, cap, 28)
    raw[:] = rng.integers(0, 256, raw.shape, dtype=np.uint8)              # every byte of a record must come through
    for name in ("x1", "y1", "x2", "y2"):
        e = rng.integers(-2000, 20000, (t, cap))
        special = rng.random((t, cap))
        e = np.where(special < 0.05, I32_MIN, np.where(special < 0.10, I32_MAX, np.where(special < 0.15, I32_MAX - 5, e)))
        dets[name] = e
    return dets, counts, tiles, first


def cuts(cap):
    """out_caps worth testing on `seeded_tiles`' batch, whose last image holds 2, 3 and 1 records (1, 1, 1 at cap = 1): 1, one that cuts
    exactly between two tiles, one that cuts inside a tile (none at cap = 1, where a tile is one record), and the largest"""
    return [1, 2, 1200] + ([3, 4] if cap >= 3 else [])


# ---- the host build ----
def tiles_host():
    """libyf_images_host.so with the prototypes of the planner and the merge set"""
    lib = host_lib()
    vp, cl, ci = ctypes.c_void_p, ctypes.c_long, ctypes.c_int
    lib.yfi_plan_tiles_host.restype = cl
    lib.yfi_plan_tiles_host.argtypes = [vp, cl, ci, ci, ci, ci, ci, ci, vp, vp, vp, cl]
    lib.yfi_gather_tiles_host.restype = cl
    lib.yfi_gather_tiles_host.argtypes = [vp, vp, cl, ci, vp, vp, cl, vp, vp, ci]
    return lib


def host_plan(lib, parents, fmt, th, tw, sy, sx, whole):
    """the host build's plan: count first, then fill -> (tiles, descriptors, first), or the negative return value"""
    parents = np.ascontiguousarray(parents)
    n = parents.shape[0]
    args = (parents.ctypes.data, n, fmt, th, tw, sy, sx, int(whole))
    t = lib.yfi_plan_tiles_host(*args, None, None, None, 0)
    if t < 0:
        return t
    tiles, desc, first = np.zeros(t + 1, TILE), np.zeros(t + 1, IMAGE), np.full(n + 2, -9, np.int32)
    tiles["image"][t] = desc["height"][t] = -9                             # one past the end: must stay
    assert lib.yfi_plan_tiles_host(*args, tiles.ctypes.data, desc.ctypes.data, first.ctypes.data, t) == t
    assert tiles["image"][t] == -9 and desc["height"][t] == -9 and first[n + 1] == -9
    return tiles[:t], desc[:t], first[:n + 1]


def host_gather(lib, dets, counts, cap, tiles, first, out_cap, fill=0xA5):
    """the host build's merge -> (bytes uint8[n, out_cap, 28], totals int32[n]), unwritten slots `fill`, unwritten totals -7"""
    n, t = len(first) - 1, dets.shape[0]
    dets, counts = np.ascontiguousarray(dets), np.ascontiguousarray(counts, np.int32)
    tiles, first = np.ascontiguousarray(tiles), np.ascontiguousarray(first, np.int32)
    out = np.full((max(n, 1), out_cap, 28), fill, np.uint8)
    totals = np.full(max(n, 1), -7, np.int32)
    assert lib.yfi_gather_tiles_host(dets.ctypes.data, counts.ctypes.data, t, cap, tiles.ctypes.data, first.ctypes.data, n,
                                     out.ctypes.data, totals.ctypes.data, out_cap) == n
    return out[:n], totals[:n]
