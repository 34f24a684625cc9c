"""The tile grid, the planner and the merge of csrc/yf_images_tiles.h in their host build (libyf_images_host.so) against the plain-Python
statement of tests/tiles_support.py.  No GPU."""
import numpy as np
import pytest

import tiles_support as ts
from images_support import host_lib


@pytest.fixture(scope="module")
def lib():
    return ts.tiles_host()


def _parents(shapes, C, crop=False):
    """packed parents one after the other, or parents that are crops of a wider picture (row stride above w * C, offset inside it)"""
    p, off = np.zeros(len(shapes), ts.IMAGE), 0
    for i, (h, w) in enumerate(shapes):
        rs = (w + 37 + i) * C if crop else w * C
        p[i] = (off + (5 * C if crop else 0), h, w, rs)
        off += h * rs + 64
    return p, off


def _lengths(T, S):
    return sorted({L for L in (1, T - 1, T, T + 1, T + S - 1, T + S, T + S + 1, 16384) if L >= 1})


@pytest.mark.parametrize("whole", [0, 1])
@pytest.mark.parametrize("T", [8, 96])
def test_plan_equals_the_restatement(lib, T, whole):
    for S in sorted({1, T // 2, T}):
        Ls = _lengths(T, S)
        # every length on each axis against every small length on the other; 16384 x 16384 is counted only (below)
        shapes = [(a, b) for a in Ls for b in Ls if min(a, b) <= T + S + 1 and max(a, b) < 16384]
        shapes += [(16384, b) for b in (1, T, T + 1)] + [(a, 16384) for a in (1, T, T + 1)]
        for fmt in (0, 3):
            parents, _ = _parents(shapes, ts.CHANNELS[fmt])
            got = ts.host_plan(lib, parents, fmt, T, T + 3, S, S, whole)
            want = ts.plan_restated(parents, fmt, T, T + 3, S, S, whole)
            for g, w in zip(got, want):
                assert g.tobytes() == w.tobytes(), (T, S, whole, fmt)


def test_axis_rule_on_every_length(lib):
    """one axis, every L up to 3 T, every stride: count, origins, the last tile flush, no gap"""
    for T in (1, 2, 5, 8):
        for S in range(1, T + 1):
            for L in range(1, 3 * T + 3):
                tiles = ts.axis_tiles(L, T, S)
                assert tiles[0][0] == 0 and tiles[-1][0] + tiles[-1][1] == L
                assert all(b[0] <= a[0] + a[1] and b[0] > a[0] for a, b in zip(tiles, tiles[1:])), (L, T, S)
                parents, _ = _parents([(L, 1)], 3)
                got, _, first = ts.host_plan(lib, parents, 0, T, 1, S, 1, 0)
                assert [(int(g["y0"]), int(g["height"])) for g in got] == tiles and first.tolist() == [0, len(tiles)]


def test_count_only_of_the_largest_image(lib):
    parents, _ = _parents([(16384, 16384)], 3)
    args = (parents.ctypes.data, 1, 0, 8, 8, 4, 4)
    k = (16384 - 8 + 3) // 4 + 1
    assert lib.yfi_plan_tiles_host(*args, 1, None, None, None, 0) == k * k + 1
    assert lib.yfi_plan_tiles_host(*args, 0, None, None, None, 0) == k * k
    assert lib.yfi_plan_tiles_host(parents.ctypes.data, 1, 0, 16384, 16384, 1, 1, 1, None, None, None, 0) == 1     # not doubled
    # 2^28 + 1 tiles per image at tile 1: eight such images reach 2^31
    eight = np.repeat(parents, 8)
    assert lib.yfi_plan_tiles_host(eight.ctypes.data, 7, 0, 1, 1, 1, 1, 1, None, None, None, 0) == 7 * (2 ** 28 + 1)
    assert lib.yfi_plan_tiles_host(eight.ctypes.data, 8, 0, 1, 1, 1, 1, 0, None, None, None, 0) == -1


@pytest.mark.parametrize("crop", [False, True])
def test_tile_descriptors_are_valid_images_and_cover_every_pixel(lib, crop):
    host_lib()                                                               # (sets yfi_image_ok_host's prototype on the same handle)
    shapes = [(1, 1), (7, 31), (20, 20), (33, 47), (64, 9), (50, 50)]
    for fmt in (0, 2):
        C = ts.CHANNELS[fmt]
        parents, nbytes = _parents(shapes, C, crop)
        for (T, S), whole in (((20, 20), 0), ((20, 13), 1), ((16, 1), 0), ((7, 3), 1)):
            tiles, desc, first = ts.host_plan(lib, parents, fmt, T, T + 1, S, S, whole)
            for i, p in enumerate(parents):
                assert lib.yfi_image_ok_host(int(p["offset"]), int(p["height"]), int(p["width"]), int(p["row_stride"]), C, nbytes)
                seen = np.zeros((p["height"], p["width"]), bool)
                for j in range(first[i], first[i + 1]):
                    d, q = desc[j], tiles[j]
                    assert lib.yfi_image_ok_host(int(d["offset"]), int(d["height"]), int(d["width"]), int(d["row_stride"]), C, nbytes), (i, j)
                    assert q["image"] == i and 0 <= q["x0"] and q["x0"] + q["width"] <= p["width"] and 0 <= q["y0"] and q["y0"] + q["height"] <= p["height"]
                    assert d["offset"] == p["offset"] + q["y0"] * p["row_stride"] + q["x0"] * C and d["row_stride"] == p["row_stride"]
                    if not (whole and j == first[i] and first[i + 1] - first[i] > 1):
                        seen[q["y0"]:q["y0"] + q["height"], q["x0"]:q["x0"] + q["width"]] = True
                assert seen.all(), (i, T, S)                                 # the grid alone covers the image, without the whole-image tile


def test_plan_refuses_bad_arguments(lib):
    parents, _ = _parents([(40, 50)], 3)
    tiles, desc, first = np.zeros(64, ts.TILE), np.zeros(64, ts.IMAGE), np.zeros(2, np.int32)
    out = (tiles.ctypes.data, desc.ctypes.data, first.ctypes.data)
    plan = lambda *a: lib.yfi_plan_tiles_host(*a)
    pp = parents.ctypes.data
    assert plan(pp, 1, 0, 16, 16, 8, 8, 1, *out, 64) == 25                   # 4 x 6 tiles and the whole image
    for bad in [(pp, 1, 4, 16, 16, 8, 8, 1, *out, 64), (pp, 1, -1, 16, 16, 8, 8, 1, *out, 64),     # format
                (pp, -1, 0, 16, 16, 8, 8, 1, *out, 64), (None, 1, 0, 16, 16, 8, 8, 1, *out, 64),   # n, images
                (pp, 1, 0, 0, 16, 1, 8, 1, *out, 64), (pp, 1, 0, 16, -2, 8, 1, 1, *out, 64),       # tile sides
                (pp, 1, 0, 16, 16, 0, 8, 1, *out, 64), (pp, 1, 0, 16, 16, 8, 17, 1, *out, 64),     # strides
                (pp, 1, 0, 16, 16, 8, 8, 1, *out, 24), (pp, 1, 0, 16, 16, 8, 8, 1, *out, -1),      # tiles_cap
                (pp, 1, 0, 16, 16, 8, 8, 1, out[0], None, out[2], 64), (pp, 1, 0, 16, 16, 8, 8, 1, out[0], out[1], None, 64)]:
        assert plan(*bad) == -1, bad
    for h, w in ((0, 5), (5, 0), (16385, 5), (5, 16385), (-3, 5)):
        p = parents.copy()
        p["height"], p["width"] = h, w
        assert plan(p.ctypes.data, 1, 0, 16, 16, 8, 8, 1, None, None, None, 0) == -1, (h, w)
    assert plan(None, 0, 0, 16, 16, 8, 8, 1, *out, 0) == 0 and first[0] == 0  # an empty batch


def test_shift_is_the_clamped_int64_sum():
    recs = np.zeros(6, ts.DET)
    recs["x1"] = [ts.I32_MIN, ts.I32_MAX, ts.I32_MAX - 5, ts.I32_MAX - 16383, ts.I32_MAX - 16384, -7]
    got = ts.translate(recs, 3, 16383, 0)["x1"].tolist()
    assert got == [ts.I32_MIN + 16383, ts.I32_MAX, ts.I32_MAX, ts.I32_MAX, ts.I32_MAX - 1, 16376]
    assert got == [ts.shift(v, 16383) for v in recs["x1"]]


@pytest.mark.parametrize("cap", [1, 147, 1200])
def test_gather_equals_the_restatement(lib, cap):
    dets, counts, tiles, first = ts.seeded_tiles(np.random.default_rng(700 + cap), cap)
    assert {0, -1, ts.I32_MIN, cap, cap + 1} <= set(counts.tolist())
    for out_cap in ts.cuts(cap):
        want, totals = ts.expect_gather(dets, counts, cap, tiles, first, out_cap)
        got, got_totals = ts.host_gather(lib, dets, counts, cap, tiles, first, out_cap)
        assert np.array_equal(got_totals, totals) and ((totals > out_cap).any() or out_cap == 1200), out_cap
        assert np.array_equal(got, want), out_cap


def test_gather_of_nothing(lib):
    dets, counts, tiles, first = ts.seeded_tiles(np.random.default_rng(5), 4, per_image=[2, 1])
    got, totals = ts.host_gather(lib, dets, counts, 4, tiles, first[:1], 9)          # n = 0
    assert got.shape[0] == 0
    out, oc = np.full((2, 9, 28), 0xA5, np.uint8), np.full(2, -7, np.int32)
    zero = np.zeros(3, np.int32)
    assert lib.yfi_gather_tiles_host(dets.ctypes.data, counts.ctypes.data, 0, 4, tiles.ctypes.data, zero.ctypes.data, 2, out.ctypes.data,
                                     oc.ctypes.data, 9) == 2                          # t = 0
    assert (out == 0xA5).all() and (oc == -7).all()
    for bad in [(-1, 4, 2, 9), (3, 0, 2, 9), (3, 1201, 2, 9), (3, 4, -1, 9), (3, 4, 2, 0), (3, 4, 2, 1201), (2 ** 31 // 4, 4, 2, 9)]:
        t, cap, n, out_cap = bad
        assert lib.yfi_gather_tiles_host(dets.ctypes.data, counts.ctypes.data, t, cap, tiles.ctypes.data, first.ctypes.data, n,
                                         out.ctypes.data, oc.ctypes.data, out_cap) == -1, bad
