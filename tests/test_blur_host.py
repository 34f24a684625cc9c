"""The blur on the CPU: the host build of csrc/yf_images_blur.h (yfi_blur_records_host, yfi_blur_records_yuv_host, libyf_images_host.so)
against the plain-numpy statement, `ptq.blur_u8` and `ptq.blur_yuv420sp` on `ptq.crop_region`, byte for byte over the whole buffer: the
designed batches of tests/redact_support.py in every packed format and as NV12 / NV21 surfaces at grids 1, 3, 8 and 16, margins 0 and 250,
square off and on; strips of 1 x W for every W up to 260 and 16384; small regions and their grid sizes; a workspace too small (the filled
tail and status bit 1); permuted records; invalid descriptors; the argument check; and a surface whose Y sum passes 2^32.  No GPU."""
import numpy as np
import pytest

import blur_support as bs
import crops_support as cs
import redact_support as rs
from images_support import ptq          # noqa: F401 (fixture)

CASES = [(g, m, s) for g in bs.GRIDS for m, s in rs.GRID]


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_host_build_equals_the_restatement_on_the_designed_batch(fmt):
    dets, counts = rs.designed()
    buf, desc, pictures = rs.packed_batch(fmt)
    n = dets.shape[0]
    want_first = rs.first_of(counts, rs.CAP)
    inside = np.zeros(buf.shape, bool)                                         # the colour bytes of the pictures
    for f, d in enumerate(desc):
        h, w, C = pictures[f].shape
        rows = np.lib.stride_tricks.as_strided(inside[int(d["offset"]):], shape=(h, w, C), strides=(int(d["row_stride"]), C, 1))
        rows[..., :3] = True
    for grid, margin, square in CASES:
        where = (fmt, grid, margin, square)
        rc, got, first, status = bs.host_blur(buf, fmt, desc, dets, counts, rs.CAP, grid, margin, square)
        assert rc == n and np.array_equal(first, want_first) and not status.any(), where
        assert np.array_equal(got, bs.expected_packed(pictures, fmt, dets, counts, rs.CAP, grid, margin, square)), where
        assert np.array_equal(got[~inside], buf[~inside]), where               # gaps, row padding and alpha bytes stay
        assert not np.array_equal(got, buf), where
        # the frames whose counts are 0 and -3, and the 1 x 1 picture, keep their bytes
        for f in (2, 5, 6):
            d, (h, w, C) = desc[f], pictures[f].shape
            a = int(d["offset"])
            z = a + (h - 1) * int(d["row_stride"]) + w * C
            assert np.array_equal(got[a:z], buf[a:z]), (where, f)


@pytest.mark.parametrize("fmt", [4, 5])
def test_host_build_equals_the_restatement_on_surfaces(fmt):
    buf, desc, surfaces, dets, counts = rs.yuv_batch()
    n = dets.shape[0]
    for grid, margin, square in CASES:
        where = (fmt, grid, margin, square)
        rc, got, first, status = bs.host_blur(buf, fmt, desc, dets, counts, rs.YUV_CAP, grid, margin, square)
        assert rc == n and np.array_equal(first, rs.first_of(counts, rs.YUV_CAP)) and not status.any(), where
        assert np.array_equal(got, bs.expected_yuv(surfaces, fmt, dets, counts, rs.YUV_CAP, grid, margin, square)), where
        assert not np.array_equal(got, buf), where
    # the blur does not care which of U and V comes first; its fill does
    a = bs.host_blur(buf, 4, desc, dets, counts, rs.YUV_CAP, 8, 0, False)[1]
    b = bs.host_blur(buf, 5, desc, dets, counts, rs.YUV_CAP, 8, 0, False)[1]
    assert np.array_equal(a, b)
    a = bs.host_blur(buf, 4, desc, dets, counts, rs.YUV_CAP, 8, 0, False, records_cap=0)[1]
    b = bs.host_blur(buf, 5, desc, dets, counts, rs.YUV_CAP, 8, 0, False, records_cap=0)[1]
    assert not np.array_equal(a, b)


@pytest.mark.parametrize("grid", bs.GRIDS)
def test_strips_of_every_small_width(grid):
    """1 x W for W = 1 .. 260 and 16384, the whole picture the region: the upsampling taps at every small size"""
    buf, desc, pictures, dets, counts = bs.strips()
    rc, got, first, status = bs.host_blur(buf, 1, desc, dets, counts, 1, grid, 0, False)
    assert rc == len(bs.STRIP_WIDTHS) and first.tolist() == list(range(len(bs.STRIP_WIDTHS) + 1)) and not status.any()
    want = bs.strips_expected(grid)
    if not np.array_equal(got, want):
        at = int(np.nonzero(got != want)[0][0])
        frame = int(np.searchsorted(desc["offset"].astype(np.int64), at, side="right")) - 1
        raise AssertionError(f"grid {grid}: first difference at byte {at}, the strip of width {bs.STRIP_WIDTHS[frame]}")
    assert got[int(desc["offset"][0])] == buf[int(desc["offset"][0])]           # only a 1 x 1 region keeps its bytes


def test_small_regions_and_their_grids(ptq):
    buf, desc, pictures, dets, counts = bs.small_batch()
    for (w, h), (gx, gy) in bs.SMALL:
        assert (ptq.blur_cells(w, 8), ptq.blur_cells(h, 8)) == (gx, gy), (w, h)
        assert ptq.blur_grid_u8(np.zeros((h, w, 3), np.uint8), 8).shape == (gy, gx, 3)
    assert ptq.blur_grid_u8(np.zeros((16, 16, 2), np.uint8), 16, 2).shape == (8, 8, 2)       # the chroma plane's minimum cell is 2
    for grid in bs.GRIDS:
        rc, got, _, status = bs.host_blur(buf, 0, desc, dets, counts, 1, grid, 0, False)
        assert rc == len(bs.SMALL) and not status.any()
        assert np.array_equal(got, bs.expected_packed(pictures, 0, dets, counts, 1, grid, 0, False)), grid
        for f, ((w, h), _) in enumerate(bs.SMALL):                             # no region larger than 1 x 1 keeps all its bytes
            d = desc[f]
            view = np.lib.stride_tricks.as_strided(got[int(d["offset"]):], shape=(40, 40, 3), strides=(int(d["row_stride"]), 3, 1))
            assert not np.array_equal(view[3:3 + h, 2:2 + w], pictures[f][3:3 + h, 2:2 + w]), (grid, w, h)
            keep = np.ones((40, 40), bool)
            keep[3:3 + h, 2:2 + w] = False
            assert np.array_equal(view[keep], pictures[f][keep]), (grid, w, h)
    # a 16 x 16 region at g = 16 is a grid of 4 x 4, not of 16 x 16 (which would give the region back byte for byte)
    region = pictures[3][3:19, 2:18]
    assert np.array_equal(ptq.resize_linear_u8(region, 16, 16), region) and not np.array_equal(ptq.blur_u8(region, [(0, 0, 16, 16)], 16), region)


@pytest.mark.parametrize("fmt", [2, 4])
def test_a_workspace_too_small_fills_the_tail(fmt):
    if fmt == 4:
        buf, desc, pictures, dets, counts = rs.yuv_batch()
        cap, expected = rs.YUV_CAP, bs.expected_yuv
    else:
        dets, counts = rs.designed()
        buf, desc, pictures = rs.packed_batch(fmt)
        cap, expected = rs.CAP, bs.expected_packed
    total = int(rs.first_of(counts, cap)[-1])
    full = bs.host_blur(buf, fmt, desc, dets, counts, cap, 8, 250, False)[1]
    for records_cap in (0, 1, total - 1, total):
        rc, got, first, status = bs.host_blur(buf, fmt, desc, dets, counts, cap, 8, 250, False, records_cap=records_cap)
        assert rc == dets.shape[0] and np.array_equal(first, rs.first_of(counts, cap)), records_cap
        assert status.tolist() == bs.want_status(counts, cap, records_cap), records_cap
        assert np.array_equal(got, expected(pictures, fmt, dets, counts, cap, 8, 250, False, records_cap=records_cap)), records_cap
        if records_cap != total - 1:                                           # (the last record may own no pixel)
            assert np.array_equal(got, full) == (records_cap == total), records_cap
    assert bs.want_status(counts, cap, 0)[0] == bs.FILLED and bs.want_status(counts, cap, total) == [0] * len(counts)
    # records_cap = 0 is the fill under the ownership rule, which for one colour is the fill
    filled = bs.host_blur(buf, fmt, desc, dets, counts, cap, 8, 250, False, records_cap=0)[1]
    assert np.array_equal(filled, rs.host_redact(buf, fmt, desc, dets, counts, cap, rs.FILLED, 0, 250, False)[1])


def _permuted(dets, counts, cap, seed):
    rng = np.random.default_rng(seed)
    out = dets.copy()
    for f in range(dets.shape[0]):
        m = cs.clamp(counts[f], cap)
        out[f, :m] = dets[f, rng.permutation(m)]
    return out


def test_the_order_of_the_records_matters_in_overlaps_only(ptq):
    buf, desc, pictures, dets, counts = bs.disjoint_batch()
    regions = rs.regions_of(dets, counts, rs.CAP, 0, 64, 48, 0, False)
    assert len(regions) == 12 and all(r is not None for r in regions)
    once = bs.host_blur(buf, 3, desc, dets, counts, rs.CAP, 8, 0, False)[1]
    assert not np.array_equal(once, buf)
    for seed in (6400, 6401):
        shuffled = _permuted(dets, counts, rs.CAP, seed)
        assert shuffled.tobytes() != dets.tobytes()
        assert np.array_equal(bs.host_blur(buf, 3, desc, shuffled, counts, rs.CAP, 8, 0, False)[1], once)
    # the overlap set (frame 4 of the designed batch) reversed: the bytes differ, and only where two regions overlap
    dets, counts = rs.designed()
    buf, desc, pictures = rs.packed_batch(0, frames=[4])
    dets, counts = dets[4:5].copy(), counts[4:5].copy()
    back = dets.copy()
    back[0, :9] = dets[0, 8::-1]
    a = bs.host_blur(buf, 0, desc, dets, counts, rs.CAP, 8, 0, False)[1]
    b = bs.host_blur(buf, 0, desc, back, counts, rs.CAP, 8, 0, False)[1]
    covered = np.zeros((48, 64), np.int32)
    for x0, y0, w, h in rs.regions_of(dets, counts, rs.CAP, 0, 64, 48, 0, False):
        covered[y0:y0 + h, x0:x0 + w] += 1
    d = desc[0]
    va, vb = (np.lib.stride_tricks.as_strided(v[int(d["offset"]):], shape=(48, 64, 3), strides=(int(d["row_stride"]), 3, 1)) for v in (a, b))
    differs = (va != vb).any(axis=2)
    assert differs.any() and not (differs & (covered < 2)).any()
    # a second call blurs the blur
    assert not np.array_equal(bs.host_blur(a, 0, desc, dets, counts, rs.CAP, 8, 0, False)[1], a)


def test_an_invalid_descriptor_between_valid_ones():
    dets, counts = rs.designed()
    buf, desc, pictures = rs.packed_batch(0)
    desc = desc.copy()
    desc["row_stride"][1] = int(desc["width"][1]) * 3 - 1                      # a stride below the row
    desc["offset"][3] = buf.nbytes + 1 - ((362 - 1) * int(desc["row_stride"][3]) + 410 * 3)          # ends one byte past the buffer
    for records_cap in (None, 20):
        rc, got, first, status = bs.host_blur(buf, 0, desc, dets, counts, rs.CAP, 8, 250, False, records_cap=records_cap)
        assert rc == 7 and np.array_equal(first, rs.first_of(counts, rs.CAP))
        assert status.tolist() == bs.want_status(counts, rs.CAP, 7 * rs.CAP if records_cap is None else records_cap, invalid={1, 3})
        assert np.array_equal(got, bs.expected_packed(pictures, 0, dets, counts, rs.CAP, 8, 250, False, records_cap=records_cap, invalid={1, 3}))
    assert status.tolist() == [0, 3, 2, 3, 2, 0, 0]
    ybuf, ydesc, surfaces, ydets, ycounts = rs.yuv_batch()
    ydesc = ydesc.copy()
    ydesc["height"][1] += 1                                                    # an odd side
    rc, got, first, status = bs.host_blur(ybuf, 5, ydesc, ydets, ycounts, rs.YUV_CAP, 3, 0, True)
    assert rc == 4 and status.tolist() == [0, 1, 0, 0]
    assert np.array_equal(got, bs.expected_yuv(surfaces, 5, ydets, ycounts, rs.YUV_CAP, 3, 0, True, invalid={1}))


FAULTS = ((dict(grid=0), "grid must be in [1, 16]"), (dict(grid=17), "grid must be"), (dict(grid=-8), "grid must be"),
          (dict(colour=0x01000000), "top byte"), (dict(colour=0xFF000000), "top byte"), (dict(margin=1001), "margin_permille"),
          (dict(margin=-1), "margin_permille"), (dict(flags=2), "flags"), (dict(flags=-1), "flags"), (dict(cap=0), "cap"),
          (dict(cap=1201), "cap"), (dict(n=-1), "n must"), (dict(n=2 ** 31 // 1200 + 1, cap=1200), "n * cap"),
          (dict(n=2 ** 31 - 1, cap=1), "n must"), (dict(records_cap=-1), "records_cap"), (dict(records_cap=4 * rs.CAP + 1), "records_cap"),
          (dict(work_bytes=4 * 64 * 4 - 1), "work_bytes"), (dict(work_bytes=0), "work_bytes"), (dict(work=0), "d_work"),
          (dict(work=24), "d_work"))


def test_the_argument_check_rejects_every_fault():
    assert bs.host_check() == "" and bs.host_check(n=0, records_cap=0) == "" and bs.host_check(colour=0xFFFFFF) == ""
    for grid in range(1, 17):
        assert bs.host_check(grid=grid) == ""
    assert bs.host_check(records_cap=0, work=0, work_bytes=0) == ""              # no workspace: no pointer is asked for
    assert bs.host_check(records_cap=4 * rs.CAP) == "" and bs.host_check(work_bytes=4 * 64 * 4) == ""
    for kw, text in FAULTS:
        assert text in bs.host_check(**kw), (kw, bs.host_check(**kw))
    lib = bs.blur_host()
    assert [lib.yfi_blur_workspace_host(c, g) for c, g in ((0, 8), (1, 1), (1, 8), (3, 3), (5, 16), (-1, 8), (1, 0), (1, 17))] == \
        [0, 16, 256, 112, 5120, 0, 0, 0]
    assert all(lib.yfi_blur_workspace_host(c, g) == bs.workspace(c, g) for c in (0, 1, 7, 560) for g in range(1, 17))
    # the entries refuse what the check refuses, and the other family's formats: nothing is written
    dets, counts = rs.designed()
    buf, desc, _ = rs.packed_batch(0)
    for kw in (dict(grid=0), dict(grid=17), dict(colour=1 << 24), dict(margin=1001), dict(records_cap=7 * rs.CAP + 1), dict(work_bytes=16)):
        rc, got, first, status = bs.host_blur(buf, 0, desc, dets, counts, rs.CAP, kw.get("grid", 8), kw.get("margin", 0), False,
                                              records_cap=kw.get("records_cap"), colour=kw.get("colour", rs.FILL), work_bytes=kw.get("work_bytes"))
        assert rc == -1 and np.array_equal(got, buf) and (first == rs.SENTINEL32).all() and (status == rs.SENTINEL32).all(), kw
    assert lib.yfi_blur_records_host(None, 0, 4, None, None, None, 0, 1, 8, 0, 0, 0, None, 0, 0, None, None) == -1
    assert lib.yfi_blur_records_yuv_host(None, 0, 0, None, None, None, 0, 1, 8, 0, 0, 0, None, 0, 0, None, None) == -1


def test_a_sum_above_32_bits():
    """4128 x 4096, every Y byte 255, grid 1: the one cell's sum is 4 311 613 440.  A constant stays constant: no restatement is needed"""
    buf, desc, dets, counts = bs.big_surface()
    assert 4128 * 4096 * 255 == 4311613440 > 2 ** 32
    rc, got, first, status = bs.host_blur(buf, 4, desc, dets, counts, 1, 1, 0, False)
    assert rc == 1 and first.tolist() == [0, 1] and status.tolist() == [0]
    assert (got[:4128 * 4096] == 255).all() and (got[4128 * 4096:] == 77).all()


def test_the_python_layer_refuses_before_it_stages(ptq):
    """`detect_blurred` and the restatement check their arguments without a GPU; an empty batch is empty"""
    images = rs._mod("images")
    img = [np.zeros((8, 8, 3), np.uint8)]
    for kw, text in ((dict(grid=0), "grid"), (dict(grid=17), "grid"), (dict(colour=(1, 2)), "colour"), (dict(colour=1 << 24), "colour"),
                     (dict(margin=1.5), "margin")):
        with pytest.raises(ValueError, match=text):
            images.detect_blurred(None, img, **kw)
    assert images.detect_blurred(None, []) == ([], [])
    assert (images.BLUR_MAX_GRID, images.BLUR_MIN_CELL) == (ptq.BLUR_MAX_GRID, ptq.BLUR_MIN_CELL) == (16, 4)
    for grid in (0, 17, 2.5, True):
        with pytest.raises(ValueError, match="grid"):
            ptq.blur_u8(img[0], [(0, 0, 8, 8)], grid)
    with pytest.raises(ValueError, match="grid"):
        ptq.blur_yuv420sp(np.zeros((4, 4), np.uint8), np.zeros((2, 4), np.uint8), [], 0)
