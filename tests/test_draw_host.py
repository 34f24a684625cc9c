"""The drawing on the CPU: the host build of csrc/yf_images_draw.h (yfi_draw_records_host, yfi_draw_records_yuv_host,
libyf_images_host.so) against the plain-numpy statement, `ptq.draw_rectangles_u8` and `ptq.draw_rectangles_yuv420sp`, byte for byte over
the whole buffer of the designed batches of tests/draw_support.py: every packed format and NV12 / NV21, half 0 to 3, one colour and keyed
colours (key strides 4 and 16; palettes of 1, 3 and 256 colours, some with a top byte; keys above the palette's size).  Every byte that is
no drawn byte -- row padding, gaps, alpha, the invalid picture -- is in the expected buffer as it was laid out.  And the rule itself
against a literal second construction, the spans the kernels walk against the rule, the order of the records, a second call, and the
argument checks.  No GPU."""
import itertools

import numpy as np
import pytest

import draw_support as ds
from images_support import ptq          # noqa: F401 (fixture)

FORMATS = [0, 1, 2, 3, 4, 5]


@pytest.mark.parametrize("fmt", FORMATS)
def test_host_build_equals_the_restatement_on_the_designed_batch(fmt):
    for half in ds.HALVES:
        buf, desc, pictures, dets, counts = ds.batch_of(fmt, half)
        n = dets.shape[0]
        invalid = ds.SURFACES_INVALID if fmt in (4, 5) else ds.PACKED_INVALID
        want_first = np.concatenate([[0], np.cumsum([min(max(int(c), 0), ds.CAP) for c in counts])]).astype(np.int32)
        assert (counts > ds.CAP).any() and (counts <= 0).any()
        rc, got, first, status = ds.host_draw(buf, fmt, desc, dets, counts, ds.CAP, half)
        assert rc == n and np.array_equal(first, want_first) and status.tolist() == ds.status_of(n, invalid), (fmt, half)
        assert np.array_equal(got, ds.expected(fmt, half)), (fmt, half)
        assert not np.array_equal(got, buf), (fmt, half)
        stride, pn = ds.KEYED[half]
        keys, pal = ds.keys_for(n, ds.CAP, stride, half), ds.palette(pn)
        assert (keys[..., 0] >= pn).any() and (pal >> 24).any()
        rc, keyed, first, status = ds.host_draw(buf, fmt, desc, dets, counts, ds.CAP, half, keys=keys, pal=pal)
        assert rc == n and np.array_equal(first, want_first) and status.tolist() == ds.status_of(n, invalid), (fmt, half)
        assert np.array_equal(keyed, ds.expected(fmt, half, keys, pal)), (fmt, half)
        # the same pixels are drawn whatever the colours: where one differs from the picture and the other does not, they chose the byte
        assert pn == 1 or not np.array_equal(keyed, got), (fmt, half)
    # alpha is never written, and U and V change places between NV12 and NV21
    if fmt in (2, 3):
        inside = np.zeros(buf.shape, bool)
        for f, d in enumerate(desc):
            h, w, C = pictures[f].shape
            np.lib.stride_tricks.as_strided(inside[int(d["offset"]):], shape=(h, w, C), strides=(w * C + 5, C, 1))[..., :3] = True
        assert np.array_equal(got[~inside], buf[~inside])
    if fmt == 5:
        other = ds.host_draw(buf, 4, desc, dets, counts, ds.CAP, 3)[1]
        assert not np.array_equal(other, got)


def _literal(boxes, half, w, h):
    """the second construction, for half 0 and 1: four bands of 2 * half + 1 pixels along the edges, each from corner to corner, and a
    plus-shaped cap of arm `half` at each corner -> bool [n, h, w]"""
    b = np.asarray(boxes, np.int64)
    xa, xb = np.minimum(b[:, 0], b[:, 2])[:, None, None], np.maximum(b[:, 0], b[:, 2])[:, None, None]
    ya, yb = np.minimum(b[:, 1], b[:, 3])[:, None, None], np.maximum(b[:, 1], b[:, 3])[:, None, None]
    x, y = np.arange(w)[None, None, :], np.arange(h)[None, :, None]
    along_x, along_y = (x >= xa) & (x <= xb), (y >= ya) & (y <= yb)
    out = along_x & (np.abs(y - ya) <= half) | along_x & (np.abs(y - yb) <= half)
    out = out | along_y & (np.abs(x - xa) <= half) | along_y & (np.abs(x - xb) <= half)
    for cx, cy in ((xa, ya), (xb, ya), (xa, yb), (xb, yb)):
        out = out | (x == cx) & (np.abs(y - cy) <= half) | (y == cy) & (np.abs(x - cx) <= half)
    return out


def _all_small_boxes():
    r = range(-3, 11)
    return np.array(list(itertools.product(r, r, r, r)), np.int32)


def test_the_rule_equals_a_literal_second_construction():
    small = _all_small_boxes()
    assert small.shape[0] == 14 ** 4
    for half in (0, 1):
        assert np.array_equal(ds.host_masks(small, half, 8, 8), _literal(small, half, 8, 8)), half
        for w, h in sorted(set(ds.PACKED + ds.SURFACES)):
            boxes = np.array(ds.designed_boxes(w, h, half), np.int64)
            assert np.array_equal(ds.host_masks(boxes, half, w, h), _literal(boxes, half, w, h)), (half, w, h)
    # half 0 is the one-pixel outline; half 1 lacks the four outermost corner pixels of its three-pixel frame
    one = ds.host_masks(np.array([[2, 2, 5, 5]], np.int32), 0, 8, 8)[0]
    want = np.zeros((8, 8), bool)
    want[2:6, 2:6] = True
    want[3:5, 3:5] = False
    assert np.array_equal(one, want)
    two = ds.host_masks(np.array([[2, 2, 5, 5]], np.int32), 1, 8, 8)[0]
    want = np.zeros((8, 8), bool)
    want[1:7, 1:7] = True
    want[[1, 1, 6, 6], [1, 6, 1, 6]] = False
    assert np.array_equal(two, want)


def test_the_rule_equals_the_restatement_for_every_half(ptq):
    small = _all_small_boxes()[::7]
    for half in ds.HALVES:
        masks = ds.host_masks(small, half, 8, 8)
        for box, mask in zip(small, masks):
            assert np.array_equal(mask, ptq.outline_mask(box, half, 8, 8)), (half, box)


def test_the_bands_hold_every_drawn_pixel_once():
    """what the kernels walk: the rows top / bottom over the columns `across`, the rows between over `left` and `right` -- disjoint,
    inside the picture, and holding the whole drawn set; a record that is not visible draws nothing"""
    small = _all_small_boxes()
    extremes = np.array([[ds.I32_MIN, ds.I32_MIN, ds.I32_MAX, ds.I32_MAX], [ds.I32_MIN, 3, 4, ds.I32_MAX], [ds.I32_MAX, 0, ds.I32_MAX, 9],
                         [-40000, -40000, 40000, 40000]], np.int64).astype(np.int32)
    boxes = np.concatenate([small, extremes])
    w, h = 8, 6
    x, y = np.arange(w)[None, :], np.arange(h)[None, :]
    for half in ds.HALVES:
        masks, bands = ds.host_masks(boxes, half, w, h), ds.host_bands(boxes, half, w, h)
        inside = lambda k, idx: (idx >= bands[:, 2 * k, None]) & (idx < bands[:, 2 * k, None] + np.maximum(bands[:, 2 * k + 1, None], 0))
        top, bottom, between, across, left, right = (inside(k, y if k < 3 else x) for k in range(6))
        for k in range(6):
            side = h if k < 3 else w
            assert ((bands[:, 2 * k + 1] <= 0) | ((bands[:, 2 * k] >= 0) & (bands[:, 2 * k] + bands[:, 2 * k + 1] <= side))).all(), (half, k)
        assert not (top & bottom).any() and not (top & between).any() and not (bottom & between).any() and not (left & right).any(), half
        walked = ((top | bottom)[:, :, None] & across[:, None, :]) | (between[:, :, None] & (left | right)[:, None, :])
        assert not (masks & ~walked).any(), half
        drawn = masks.any(axis=(1, 2))
        assert not (drawn & (bands[:, 12] == 0)).any(), half                       # "not visible" is never wrong ...
        if half == 0:                                      # ... and the one-pixel outline is its bands exactly, and visible iff drawn
            assert np.array_equal(masks, walked) and np.array_equal(drawn, bands[:, 12] != 0)
    assert not ds.host_masks(extremes[:1], 3, w, h).any() and ds.host_bands(extremes[:1], 3, w, h)[0, 12] == 0


def _permuted(dets, counts, cap, seed):
    rng = np.random.default_rng(seed)
    out = dets.copy()
    for f in range(dets.shape[0]):
        m = min(max(int(counts[f]), 0), cap)
        out[f, :m] = dets[f, rng.permutation(m)]
    return out


@pytest.mark.parametrize("fmt", [2, 4])
def test_order_of_the_records_and_a_second_call(fmt):
    half = 2
    buf, desc, _, dets, counts = ds.batch_of(fmt, half)
    n = dets.shape[0]
    shuffled = _permuted(dets, counts, ds.CAP, 6500)
    assert shuffled.tobytes() != dets.tobytes()
    once = ds.host_draw(buf, fmt, desc, dets, counts, ds.CAP, half)[1]
    assert np.array_equal(ds.host_draw(buf, fmt, desc, shuffled, counts, ds.CAP, half)[1], once)          # one colour: any order
    assert np.array_equal(ds.host_draw(once, fmt, desc, dets, counts, ds.CAP, half)[1], once)             # a second call
    keys, pal = ds.keys_for(n, ds.CAP, 4), ds.palette(256)
    keyed = ds.host_draw(buf, fmt, desc, dets, counts, ds.CAP, half, keys=keys, pal=pal)[1]
    assert np.array_equal(keyed, ds.expected(fmt, half, keys, pal))                                       # slot order (the restatement's)
    assert np.array_equal(ds.host_draw(keyed, fmt, desc, dets, counts, ds.CAP, half, keys=keys, pal=pal)[1], keyed)
    # with keys the order shows: the same records and keys, each frame's in reverse order, give other bytes where outlines overlap
    rev, rkeys = dets.copy(), keys.copy()
    for f in range(n):
        m = min(max(int(counts[f]), 0), ds.CAP)
        rev[f, :m], rkeys[f, :m] = dets[f, :m][::-1], keys[f, :m][::-1]
    other = ds.host_draw(buf, fmt, desc, rev, counts, ds.CAP, half, keys=rkeys, pal=pal)[1]
    assert not np.array_equal(other, keyed)


def test_the_capacity_frame():
    """1200 keyed records on one 64 x 48 picture, cap 1200"""
    dets, counts = ds.capacity_batch()
    pictures = [ds.cs.in_format(ds._rgb(4), 1)]
    buf, desc = ds.rs.lay_out_packed(pictures)
    keys, pal = ds.keys_for(1, 1200, 16), ds.palette(256)
    rc, got, first, status = ds.host_draw(buf, 1, desc, dets, counts, 1200, 1, keys=keys, pal=pal)
    assert rc == 1 and first.tolist() == [0, 1200] and status.tolist() == [0]
    assert np.array_equal(got, ds.expected_packed(pictures, 1, dets, counts, 1200, 1, keys, pal, invalid=()))


def test_the_argument_check_rejects_every_fault():
    keys, pal = ds.keys_for(4, ds.CAP, 16), ds.palette(3)
    kp, pp = keys.ctypes.data, pal.ctypes.data
    keyed = dict(keys=kp, key_stride=16, palette=pp, palette_n=3)
    assert ds.host_check() == "" and ds.host_check(colour=0xFFFFFF, half=0) == "" and ds.host_check(n=0) == "" and ds.host_check(**keyed) == ""
    for half in ds.HALVES:
        assert ds.host_check(half=half) == ""
    for stride in range(4, 65, 4):
        assert ds.host_check(**dict(keyed, key_stride=stride)) == ""
    assert ds.host_check(**dict(keyed, colour=0xFF000000)) == ""                  # with keys the colour is not looked at
    for kw, text in ((dict(half=-1), "half must be in [0, 3]"), (dict(half=4), "half must be in [0, 3]"), (dict(colour=0x01000000), "top byte"),
                     (dict(colour=0xFF000000), "top byte"), (dict(key_stride=4), "without d_keys"), (dict(palette=pp), "without d_keys"),
                     (dict(palette_n=1), "without d_keys"), (dict(keyed, key_stride=0), "key_stride must be a multiple of 4 in [4, 64]"),
                     (dict(keyed, key_stride=6), "key_stride"), (dict(keyed, key_stride=68), "key_stride"), (dict(keyed, key_stride=-4), "key_stride"),
                     (dict(keyed, palette=None), "d_palette is NULL"), (dict(keyed, palette_n=0), "palette_n must be in [1, 256]"),
                     (dict(keyed, palette_n=257), "palette_n"), (dict(keyed, keys=kp + 2), "4-byte aligned"),
                     (dict(keyed, palette=pp + 1), "4-byte aligned"), (dict(cap=0), "cap"), (dict(cap=1201), "cap"), (dict(n=-1), "n must"),
                     (dict(n=2 ** 31 // 1200 + 1, cap=1200), "n * cap"), (dict(n=2 ** 31 - 1, cap=1), "n must")):
        assert text in ds.host_check(**kw), (kw, ds.host_check(**kw))
    # the entries refuse what the check refuses, and the other family's formats, and touch nothing
    buf, desc, _, dets, counts = ds.batch_of(0, 1)
    lib = ds.draw_host()
    for half, colour in ((4, 0), (1, 1 << 24)):
        rc, got, first, status = ds.host_draw(buf, 0, desc, dets, counts, ds.CAP, half, colour=colour)
        assert rc == -1 and np.array_equal(got, buf) and (first == ds.SENTINEL32).all() and (status == ds.SENTINEL32).all()
    assert lib.yfi_draw_records_host(None, 0, 4, None, None, None, 0, 1, 1, 0, None, 0, None, 0, None, None) == -1
    assert lib.yfi_draw_records_yuv_host(None, 0, 0, None, None, None, 0, 1, 1, 0, None, 0, None, 0, None, None) == -1
