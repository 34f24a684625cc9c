"""The redaction on the CPU: the host build of csrc/yf_images_redact.h (yfi_redact_records_host, yfi_redact_records_yuv_host,
libyf_images_host.so) against the plain-Python statement, `ptq.redact_u8` and `ptq.redact_yuv420sp` on `ptq.crop_region`, byte for byte
over the whole buffer of the designed batches of tests/redact_support.py: every packed format and NV12 / NV21, the mosaic at blocks of 4,
8 and 64 and the fill, margins 0 and 250, square off and on.  Every byte that is no pixel of the redacted set -- row padding, the gaps
between pictures, alpha bytes -- is in the expected buffer as it was laid out, so the comparison of whole buffers holds them too.  No GPU."""
import numpy as np
import pytest

import crops_support as cs
import redact_support as rs
from images_support import ptq          # noqa: F401 (fixture)


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_host_build_equals_the_restatement_on_the_designed_batch(fmt):
    dets, counts = rs.designed()
    buf, desc, pictures = rs.packed_batch(fmt)
    n = dets.shape[0]
    assert counts.tolist() == [13, 70, 13, rs.CAP + 84, 9, 0, -3]
    want_first = rs.first_of(counts, rs.CAP)
    for mode, block, margin, square in rs.cases():
        where = (fmt, mode, block, margin, square)
        rc, got, first, status = rs.host_redact(buf, fmt, desc, dets, counts, rs.CAP, mode, block, margin, square)
        assert rc == n and np.array_equal(first, want_first) and not status.any(), where
        want = rs.expected_packed(pictures, fmt, dets, counts, rs.CAP, mode, block, margin, square)
        assert np.array_equal(got, want), where
        # what is no colour byte of a picture keeps what the layout put there: the gaps and the row padding, and the alpha bytes
        inside = np.zeros(buf.shape, bool)
        for f, d in enumerate(desc):
            h, w, C = pictures[f].shape
            assert int(d["offset"]) + (h - 1) * int(d["row_stride"]) + w * C <= buf.nbytes
            rows = np.lib.stride_tricks.as_strided(inside[int(d["offset"]):], shape=(h, w, C), strides=(int(d["row_stride"]), C, 1))
            rows[..., :3] = True
        assert np.array_equal(got[~inside], buf[~inside]), where
        assert not np.array_equal(got, buf), where                             # ... and something was redacted
    # the 1 x 1 picture is one block of one pixel: the mosaic leaves it as it is; at 64 the 37 x 53 picture is one clipped block
    rc, got, _, _ = rs.host_redact(buf, fmt, desc, dets, counts, rs.CAP, rs.MOSAIC, 64, 0, False)
    d = desc[0]
    p0 = np.lib.stride_tricks.as_strided(got[int(d["offset"]):], shape=pictures[0].shape, strides=(int(d["row_stride"]), pictures[0].shape[2], 1))
    mean = (pictures[0][..., :3].astype(np.int64).sum(axis=(0, 1)) + 37 * 53 // 2) // (37 * 53)
    assert (p0[..., :3] == mean).all() and got[int(desc[2]["offset"])] == buf[int(desc[2]["offset"])]


@pytest.mark.parametrize("fmt", [4, 5])
def test_host_build_equals_the_restatement_on_surfaces(fmt):
    buf, desc, surfaces, dets, counts = rs.yuv_batch()
    n = dets.shape[0]
    regions = rs.regions_of(dets, counts, rs.YUV_CAP, 2, 410, 362, 0, False)
    odd = [r for r in regions if r is not None and r[0] % 2 and r[1] % 2]
    assert len(odd) >= 2 and any(r[2] % 2 for r in odd) and any(r[3] % 2 for r in odd)          # odd origins and odd sides
    for mode, block, margin, square in rs.cases():
        where = (fmt, mode, block, margin, square)
        rc, got, first, status = rs.host_redact(buf, fmt, desc, dets, counts, rs.YUV_CAP, mode, block, margin, square)
        assert rc == n and np.array_equal(first, rs.first_of(counts, rs.YUV_CAP)) and not status.any(), where
        assert np.array_equal(got, rs.expected_yuv(surfaces, fmt, dets, counts, rs.YUV_CAP, mode, block, margin, square)), where
        assert not np.array_equal(got, buf), where
    # the mosaic does not care which of U and V comes first; the fill does
    a = rs.host_redact(buf, 4, desc, dets, counts, rs.YUV_CAP, rs.MOSAIC, 8, 0, False)[1]
    b = rs.host_redact(buf, 5, desc, dets, counts, rs.YUV_CAP, rs.MOSAIC, 8, 0, False)[1]
    assert np.array_equal(a, b)
    a = rs.host_redact(buf, 4, desc, dets, counts, rs.YUV_CAP, rs.FILLED, 0, 0, False)[1]
    b = rs.host_redact(buf, 5, desc, dets, counts, rs.YUV_CAP, rs.FILLED, 0, 0, False)[1]
    assert not np.array_equal(a, b)


def _permuted(dets, counts, cap, seed):
    """the records of every frame that count, in another order"""
    rng = np.random.default_rng(seed)
    out = dets.copy()
    for f in range(dets.shape[0]):
        m = cs.clamp(counts[f], cap)
        out[f, :m] = dets[f, rng.permutation(m)]
    return out


def test_mosaic_ignores_the_order_of_the_records_and_a_second_call():
    dets, counts = rs.designed()
    shuffled = _permuted(dets, counts, rs.CAP, 5500)
    assert shuffled.tobytes() != dets.tobytes()
    buf, desc, _ = rs.packed_batch(2)
    ybuf, ydesc, _, ydets, ycounts = rs.yuv_batch()
    for block, margin, square in ((4, 0, False), (8, 250, True), (64, 0, False)):
        once = rs.host_redact(buf, 2, desc, dets, counts, rs.CAP, rs.MOSAIC, block, margin, square)[1]
        assert np.array_equal(rs.host_redact(buf, 2, desc, shuffled, counts, rs.CAP, rs.MOSAIC, block, margin, square)[1], once)
        assert np.array_equal(rs.host_redact(once, 2, desc, dets, counts, rs.CAP, rs.MOSAIC, block, margin, square)[1], once)
        once = rs.host_redact(ybuf, 4, ydesc, ydets, ycounts, rs.YUV_CAP, rs.MOSAIC, block, margin, square)[1]
        again = rs.host_redact(ybuf, 4, ydesc, _permuted(ydets, ycounts, rs.YUV_CAP, 5501), ycounts, rs.YUV_CAP, rs.MOSAIC, block, margin, square)[1]
        assert np.array_equal(again, once)
        assert np.array_equal(rs.host_redact(once, 4, ydesc, ydets, ycounts, rs.YUV_CAP, rs.MOSAIC, block, margin, square)[1], once)


def test_the_capacity_frame():
    """1200 records on one 37 x 53 picture, cap 1200"""
    dets, counts = rs.capacity_batch()
    pictures = [cs.in_format(rs.picture(0), 0)]
    buf, desc = rs.lay_out_packed(pictures)
    for mode, block in ((rs.MOSAIC, 4), (rs.FILLED, 0)):
        rc, got, first, status = rs.host_redact(buf, 0, desc, dets, counts, 1200, mode, block, 0, False)
        assert rc == 1 and first.tolist() == [0, 1200] and status.tolist() == [0]
        assert np.array_equal(got, rs.expected_packed(pictures, 0, dets, counts, 1200, mode, block, 0, False))


def test_an_invalid_descriptor_between_valid_ones():
    dets, counts = rs.designed()
    buf, desc, pictures = rs.packed_batch(0)
    desc = desc.copy()
    desc["row_stride"][1] = int(desc["width"][1]) * 3 - 1                      # a stride below the row
    desc["offset"][3] = buf.nbytes + 1 - ((362 - 1) * int(desc["row_stride"][3]) + 410 * 3)          # ends one byte past the buffer
    for mode, block in ((rs.MOSAIC, 8), (rs.FILLED, 0)):
        rc, got, first, status = rs.host_redact(buf, 0, desc, dets, counts, rs.CAP, mode, block, 250, False)
        assert rc == 7 and status.tolist() == [0, 1, 0, 1, 0, 0, 0] and np.array_equal(first, rs.first_of(counts, rs.CAP))
        assert np.array_equal(got, rs.expected_packed(pictures, 0, dets, counts, rs.CAP, mode, block, 250, False, invalid={1, 3}))
    ybuf, ydesc, surfaces, ydets, ycounts = rs.yuv_batch()
    ydesc = ydesc.copy()
    ydesc["height"][1] += 1                                                    # an odd side
    rc, got, first, status = rs.host_redact(ybuf, 5, ydesc, ydets, ycounts, rs.YUV_CAP, rs.MOSAIC, 4, 0, True)
    assert rc == 4 and status.tolist() == [0, 1, 0, 0]
    assert np.array_equal(got, rs.expected_yuv(surfaces, 5, ydets, ycounts, rs.YUV_CAP, rs.MOSAIC, 4, 0, True, invalid={1}))


def test_the_argument_check_rejects_every_fault():
    assert rs.host_check() == "" and rs.host_check(mode=rs.FILLED, block=0, colour=0xFFFFFF) == "" and rs.host_check(n=0) == ""
    for block in (4, 8, 16, 32, 64):
        assert rs.host_check(block=block) == ""
    for kw, text in ((dict(block=0), "block must be 4, 8, 16, 32 or 64"), (dict(block=12), "block must be 4"), (dict(block=128), "block must be 4"),
                     (dict(block=-8), "block must be 4"), (dict(block=2), "block must be 4"),
                     (dict(mode=rs.FILLED, block=8), "block must be 0"), (dict(mode=rs.FILLED, block=0, colour=0x01000000), "top byte"),
                     (dict(mode=rs.FILLED, block=0, colour=0xFF000000), "top byte"), (dict(mode=2), "mode"), (dict(mode=-1), "mode"),
                     (dict(margin=1001), "margin_permille"), (dict(margin=-1), "margin_permille"), (dict(flags=2), "flags"),
                     (dict(flags=-1), "flags"), (dict(cap=0), "cap"), (dict(cap=1201), "cap"), (dict(n=-1), "n must"),
                     (dict(n=2 ** 31 // 1200 + 1, cap=1200), "n * cap"), (dict(n=2 ** 31 - 1, cap=1), "n must")):
        assert text in rs.host_check(**kw), (kw, rs.host_check(**kw))
    # the colour is not looked at in the mosaic; the entries refuse what the check refuses, and the other family's formats
    assert rs.host_check(colour=0xFF000000) == ""
    dets, counts = rs.designed()
    buf, desc, _ = rs.packed_batch(0)
    for kw in (dict(mode=rs.MOSAIC, block=12), dict(mode=rs.FILLED, block=0, colour=1 << 24), dict(mode=rs.MOSAIC, block=8, margin=1001)):
        rc, got, first, status = rs.host_redact(buf, 0, desc, dets, counts, rs.CAP, kw["mode"], kw["block"], kw.get("margin", 0), False,
                                                colour=kw.get("colour", rs.FILL))
        assert rc == -1 and np.array_equal(got, buf) and (first == rs.SENTINEL32).all() and (status == rs.SENTINEL32).all(), kw
    lib = rs.redact_host()
    assert lib.yfi_redact_records_host(None, 0, 4, None, None, None, 0, 1, 0, 8, 0, 0, 0, None, None) == -1
    assert lib.yfi_redact_records_yuv_host(None, 0, 0, None, None, None, 0, 1, 0, 8, 0, 0, 0, None, None) == -1
