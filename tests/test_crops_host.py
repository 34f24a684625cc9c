"""The face chips on the CPU: the host build of csrc/yf_images_crop.h (yfi_crop_records_host, libyf_images_host.so) against the plain-Python
statement, `ptq.crop_region` in Python integers and `ptq.crop_resize_u8` (the restated cv2.resize of the slice), byte for byte on the
designed records of tests/crops_support.py; and the claim of csrc/yf_images_taps.h that its scale n_in / n_out gives the float32 source
coordinate OpenCV's 1 / (n_out / n_in) gives, for every output side 1..256 and every input side 1..16384.  No GPU."""
import numpy as np
import pytest

import crops_support as cs
from images_support import ptq          # noqa: F401 (fixture)


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_host_build_equals_the_restatement_on_the_designed_records(fmt):
    buf, desc, dets, counts, keys = cs.designed_batch(fmt)
    n = dets.shape[0]
    total = sum(cs.clamp(c, cs.CAP) for c in counts)
    assert total == 4 * 13 + cs.CAP and counts.tolist() == [13, 13, 13, 13, 0, cs.CAP + 84, -3]
    for out_h, out_w in cs.OUTS:
        for margin, square in cs.GRID:
            for order in ("rgb", "bgr"):
                want, want_info, want_first = cs.expected(dets, counts, cs.CAP, keys, out_h, out_w, margin, square, order)
                rc, chips, info, first = cs.host_crop(buf, fmt, desc, dets, counts, cs.CAP, out_h, out_w, margin, square, order, total + 2)
                where = (fmt, out_h, out_w, margin, square, order)
                assert rc == n, where
                assert np.array_equal(first, want_first), where
                assert info[:total].tobytes() == want_info.tobytes(), where
                assert np.array_equal(chips[:total], want), where
                assert (chips[total:] == 0xA5).all() and (info[total:].view(np.uint8) == 0xA5).all(), where
    # every kind of chip occurs: status 0 and 1, clamped regions, and regions the margin or the square changes
    _, info0, _ = cs.expected(dets, counts, cs.CAP, keys, 16, 16, 0, False, "rgb")
    _, info1, _ = cs.expected(dets, counts, cs.CAP, keys, 16, 16, 250, True, "rgb")
    assert {0, 1} == set(info0["status"].tolist()) and (info0["status"] == 1).sum() >= 3 * 4
    assert (info0.tobytes() != info1.tobytes()) and ((info1["width"] == info1["height"]) & (info1["status"] == 0)).any()


def test_region_rule_of_the_host_build_equals_python_integers(ptq):
    """the rule alone, on seeded edges that include the int32 extremes, all margins' ends and both flags"""
    host = cs.crops_host()
    rng = np.random.default_rng(4400)
    special = [cs.I32_MIN, cs.I32_MIN + 1, -1, 0, 1, 16383, 16384, cs.I32_MAX - 1, cs.I32_MAX]
    out = np.zeros(5, np.int32)
    for trial in range(4000):
        e = [int(rng.choice(special)) if rng.random() < 0.3 else int(rng.integers(-600, 1000)) for _ in range(4)]
        w, h = (int(rng.integers(1, 700)), int(rng.integers(1, 700))) if trial % 7 else (16384, 1)
        margin, square = int(rng.choice([0, 1, 250, 999, 1000])), bool(trial & 1)
        host.yfi_crop_region_host(*e, w, h, margin, int(square), out.ctypes.data)
        region = ptq.crop_region(e, w, h, margin, square)
        want = [0, 0, 0, 0, 1] if region is None else list(region) + [0]
        assert out.tolist() == want, (e, w, h, margin, square)
    # the region is not squared again after the clamp
    assert ptq.crop_region((-10, 0, 9, 9), 40, 40, 0, True) == (0, 0, 10, 15)
    assert ptq.crop_region((0, 0, 9, 29), 40, 40, 0, True) == (0, 0, 20, 30)


def test_host_refuses_what_the_device_entries_refuse():
    buf, desc, dets, counts, _ = cs.designed_batch(0)
    ok = dict(out_h=16, out_w=16, margin=0, square=False, order="rgb", chips_cap=4)
    assert cs.host_crop(buf, 0, desc, dets, counts, cs.CAP, **ok)[0] == dets.shape[0]
    for change in (dict(out_h=24), dict(out_w=272), dict(out_h=0), dict(margin=1001), dict(margin=-1), dict(chips_cap=-1)):
        rc, chips, info, first = cs.host_crop(buf, 0, desc, dets, counts, cs.CAP, **dict(ok, **change))
        assert rc == -1 and (chips == 0xA5).all() and (first == -1515870811).all(), change
    lib = cs.crops_host()                                                                 # each entry refuses the other family's formats
    assert lib.yfi_crop_records_host(buf.ctypes.data, buf.nbytes, 4, None, None, None, 0, 1, 16, 16, 1, 0, 0, None, 0, None, None) == -1
    assert lib.yfi_crop_records_yuv_host(buf.ctypes.data, buf.nbytes, 0, None, None, None, 0, 1, 16, 16, 1, 0, 0, None, 0, None, None) == -1
    # the cut falls inside a frame; first still holds the true total
    rc, chips, info, first = cs.host_crop(buf, 0, desc, dets, counts, cs.CAP, 16, 16, 0, False, "rgb", 20)
    assert rc == dets.shape[0] and first[-1] == 67 and first[1] == 13 and (info["frame"][:20] == [0] * 13 + [1] * 7).all()


def test_upscaled_region_and_halved_region(ptq):
    """an 8 x 8 region to 112 x 112, and a 2x reduction (64 x 48 to 32 x 24 is no chip size: 64 x 64 to 32 x 32), against the restatement"""
    rng = np.random.default_rng(4500)
    images = cs._mod("images")
    img = rng.integers(0, 256, (90, 80, 3), dtype=np.uint8)
    key = cs.register(("host", "up"), img)
    dets = np.zeros((1, 2), cs.DET)
    dets[0, 0] = (0, 0, 0, 0, 0, 0.9, 11, 13, 18, 20)                          # 8 x 8
    dets[0, 1] = (0, 0, 0, 0, 0, 0.8, 7, 21, 70, 84)                           # 64 x 64
    counts = np.array([2], np.int32)
    buf, desc = images.pack_images([img], "rgb")
    for out, k in ((112, 0), (32, 1)):
        rc, chips, info, first = cs.host_crop(buf, 1, desc, dets, counts, 2, out, out, 0, False, "rgb", 2)
        want, want_info, _ = cs.expected(dets, counts, 2, [key], out, out, 0, False, "rgb")
        assert rc == 1 and np.array_equal(chips, want) and info.tobytes() == want_info.tobytes()
        d = dets[0, k]
        assert np.array_equal(chips[k], ptq.crop_resize_u8(img, (d["x1"], d["y1"], d["x2"], d["y2"]), out, out))
    # the exact 2x reduction is the rounded mean of each 2 x 2 block (what cv2's switch to INTER_AREA gives)
    blk = img[21:85, 7:71].astype(np.int32).reshape(32, 2, 32, 2, 3).sum(axis=(1, 3))
    assert np.array_equal(chips[1], ((blk + 2) >> 2).astype(np.uint8))
    assert info["width"].tolist() == [8, 64] and info["x0"].tolist() == [11, 7]


def test_the_two_forms_of_the_scale_give_the_same_float32_coordinate():
    """csrc/yf_images_taps.h forms the scale as n_in / n_out, OpenCV as 1 / (n_out / n_in), both in double; the source coordinate
    (float)((d + 0.5) * scale - 0.5) is the same float32 for every output side 1..256, every output index and every input side 1..16384"""
    n_in = np.arange(1, 16385, dtype=np.float64)[:, None]
    for n_out in range(1, 257):
        d = np.arange(n_out, dtype=np.float64)[None, :] + 0.5
        ours = (d * (n_in / n_out) - 0.5).astype(np.float32)
        cv = (d * (1.0 / (n_out / n_in)) - 0.5).astype(np.float32)
        assert np.array_equal(ours, cv), n_out
