"""The IoU suppression of libyf_images on the host (no GPU): the pairwise decision of csrc/yf_images_nms.h -- the same function the device
kernel calls, compiled for the host -- against numpy's float64 arithmetic, the record order key, the restatement of the reference's
non_max_suppression against its literal code, and the argument checks of yf_images_nms_device (which return before any launch).
The restatement itself (`nms_restated`, `nms_reference_literal`) is in tests/images_support.py."""
import os

import numpy as np
import pytest

from conftest import ROOT
from images_support import PKG, host, images, last_error, nms_reference_literal, nms_restated          # noqa: F401 (host, images: fixtures)

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def _pairs_host(lib, a, b, thr):
    a = np.ascontiguousarray(a, np.int32)
    b = np.ascontiguousarray(b, np.int32)
    out = np.empty(a.shape[0], np.uint8)
    area = np.empty((a.shape[0], 2), np.float64)
    lib.yfi_nms_pairs_host(a.ctypes.data, b.ctypes.data, a.shape[0], thr, out.ctypes.data, area.ctypes.data)
    return out.astype(bool), area


def _pairs_numpy(a, b, thr):
    """the reference's arithmetic, vectorised over pairs: box a is the kept one (i), box b the candidate (j)"""
    a = a.astype(np.float64)
    b = b.astype(np.float64)
    area_a = (a[:, 2] - a[:, 0] + 1) * (a[:, 3] - a[:, 1] + 1)
    area_b = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)
    xx1 = np.maximum(a[:, 0], b[:, 0])
    yy1 = np.maximum(a[:, 1], b[:, 1])
    xx2 = np.minimum(a[:, 2], b[:, 2])
    yy2 = np.minimum(a[:, 3], b[:, 3])
    w = np.maximum(0.0, xx2 - xx1 + 1)
    h = np.maximum(0.0, yy2 - yy1 + 1)
    inter = w * h
    union = area_a + area_b - inter
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = inter / union
    return iou <= thr, np.stack([area_a, area_b], axis=1)


def _random_pairs(rng, n):
    """n pairs of boxes from four populations: faces in a 410 x 450 picture (overlaps common), boxes at 2^20 scale, edges anywhere in int32
    (products beyond 2^53, x1 > x2, negative areas), and near-copies of one another"""
    q = n // 4
    xs, ys = np.sort(rng.integers(-20, 460, (q, 2)), axis=1), np.sort(rng.integers(-20, 460, (q, 2)), axis=1)
    small_a = np.stack([xs[:, 0], ys[:, 0], xs[:, 1], ys[:, 1]], 1)
    small_b = small_a + rng.integers(-40, 41, (q, 4))
    big = rng.integers(-(1 << 20), 1 << 20, (q, 4))
    big_b = big + rng.integers(-(1 << 19), 1 << 19, (q, 4))
    wild_a = rng.integers(I32_MIN, I32_MAX, (q, 4), endpoint=True)
    wild_b = rng.integers(I32_MIN, I32_MAX, (q, 4), endpoint=True)
    near = rng.integers(I32_MIN // 2, I32_MAX // 2, (n - 3 * q, 4))
    near_b = near + rng.integers(-3, 4, near.shape)
    a = np.concatenate([small_a, big, wild_a, near]).astype(np.int32)
    b = np.concatenate([small_b, big_b, wild_b, near_b]).astype(np.int32)
    return a, b


@pytest.mark.parametrize("thr", [0.0, 0.4, 0.5, 1.0, 1e300, -0.25, float("inf")])
def test_pairwise_decision_equals_numpy_on_millions_of_pairs(host, thr):
    rng = np.random.default_rng(int(abs(thr) * 1000) % 10007 if np.isfinite(thr) else 99)
    a, b = _random_pairs(rng, 1 << 20)
    got, area = _pairs_host(host, a, b, thr)
    want, area_np = _pairs_numpy(a, b, thr)
    assert np.array_equal(area.view(np.uint64), area_np.view(np.uint64))
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{bad.size} pairs differ, first {a[bad[:3]].tolist()} / {b[bad[:3]].tolist()}"
    # the populations reach what they are for: both outcomes, products above 2^53, x1 > x2, unions <= 0
    assert not got.all() and (got.any() or thr < 0)
    assert (np.abs(area_np) > 2.0 ** 53).any() and (a[:, 0] > a[:, 2]).any()
    assert ((area_np[:, 0] + area_np[:, 1]) <= 0).any()


def test_pairwise_edge_cases(host):
    m, M = I32_MIN, I32_MAX
    cases = [  # (kept box, candidate, {threshold: survives})
        ((0, 0, 9, 9), (0, 0, 9, 9), {0.0: False, 0.4: False, 1.0: True, 1e300: True}),          # identical: iou 1
        ((0, 0, 9, 9), (10, 0, 19, 9), {0.0: True, 0.4: True, 1.0: True}),                         # touching: the +1 makes w = 0
        ((0, 0, 9, 9), (9, 0, 18, 9), {0.0: False, 0.4: True, 1.0: True}),                         # one shared column: iou 10 / 190
        ((0, 0, 9, 9), (100, 100, 109, 109), {0.0: True, 0.4: True}),                              # disjoint
        ((0, 0, 9, 9), (2, 2, 7, 7), {0.0: False, 0.4: True, 1.0: True}),                          # nested: iou 36 / 100
        ((0, 0, 9, 9), (0, 0, 14, 9), {0.4: False, 0.5: False, 1.0: True}),                       # iou 100 / 150
        ((5, 5, 4, 4), (5, 5, 4, 4), {0.0: False, 0.4: False, 1.0: False, 1e300: False}),          # zero areas, zero union: 0 / 0 = NaN
        ((10, 0, 0, 9), (0, 0, 9, 9), {0.0: True, 0.4: True, 1e300: True}),                        # x1 > x2: area -90, inter 0, union 10
        ((10, 0, 0, 9), (10, 0, 0, 9), {0.0: True, 0.4: True, -0.25: False}),                      # negative union: iou 0 / -180 = -0.0
        ((m, m, M, M), (m, m, M, M), {0.4: False, 1.0: True}),                                     # the whole int32 plane: areas 2^64
        ((m, m, M, M), (0, 0, 0, 0), {0.0: False, 0.4: True, 1.0: True}),
        ((m, 0, m, 0), (m, 0, m, 0), {0.4: False, 1.0: True}),                                     # INT32_MIN edges (a PY decode out of range)
        ((M, M, m, m), (M, M, m, m), {0.0: True, 0.4: True, 1e300: True}),                          # area 2^64, inter 0: iou 0
    ]
    a = np.array([c[0] for c in cases], np.int32)
    b = np.array([c[1] for c in cases], np.int32)
    for thr in (0.0, 0.4, 0.5, 1.0, 1e300, -0.25):
        got, _ = _pairs_host(host, a, b, thr)
        want, _ = _pairs_numpy(a, b, thr)
        assert np.array_equal(got, want), thr
        for k, (_, _, exp) in enumerate(cases):
            if thr in exp:
                assert bool(got[k]) == exp[thr], (cases[k][:2], thr)


def test_order_key_is_the_stable_descending_argsort(host):
    rng = np.random.default_rng(4)
    special = np.array([0.0, -0.0, 1.0, 1.0, np.inf, -np.inf, np.nan, -np.nan, 0.7000001, 1e-45, -1e-45, -3.0], np.float32)
    for trial in range(200):
        k = int(rng.integers(1, 256))
        pool = np.concatenate([special, rng.choice(np.float32([0.71, 0.8, 0.9, 0.99, 1.0]), 8), rng.standard_normal(8).astype(np.float32)])
        conf = rng.choice(pool, k)
        keys = np.array([host.yfi_nms_key_host(int(c), i) for i, c in enumerate(conf.view(np.uint32))], np.uint64)
        assert len(set(keys.tolist())) == k
        got = np.argsort(keys)[::-1]
        want = np.argsort(conf.astype(np.float64), kind="stable")[::-1]
        assert np.array_equal(got, want), (trial, conf[got], conf[want])


def test_restatement_equals_the_reference_code_on_distinct_confidences():
    rng = np.random.default_rng(8)
    for trial in range(400):
        k = int(rng.integers(0, 148))
        conf = rng.permutation(np.linspace(0.7, 1.0, 300, dtype=np.float32))[:k]       # distinct
        cx, cy = rng.integers(0, 410, k), rng.integers(0, 450, k)
        bw, bh = rng.integers(5, 80, k), rng.integers(5, 80, k)
        boxes = [[int(cx[j] - bw[j]), int(cy[j] - bh[j]), int(cx[j] + bw[j]), int(cy[j] + bh[j]), float(conf[j])] for j in range(k)]
        for thr in (0.0, 0.4, 1.0):
            assert nms_restated(boxes, thr) == nms_reference_literal(boxes, thr), (trial, thr)
    # with ties the two may differ; the restatement's tie rule: later record first
    tie = [[0, 0, 9, 9, 0.9], [0, 0, 9, 9, 0.9], [50, 50, 59, 59, 0.8]]
    assert nms_restated(tie, 0.4) == [1, 2]


def test_nms_entry_checks_every_argument_before_any_launch(images):
    lib = images.load()
    D, C, O, OC = 0x10000, 0x20000, 0x30000, 0x40000                    # never dereferenced: every call below fails its host checks
    good = dict(dets=D, counts=C, n=4, cap=147, thr=0.4, out=O, out_counts=OC)

    def nms(**kw):
        a = dict(good, **kw)
        rc = lib.yf_images_nms_device(a["dets"], a["counts"], a["n"], a["cap"], a["thr"], a["out"], a["out_counts"], None)
        return rc, last_error(lib)

    cases = [
        (dict(n=-1), "n < 0"), (dict(cap=0), "cap must be"), (dict(cap=-3), "cap must be"), (dict(cap=images.NMS_MAX_CAP + 1), "cap must be"),
        (dict(thr=float("nan")), "NaN"), (dict(dets=None), "d_dets is NULL"), (dict(counts=None), "d_counts is NULL"),
        (dict(out=None), "d_out is NULL"), (dict(out_counts=None), "d_out_counts is NULL"), (dict(dets=D + 2), "d_dets is not 4-byte"),
        (dict(out=O + 1), "d_out is not 4-byte"), (dict(counts=C + 2), "d_counts or d_out_counts"), (dict(out_counts=OC + 3), "d_counts or d_out_counts"),
    ]
    texts = set()
    for kw, word in cases:
        rc, text = nms(**kw)
        assert rc <= 0 and word in text, (kw, rc, text)
        texts.add(text)
    assert len(texts) == 10                               # one text per kind of fault
    # the NaN check is on the value, not on a bit pattern: any other double is a threshold
    rc, text = nms(thr=-float("nan"), n=-1)
    assert "n < 0" in text
    # n = 0 is a valid empty batch: nothing is launched (no GPU here), whatever the threshold
    for thr in (0.0, 0.4, 1.0, 1e300, -1.0, float("inf")):
        assert nms(n=0, thr=thr)[0] == 0
    assert nms(n=0, cap=images.NMS_MAX_CAP)[0] == 0
    # and the Python wrapper raises with the library's text
    with pytest.raises(images.ImagesError, match="NaN"):
        images.nms_device(D, C, 4, 147, float("nan"))


def test_suppression_is_part_of_the_companion_library_only(images):
    """the new source is covered by the images build id and stays out of the network's"""
    flags = open(os.path.join(PKG, "csrc", "flags.mk")).read()
    assert "yf_images_nms.h" in images._images_srcs() and "yf_images_nms.h" not in flags
    lib = images.load()
    assert (lib.yf_images_build_id() or b"").decode() == images.expected_build_id()
    assert "yf_images_nms_device" in open(os.path.join(ROOT, "include", "yf_images.h")).read()
    assert "yf_images_nms_device" not in open(os.path.join(ROOT, "include", "yf_network.h")).read()
