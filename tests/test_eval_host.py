"""The scoring of libyf_images on the host (no GPU): the arithmetic of csrc/yf_images_eval.h -- the same functions the device kernels call,
built into libyf_images_host.so -- against the plain-Python statement of tests/eval_support.py, bit for bit; that statement against the
reference's own three functions where the reference tree exists; the order key; the argument checks of the two device entry points,
which run before anything touches a GPU."""
import ast
import ctypes
import os

import numpy as np
import pytest

import eval_support as es
from conftest import REFERENCE, ROOT, has_reference
from images_support import PKG, last_error
from images_support import images                                         # noqa: F401 (fixture)

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
REF_SCRIPT = os.path.join(REFERENCE, "yoloface", "tensorflow", "yolov3_train_tf.py")


@pytest.fixture(scope="module")
def host():
    return es.eval_host()


@pytest.fixture(scope="module")
def det_dtype(yf):
    return yf.DET_DTYPE


def _random_case(rng, k, conf_of_y2=False):
    """a small evaluation for the pin against the reference: few distinct confidences (ties), empty frames, frames without ground truth,
    duplicate boxes, 0, 1 and 2 detections in all.  conf_of_y2: every confidence is an increasing function of its box's y2 (ties where
    the y2 tie), so ordering by either is the same order"""
    n = int(rng.integers(1, 5))
    total = [0, 1, 2][k % 7] if k % 7 < 3 else None
    preds, gts = [], []
    for f in range(n):
        m = int(rng.integers(0, 7)) if total is None else (total if f == 0 else 0)
        g = int(rng.integers(0, 5)) if k % 5 else 0
        boxes = []
        for _ in range(m):
            x, y = rng.integers(0, 40, 2)
            boxes.append([int(x), int(y), int(x + rng.integers(-2, 30)), int(y + rng.integers(-2, 30)),
                          float(np.float32(rng.choice([0.71, 0.8, 0.9, 1.0, rng.random()])))])
        if m > 1 and rng.random() < 0.4:
            boxes[1][:4] = boxes[0][:4]
        if conf_of_y2:
            for b in boxes:
                b[4] = float(np.float32(0.7 + (b[3] // 4 + 2) / 64.0))          # y2 in [-2, 68]; steps of 4 tie
                b[3] = b[3] // 4 * 4
        truth = []
        for j in range(g):
            if boxes and rng.random() < 0.6:
                b = boxes[int(rng.integers(0, len(boxes)))]
                d = rng.choice([0.0, 0.0, 1.0, 2.5, -3.0])
                truth.append([b[0] + d, float(b[1]), b[2] + d, float(b[3])])
            else:
                x, y = rng.integers(0, 40, 2)
                truth.append([float(x), float(y), float(x + rng.integers(1, 30)), float(y + rng.integers(1, 30))])
            if j > 0 and rng.random() < 0.3:
                truth[j] = list(truth[j - 1])
        preds.append(boxes)
        gts.append(truth)
    return preds, gts


@pytest.mark.skipif(not has_reference(), reason="the reference tree is not here")
def test_the_statement_equals_the_references_three_functions():
    """calculate_iou, calculate_ap and calculate_map are taken out of the reference's training script as FunctionDef nodes (the module
    imports TensorFlow and cannot be imported), executed with numpy in their namespace and compared with the statement: equal ap.
    The reference's line 713 orders the detections by `x[4]` of (image, x1, y1, x2, y2, conf), which is y2, under a comment that says
    confidence.  Every case is compared with the statement of the line as written (sort_index=3); every second case is built so that the
    confidences order exactly as the y2 do, and there the reference also equals the statement the library follows (by confidence)."""
    tree = ast.parse(open(REF_SCRIPT, encoding="utf-8").read())
    wanted = ("calculate_iou", "calculate_ap", "calculate_map")
    nodes = [nd for nd in tree.body if isinstance(nd, ast.FunctionDef) and nd.name in wanted]
    assert sorted(nd.name for nd in nodes) == sorted(wanted)
    ns = {"np": np}
    exec(compile(ast.Module(body=nodes, type_ignores=[]), REF_SCRIPT, "exec"), ns)
    rng = np.random.default_rng(2024)
    seen, positive, ties = set(), 0, 0
    for k in range(400):
        preds, gts = _random_case(rng, k, conf_of_y2=k % 2 == 1)
        thr = [0.5, 0.5, 0.3, 0.75, 1.0, 0.0][k // 2 % 6]
        # the reference reads a class at index 5 of a ground-truth row and ignores it
        ref = ns["calculate_map"]([list(p) for p in preds], [[g + [1.0, 0.0] for g in gg] for gg in gts], thr)
        assert es.same_bits(ref, es.calculate_map(preds, gts, thr, sort_index=3)), (k, ref)
        mine = es.calculate_map(preds, gts, thr)
        whole = es.score_restated(preds, gts, thr)
        assert es.same_bits(whole["ap"], mine), k
        if k % 2 == 1:
            assert es.same_bits(ref, mine), (k, ref, mine)
            seen.add(min(whole["detections"], 3))
            positive += mine > 0
            ties += len({p[4] for pp in preds for p in pp}) < whole["detections"]
        for _ in range(3):
            a, b = rng.integers(-5, 30, 4).tolist(), (rng.integers(-10, 60, 4) / 2.0).tolist()
            assert es.same_bits(ns["calculate_iou"](a, b), es.calculate_iou(a, b))
    assert seen == {0, 1, 2, 3} and positive >= 20 and ties >= 20
    # nothing of the reference is written anywhere: the functions lived in `ns` only


def _special_batch(det_dtype, rng, n, cap, gt_cap):
    """records and ground truths with everything the arithmetic can meet: edges at the int32 limits, boxes with x1 > x2, ground-truth rows
    with inf and NaN, confidences -0.0, 0.0, 1.0 repeated and NaN, counts below zero and above the caps"""
    recs = np.zeros((n, cap), det_dtype)
    recs["frame"] = np.arange(n)[:, None]
    recs["conf"] = rng.choice(np.float32([-0.0, 0.0, 1.0, 1.0, 1.0, 0.9, 0.8, np.nan, -2.5, np.inf, 0.71]), (n, cap))
    cx, cy = rng.integers(0, 120, (n, cap)), rng.integers(0, 120, (n, cap))
    recs["x1"], recs["y1"] = cx, cy
    recs["x2"], recs["y2"] = cx + rng.integers(-3, 40, (n, cap)), cy + rng.integers(-3, 40, (n, cap))
    lim = rng.random((n, cap))
    for name, p in (("x1", 0.03), ("y1", 0.06), ("x2", 0.09), ("y2", 0.12)):
        pick = (lim > p - 0.03) & (lim < p)
        recs[name][pick] = rng.choice([I32_MIN, I32_MAX], int(pick.sum()))
    counts = rng.integers(0, cap + 1, n).astype(np.int32)
    counts[1::7] = -3
    counts[2::7] = cap + 1000
    counts[3::7] = cap
    gt_counts = rng.integers(0, gt_cap + 1, n).astype(np.int32)
    gt_counts[0::5] = -1
    gt_counts[1::5] = gt_cap + 9
    gt = es.truths_near(rng, recs, counts, cap, gt_cap, gt_counts)
    rows = gt.view(np.float64).reshape(n, gt_cap, 4)
    odd = rng.random((n, gt_cap))
    rows[odd < 0.05, 2] = np.inf
    rows[(odd >= 0.05) & (odd < 0.08), 0] = -np.inf
    rows[(odd >= 0.08) & (odd < 0.12), int(rng.integers(0, 4))] = np.nan
    rows[(odd >= 0.12) & (odd < 0.14)] = (-np.inf, -np.inf, np.inf, np.inf)
    swap = (odd >= 0.14) & (odd < 0.18)
    rows[swap] = rows[swap][:, [2, 1, 0, 3]]
    return recs, counts, gt, gt_counts


@pytest.mark.parametrize("thr", [0.0, 0.5, 1.0, -1.0])
def test_host_build_equals_the_statement_bit_for_bit(host, det_dtype, thr):
    cap, gt_cap, n = 40, 9, 60
    recs, counts, gt, gt_counts = _special_batch(det_dtype, np.random.default_rng(int(thr * 10) + 50), n, cap, gt_cap)
    got = es.host_score(host, recs, counts, cap, gt, gt_counts, gt_cap, thr)
    want = es.check_against_restatement(got, recs, counts, cap, gt, gt_counts, gt_cap, thr)
    assert want["detections"] > 500 and want["ground_truths"] > 100
    if thr == 0.5:
        assert want["stats"]["ties"] > 0 and want["stats"]["taken"] > 0 and 0 < want["true_positives"] < want["stats"]["candidates"]
    if thr == -1.0:
        # a record without any overlap is no candidate even below threshold 0
        assert any(b == -1 for row in want["best"] for b in row)
        assert want["true_positives"] <= sum(b >= 0 for row in want["best"] for b in row)


def test_host_iou_pairs_at_the_limits(host):
    rng = np.random.default_rng(8)
    n = 4000
    d = rng.integers(-60, 60, (n, 4)).astype(np.int32)
    d[rng.random((n, 4)) < 0.1] = I32_MIN
    d[rng.random((n, 4)) < 0.1] = I32_MAX
    g = rng.integers(-120, 120, (n, 4)) / 2.0
    g[rng.random((n, 4)) < 0.05] = np.inf
    g[rng.random((n, 4)) < 0.05] = -np.inf
    g[rng.random((n, 4)) < 0.05] = np.nan
    g[rng.random((n, 4)) < 0.05] = 2.0 ** 62
    g[::9] = d[::9]                                                          # the same box: IoU 1 wherever its area is positive
    out = np.zeros(n)
    host.yfi_eval_iou_host(np.ascontiguousarray(d).ctypes.data, np.ascontiguousarray(g).ctypes.data, n, out.ctypes.data)
    want = np.array([es.calculate_iou([int(v) for v in d[k]], [float(v) for v in g[k]]) for k in range(n)], np.float64)
    assert es.same_bits(out, want)
    assert (want == 1.0).any() and (want == 0.0).any() and ((want > 0) & (want < 1)).any()      # (no NaN: a union that is not > 0 gives 0.0)


def test_order_key(host):
    """ascending key = descending confidence, -0.0 with +0.0, NaN (any payload, either sign) behind every number"""
    conf = np.float32([np.inf, 3.0e38, 1.0, 0.999, 0.7, 1e-45, 0.0, -0.0, -1e-45, -1.0, -np.inf])
    keys = [host.yfi_eval_key_host(int(b)) for b in conf.view(np.uint32)]
    assert keys[6] == keys[7]
    assert keys == sorted(keys) and len(set(keys)) == len(keys) - 1
    nans = [0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF]
    assert all(host.yfi_eval_key_host(b) == 0xFFFFFFFF for b in nans) and keys[-1] < 0xFFFFFFFF
    rng = np.random.default_rng(3)
    bits = rng.integers(0, 2 ** 32, 5000, dtype=np.uint64).astype(np.uint32)
    vals = [float(v) for v in bits.view(np.float32)]
    mine = sorted(range(len(vals)), key=lambda i: host.yfi_eval_key_host(int(bits[i])))
    want = sorted(range(len(vals)), key=lambda i: es.order_key(vals[i]), reverse=True)
    assert mine == want


def test_argument_checks_before_any_launch(images):
    """every fault is refused with its own text and nothing is launched (there is no GPU here); n = 0 is a valid empty batch"""
    lib = images.load()
    D, C, G, GC, TP, B, W, R, CV = (0x1000 * k for k in range(1, 10))
    need = images.average_precision_workspace(4, 147)
    assert need > 0 and images.average_precision_workspace(300, 1200) > need
    for bad in ((-1, 147), (4, 0), (4, images.NMS_WIDE_MAX_CAP + 1), (2 ** 31 // 147 + 1, 147)):
        assert images.average_precision_workspace(*bad) == 0

    def match(**kw):
        a = dict(dict(dets=D, counts=C, n=4, cap=147, gt=G, gt_counts=GC, gt_cap=8, thr=0.5, tp=TP, best=B), **kw)
        rc = lib.yf_images_match_device(a["dets"], a["counts"], a["n"], a["cap"], a["gt"], a["gt_counts"], a["gt_cap"], a["thr"], a["tp"],
                                        a["best"], None)
        return rc, last_error(lib)

    def ap(**kw):
        a = dict(dict(dets=D, counts=C, tp=TP, n=4, cap=147, gt_counts=GC, gt_cap=8, work=W, bytes=need, res=R, curve=CV), **kw)
        rc = lib.yf_images_average_precision_device(a["dets"], a["counts"], a["tp"], a["n"], a["cap"], a["gt_counts"], a["gt_cap"], a["work"],
                                                    a["bytes"], a["res"], a["curve"], None)
        return rc, last_error(lib)

    shared = [(dict(n=-1), "n < 0"), (dict(cap=0), "cap must be"), (dict(cap=images.NMS_WIDE_MAX_CAP + 1), "cap must be"),
              (dict(gt_cap=0), "gt_cap must be"), (dict(gt_cap=images.EVAL_MAX_GT + 1), "gt_cap must be"), (dict(dets=None), "d_dets is NULL"),
              (dict(counts=None), "d_counts is NULL"), (dict(gt_counts=None), "d_gt_counts is NULL"), (dict(dets=D + 2), "d_dets is not 4-byte"),
              (dict(counts=C + 1), "d_counts or d_gt_counts"), (dict(gt_counts=GC + 2), "d_counts or d_gt_counts"), (dict(tp=None), "d_tp is NULL")]
    for kw, word in shared + [(dict(thr=float("nan")), "NaN"), (dict(gt=None), "d_gt is NULL"), (dict(gt=G + 4), "d_gt is not 8-byte"),
                              (dict(best=B + 2), "d_best is not 4-byte")]:
        rc, text = match(**kw)
        assert rc <= 0 and word in text, (kw, rc, text)
    for kw, word in shared + [(dict(n=2 ** 31 // 147 + 1), "2^31"), (dict(work=None), "d_work"), (dict(work=W + 8), "d_work"),
                              (dict(res=None), "d_result"), (dict(res=R + 4), "d_result"), (dict(curve=CV + 4), "d_curve"),
                              (dict(bytes=need - 1), "work_bytes"), (dict(bytes=0), "work_bytes")]:
        rc, text = ap(**kw)
        assert rc <= 0 and word in text, (kw, rc, text)
    assert str(need) in ap(bytes=need - 1)[1]
    # an empty batch launches nothing, whatever the threshold; the optional outputs may be NULL
    for thr in (0.0, 0.5, 1.0, -1.0, float("inf")):
        assert match(n=0, thr=thr)[0] == 0
    assert match(n=0, best=None)[0] == 0 and ap(n=0, curve=None, bytes=images.average_precision_workspace(0, 147))[0] == 0
    with pytest.raises(images.ImagesError, match="NaN"):
        images.match_device(D, C, 4, 147, G, GC, 8, float("nan"), TP)
    with pytest.raises(images.ImagesError, match="work_bytes"):
        images.average_precision_device(D, C, TP, 4, 147, GC, 8, W, need - 16, R)


def test_scoring_is_part_of_the_companion_library_only(images):
    """the new sources are covered by the images build id and stay out of the network's; the binding's constants are the header's"""
    flags = open(os.path.join(PKG, "csrc", "flags.mk")).read()
    for src in ("yf_images_eval.h", "yf_images_eval.hip.h"):
        assert src in images._images_srcs() and src not in flags
    lib = images.load()
    assert (lib.yf_images_build_id() or b"").decode() == images.expected_build_id()
    header = open(os.path.join(ROOT, "include", "yf_images.h")).read()
    network_header = open(os.path.join(ROOT, "include", "yf_network.h")).read()
    for name in ("yf_images_match_device", "yf_images_average_precision_device", "yf_images_average_precision_workspace"):
        assert name in header and name not in network_header and hasattr(lib, name)
    assert f"#define YF_IMAGES_EVAL_SORT_TILE {images.EVAL_SORT_TILE}" in header and lib.yf_images_eval_sort_tile() == images.EVAL_SORT_TILE
    assert f"#define YF_IMAGES_EVAL_MAX_GT {images.EVAL_MAX_GT}" in header
    assert images.GT_DTYPE == es.GT and images.EVAL_RESULT_DTYPE == es.RESULT and images.GT_DTYPE.itemsize == ctypes.sizeof(ctypes.c_double) * 4


def test_pack_ground_truths(images):
    gt, counts = images.pack_ground_truths([np.zeros((0, 4)), [[1, 2, 3, 4]], np.arange(12).reshape(3, 4)])
    assert gt.shape == (3, 3) and gt.dtype == images.GT_DTYPE and counts.tolist() == [0, 1, 3]
    assert gt[2, 1].tolist() == (4.0, 5.0, 6.0, 7.0) and gt[1, 0].tolist() == (1.0, 2.0, 3.0, 4.0)
    assert images.pack_ground_truths([[], []])[0].shape == (2, 1)
    with pytest.raises(ValueError, match="at most"):
        images.pack_ground_truths([np.zeros((images.EVAL_MAX_GT + 1, 4))])
