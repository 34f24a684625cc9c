"""What the tests of the scoring in libyf_images share (test_eval_host, test_eval_gpu): the project's own statement, in plain Python, of
the reference's calculate_iou / calculate_ap / calculate_map (yoloface/tensorflow/yolov3_train_tf.py:657-759) -- Python's own max and min,
float64, the loops the reference has -- a variant of it in two halves that also returns the flags, the best indices and the curve, the
prototypes of the host build, and the builders of records and ground truths.

The order of the detections is a stable list.sort(..., reverse=True) by confidence: what the reference's comment at :712 says and what
the library does.  The reference's line 713 itself reads `x[4]` of a tuple that carries the image id in front of the five values of a
prediction, which is the box's y2, not its confidence; `calculate_map(..., sort_index=3)` states the line as written, the default
(`sort_index=4`) the confidence, and tests/test_eval_host.py pins both against the reference (the two agree wherever the confidences
order as the y2 do).  Python does not define the sort for a NaN confidence; the library's choice (csrc/yf_images_eval.h) is "NaN after
every number", and `order_key` states that choice, so that the statement below and the library can be compared on NaN too.  Without NaN
`order_key` orders exactly as the value itself does."""
import ctypes
import math

import numpy as np

from images_support import host_lib

GT = np.dtype([("x1", "<f8"), ("y1", "<f8"), ("x2", "<f8"), ("y2", "<f8")])
RESULT = np.dtype([("ap", "<f8"), ("detections", "<i8"), ("ground_truths", "<i8"), ("true_positives", "<i8")])


# ---- the statement ----
def calculate_iou(det, truth):
    """overlap over union of [x1, y1, x2, y2] boxes; no + 1 anywhere"""
    left = max(det[0], truth[0])
    top = max(det[1], truth[1])
    right = min(det[2], truth[2])
    bottom = min(det[3], truth[3])
    overlap = max(0, right - left) * max(0, bottom - top)
    det_area = (det[2] - det[0]) * (det[3] - det[1])
    truth_area = (truth[2] - truth[0]) * (truth[3] - truth[1])
    total = det_area + truth_area - overlap
    return overlap / total if total > 0 else 0.0


def calculate_ap(recall, precision):
    """precision made non-increasing from the back (in place), then the steps of recall times it, from index 1"""
    for k in range(len(precision) - 2, -1, -1):
        precision[k] = max(precision[k], precision[k + 1])
    area = 0.0
    for k in range(1, len(recall)):
        area += (recall[k] - recall[k - 1]) * precision[k]
    return area


def order_key(conf):
    """sort key with reverse=True: numbers by value, every NaN behind them"""
    return (0, 0.0) if math.isnan(conf) else (1, conf)


def calculate_map(predictions, ground_truths, iou_threshold=0.5, sort_index=4):
    """predictions: per image a list of [x1, y1, x2, y2, conf]; ground_truths: per image a list of [x1, y1, x2, y2]; sort_index: the
    value of a prediction the detections are ordered by (4: the confidence; 3: what the reference's line 713 reads)"""
    dets, truths = [], []
    for image, (preds, gts) in enumerate(zip(predictions, ground_truths)):
        for p in preds:
            dets.append((image, p[0], p[1], p[2], p[3], p[4]))
        for g in gts:
            truths.append((image, g[0], g[1], g[2], g[3]))
    dets.sort(key=lambda d: order_key(d[1 + sort_index]), reverse=True)
    hits = np.zeros(len(dets))
    misses = np.zeros(len(dets))
    used = set()
    for k, (image, x1, y1, x2, y2, _) in enumerate(dets):
        mine = [t for t in truths if t[0] == image]
        best_iou = 0
        best = -1
        for j, (_, gx1, gy1, gx2, gy2) in enumerate(mine):
            iou = calculate_iou([x1, y1, x2, y2], [gx1, gy1, gx2, gy2])
            if iou > best_iou:
                best_iou = iou
                best = j
        if best_iou >= iou_threshold and best >= 0:
            if (image, best) not in used:
                used.add((image, best))
                hits[k] = 1
            else:
                misses[k] = 1
        else:
            misses[k] = 1
    chits = np.cumsum(hits)
    cmisses = np.cumsum(misses)
    precision = chits / (chits + cmisses + 1e-16)
    recall = chits / max(1, len(truths))
    return calculate_ap(recall, precision)


# ---- the same in two halves, with everything the library reports ----
def match_restated(predictions, ground_truths, iou_threshold):
    """-> (tp, best, stats): per image the flag and the best ground truth's index of every record, in record order; stats counts the
    records that met an equal best IoU again at a later ground truth ("ties") and the candidates whose ground truth was taken ("taken")"""
    dets = [(image, slot, p) for image, preds in enumerate(predictions) for slot, p in enumerate(preds)]
    dets.sort(key=lambda d: order_key(d[2][4]), reverse=True)
    tp = [[0] * len(p) for p in predictions]
    best_of = [[-1] * len(p) for p in predictions]
    used = set()
    stats = {"ties": 0, "taken": 0, "candidates": 0}
    for image, slot, p in dets:
        best_iou = 0
        best = -1
        tied = False
        for j, g in enumerate(ground_truths[image]):
            iou = calculate_iou([p[0], p[1], p[2], p[3]], [g[0], g[1], g[2], g[3]])
            if iou > best_iou:
                best_iou = iou
                best = j
                tied = False
            elif best >= 0 and iou == best_iou:
                tied = True
        stats["ties"] += tied
        best_of[image][slot] = best
        if best_iou >= iou_threshold and best >= 0:
            stats["candidates"] += 1
            if (image, best) not in used:
                used.add((image, best))
                tp[image][slot] = 1
            else:
                stats["taken"] += 1
    return tp, best_of, stats


def ap_restated(confs, tp, num_gt):
    """confs, tp: per image, in record order -> (ap, curve float64 [m, 2] = (recall, envelope precision), true positives)"""
    flat = [(c, t) for cs, ts in zip(confs, tp) for c, t in zip(cs, ts)]
    flat.sort(key=lambda e: order_key(e[0]), reverse=True)
    hits = np.array([float(t != 0) for _, t in flat])
    misses = 1.0 - hits
    chits = np.cumsum(hits)
    cmisses = np.cumsum(misses)
    precision = chits / (chits + cmisses + 1e-16)
    recall = chits / max(1, num_gt)
    ap = calculate_ap(recall, precision)
    return float(ap), np.stack([recall, precision], axis=1).reshape(-1, 2), int(hits.sum())


def score_restated(predictions, ground_truths, iou_threshold):
    """the whole evaluation -> dict(ap, detections, ground_truths, true_positives, tp, best, curve, stats)"""
    tp, best, stats = match_restated(predictions, ground_truths, iou_threshold)
    num_gt = sum(len(g) for g in ground_truths)
    ap, curve, hits = ap_restated([[p[4] for p in preds] for preds in predictions], tp, num_gt)
    return dict(ap=ap, detections=sum(len(p) for p in predictions), ground_truths=num_gt, true_positives=hits, tp=tp, best=best,
                curve=curve, stats=stats)


# ---- records and ground truths as the library takes them, and as the statement does ----
def clamp(count, cap):
    return min(max(int(count), 0), cap)


def predictions_of(dets, counts, cap):
    """DET_DTYPE [n, cap], counts -> per image [x1, y1, x2, y2, conf] with Python ints for the edges (exact, as the library converts
    them) and the float32 confidence as a Python float"""
    out = []
    for f in range(dets.shape[0]):
        r = dets[f, :clamp(counts[f], cap)]
        out.append([[int(a), int(b), int(c), int(d), float(e)] for a, b, c, d, e in zip(r["x1"], r["y1"], r["x2"], r["y2"], r["conf"])])
    return out


def truths_of(gt, gt_counts, gt_cap):
    """GT [n, gt_cap], counts -> per image [x1, y1, x2, y2] floats"""
    return [[[float(v) for v in row] for row in gt[f, :clamp(gt_counts[f], gt_cap)].tolist()] for f in range(gt.shape[0])]


def pad_flags(lists, cap, fill, dtype):
    """per-image lists -> [n, cap] with `fill` beyond each list"""
    out = np.full((len(lists), cap), fill, dtype)
    for f, row in enumerate(lists):
        out[f, :len(row)] = row
    return out


def truths_near(rng, dets, counts, cap, gt_cap, gt_counts):
    """GT [n, gt_cap] drawn from each frame's own records: an exact copy (IoU 1; two copies of one record tie), the record twice as wide
    (IoU exactly 0.5) and one pixel more or less than that (just under, just over), a shifted copy, a random box; frames without records
    get random boxes.  Rows beyond the count are filled too (they must not be read)."""
    n = dets.shape[0]
    gt = np.zeros((n, gt_cap), GT)
    for f in range(n):
        m = clamp(counts[f], cap)
        rows = np.zeros((gt_cap, 4))
        for j in range(gt_cap):
            kind = rng.integers(0, 7)
            if m == 0 or kind == 6:
                x, y = rng.integers(-50, 500, 2)
                rows[j] = (x, y, x + rng.integers(1, 200), y + rng.integers(1, 200))
                continue
            # a duplicate of the previous ground truth now and then: equal best IoUs, the first one wins
            if j > 0 and rng.random() < 0.15:
                rows[j] = rows[j - 1]
                continue
            r = dets[f, rng.integers(0, m)]
            x1, y1, x2, y2 = float(r["x1"]), float(r["y1"]), float(r["x2"]), float(r["y2"])
            w = x2 - x1
            if kind == 0:
                rows[j] = (x1, y1, x2, y2)
            elif kind == 1:
                rows[j] = (x1, y1, x2 + w, y2)
            elif kind == 2:
                rows[j] = (x1, y1, x2 + w + 1, y2)
            elif kind == 3:
                rows[j] = (x1, y1, x2 + w - 1, y2)
            elif kind == 4:
                rows[j] = (x1 + rng.integers(-9, 10), y1 + rng.integers(-9, 10), x2 + rng.integers(-9, 10), y2 + rng.integers(-9, 10))
            else:
                rows[j] = (x1 + 0.25 * w, y1, x2 + 0.25 * w, y2)
        gt[f] = np.ascontiguousarray(rows).view(GT).reshape(-1)
    return gt


def spread(rng, m, n, cap):
    """n counts in [0, cap] that add up to m"""
    assert 0 <= m <= n * cap
    counts = np.zeros(n, np.int64)
    left = m
    for f in rng.permutation(n):
        counts[f] = rng.integers(0, min(cap, left) + 1)
        left -= counts[f]
    if left:                                        # top up wherever there is room
        for f in range(n):
            add = min(cap - counts[f], left)
            counts[f] += add
            left -= add
    assert counts.sum() == m and counts.max(initial=0) <= cap
    return counts.astype(np.int32)


# ---- the host build ----
def eval_host():
    """libyf_images_host.so with the prototypes of the scoring set"""
    lib = host_lib()
    vp, cl, ci = ctypes.c_void_p, ctypes.c_long, ctypes.c_int
    lib.yfi_eval_iou_host.restype = None
    lib.yfi_eval_iou_host.argtypes = [vp, vp, cl, vp]
    lib.yfi_eval_key_host.restype = ctypes.c_uint32
    lib.yfi_eval_key_host.argtypes = [ctypes.c_uint32]
    lib.yfi_eval_match_host.restype = cl
    lib.yfi_eval_match_host.argtypes = [vp, vp, cl, ci, vp, vp, ci, ctypes.c_double, vp, vp]
    lib.yfi_eval_ap_host.restype = cl
    lib.yfi_eval_ap_host.argtypes = [vp, vp, vp, cl, ci, vp, ci, vp, vp]
    return lib


def host_score(lib, dets, counts, cap, gt, gt_counts, gt_cap, thr, tp_in=None):
    """match and average precision of the host build -> dict like score_restated's, tp and best as [n, cap] with -9 beyond the records
    (tp_in: flags to score instead of the match's)"""
    n = dets.shape[0]
    dets, counts = np.ascontiguousarray(dets), np.ascontiguousarray(counts, np.int32)
    gt, gt_counts = np.ascontiguousarray(gt), np.ascontiguousarray(gt_counts, np.int32)
    tp = np.full((n, cap), 0xA5, np.uint8)
    best = np.full((n, cap), -9, np.int32)
    assert lib.yfi_eval_match_host(dets.ctypes.data, counts.ctypes.data, n, cap, gt.ctypes.data, gt_counts.ctypes.data, gt_cap, thr,
                                   tp.ctypes.data, best.ctypes.data) == n
    flags = tp if tp_in is None else np.ascontiguousarray(tp_in, np.uint8)
    res = np.zeros(1, RESULT)
    curve = np.full((max(n * cap, 1), 2), -9.0)
    assert lib.yfi_eval_ap_host(dets.ctypes.data, counts.ctypes.data, flags.ctypes.data, n, cap, gt_counts.ctypes.data, gt_cap,
                                res.ctypes.data, curve.ctypes.data) == n
    return dict(ap=float(res["ap"][0]), detections=int(res["detections"][0]), ground_truths=int(res["ground_truths"][0]),
                true_positives=int(res["true_positives"][0]), tp=tp, best=best, curve=curve)


def same_bits(a, b):
    return np.asarray(a, np.float64).tobytes() == np.asarray(b, np.float64).tobytes()


def check_against_restatement(got, dets, counts, cap, gt, gt_counts, gt_cap, thr, tp_fill=0xA5, best_fill=-9, curve_fill=-9.0):
    """a dict like host_score's (from the host build or from the device) equals the statement: flags and best indices with their fill
    beyond the records, counts, the bits of ap and of the curve; returns the statement's dict"""
    want = score_restated(predictions_of(dets, counts, cap), truths_of(gt, gt_counts, gt_cap), thr)
    assert np.array_equal(got["tp"], pad_flags(want["tp"], cap, tp_fill, np.uint8))
    if got.get("best") is not None:
        assert np.array_equal(got["best"], pad_flags(want["best"], cap, best_fill, np.int32))
    check_result(got, want, curve_fill)
    return want


def check_result(got, want, curve_fill=-9.0):
    for k in ("detections", "ground_truths", "true_positives"):
        assert got[k] == want[k], (k, got[k], want[k])
    assert same_bits(got["ap"], want["ap"]), (got["ap"], want["ap"])
    if got.get("curve") is not None:
        m = want["detections"]
        assert same_bits(got["curve"][:m], want["curve"]), "curve"
        assert (got["curve"][m:] == curve_fill).all()
