"""Scoring of detection records against ground truth on the MI355X (yf_images_match_device, yf_images_average_precision_device,
images.evaluate): flags, best indices, counts, the curve and the bits of the average precision equal the plain-Python statement of the
reference's calculate_iou / calculate_ap / calculate_map (tests/eval_support.py) -- on seeded synthetic heads against ground truths drawn
near the records' own boxes, on hand-built counts around the 64-record pass, at cap 1200, around the sort's tile size, under pure ties,
captured in a graph, and through images.evaluate() on the reference's 27 images at both frame sizes and on the fp16 network."""
import numpy as np
import pytest

import eval_support as es
from float_support import F16Batch
from images_support import Batch, expect_frame, real_images, suppress, synthetic_heads, synthetic_heads160, to_host, tuples
from images_support import images_after_network, ptq, torch_cuda          # noqa: F401 (fixtures; `images` is images_after_network)

pytestmark = pytest.mark.gpu

CAP = 147


class Run:
    """one batch on the device: the inputs, sentinels in every output (flags 0xA5, best -9, curve -9.0, result -9.0), the workspace"""

    def __init__(self, torch, images, dets, counts, cap, gt, gt_counts, gt_cap):
        self.torch, self.images, self.n, self.cap, self.gt_cap = torch, images, dets.shape[0], cap, gt_cap
        n = max(self.n, 1)
        self.d_dets = torch.from_numpy(np.ascontiguousarray(dets).view(np.uint8).reshape(-1, cap, 28).copy()).cuda()
        self.d_counts = torch.from_numpy(np.ascontiguousarray(counts, np.int32)).cuda()
        self.d_gt = torch.from_numpy(np.ascontiguousarray(gt).view(np.float64).reshape(-1, gt_cap, 4).copy()).cuda()
        self.d_gt_counts = torch.from_numpy(np.ascontiguousarray(gt_counts, np.int32)).cuda()
        self.d_tp = torch.full((n, cap), 0xA5, dtype=torch.uint8, device="cuda")
        self.d_best = torch.full((n, cap), -9, dtype=torch.int32, device="cuda")
        self.d_result = torch.full((4,), -9.0, dtype=torch.float64, device="cuda")
        self.d_curve = torch.full((n * cap, 2), -9.0, dtype=torch.float64, device="cuda")
        self.work_bytes = images.average_precision_workspace(self.n, cap)
        self.d_work = torch.zeros(max(self.work_bytes, 16), dtype=torch.uint8, device="cuda")
        self.saved = (self.d_dets.clone(), self.d_counts.clone(), self.d_gt.clone(), self.d_gt_counts.clone())

    def match(self, thr, stream=None, best=True):
        self.images.match_device(self.d_dets.data_ptr(), self.d_counts.data_ptr(), self.n, self.cap, self.d_gt.data_ptr(),
                                 self.d_gt_counts.data_ptr(), self.gt_cap, thr, self.d_tp.data_ptr(), self.d_best.data_ptr() if best else None,
                                 stream=stream)

    def average_precision(self, stream=None, work_bytes=None, curve=True):
        self.images.average_precision_device(self.d_dets.data_ptr(), self.d_counts.data_ptr(), self.d_tp.data_ptr(), self.n, self.cap,
                                             self.d_gt_counts.data_ptr(), self.gt_cap, self.d_work.data_ptr(),
                                             self.work_bytes if work_bytes is None else work_bytes, self.d_result.data_ptr(),
                                             self.d_curve.data_ptr() if curve else None, stream=stream)

    def got(self):
        self.torch.cuda.synchronize()
        res = self.d_result.cpu().numpy().view(es.RESULT)[0]
        return dict(ap=float(res["ap"]), detections=int(res["detections"]), ground_truths=int(res["ground_truths"]),
                    true_positives=int(res["true_positives"]), tp=self.d_tp.cpu().numpy()[:self.n], best=self.d_best.cpu().numpy()[:self.n],
                    curve=self.d_curve.cpu().numpy())

    def inputs_untouched(self):
        now = (self.d_dets, self.d_counts, self.d_gt, self.d_gt_counts)                  # as bytes: a NaN in a label equals itself
        return all(self.torch.equal(a.view(self.torch.uint8), b.view(self.torch.uint8)) for a, b in zip(self.saved, now))


@pytest.fixture(scope="module")
def synthetic(yf, network, torch_cuda):
    """300 frames of seeded 7x7 heads decoded on the device: records of 0 .. 147 per frame, ties in the confidence (an int8 logit)"""
    torch = torch_cuda
    n = 300
    heads = synthetic_heads(np.random.default_rng(41), n)
    d_heads = torch.from_numpy(heads).cuda()
    d_dets = torch.zeros((n, CAP, 28), dtype=torch.uint8, device="cuda")
    d_counts = torch.zeros((n,), dtype=torch.int32, device="cuda")
    network.decode_device(d_heads.data_ptr(), n, d_dets.data_ptr(), d_counts.data_ptr(), CAP, w_scale=7.3, h_scale=8.1)
    dets, counts = to_host(yf, d_dets, d_counts, CAP)
    assert counts.max() == CAP and counts.min() >= 0 and 5000 < counts.sum() <= 20000
    return dets.copy(), counts.copy()


def _gt_counts(rng, n, gt_cap):
    """0 .. gt_cap with both ends; mostly few, so that the loop statement stays quick"""
    few = rng.integers(0, min(gt_cap, 6) + 1, n)
    counts = np.where(rng.random(n) < 0.12, rng.integers(0, gt_cap + 1, n), few).astype(np.int32)
    counts[0], counts[1], counts[2] = 0, gt_cap, gt_cap
    return counts


@pytest.mark.parametrize("gt_cap", [1, 7, 64, 256])
def test_match_and_average_precision_on_synthetic_heads(torch_cuda, images, synthetic, gt_cap):
    dets, counts = synthetic
    rng = np.random.default_rng(500 + gt_cap)
    gt_counts = _gt_counts(rng, dets.shape[0], gt_cap)
    gt = es.truths_near(rng, dets, counts, CAP, gt_cap, gt_counts)
    run = Run(torch_cuda, images, dets, counts, CAP, gt, gt_counts, gt_cap)
    run.match(0.5)
    run.average_precision()
    want = es.check_against_restatement(run.got(), dets, counts, CAP, gt, gt_counts, gt_cap, 0.5)
    assert run.inputs_untouched()
    assert 0 < want["true_positives"] < want["stats"]["candidates"] and want["stats"]["taken"] > 0       # doubly claimed ground truths
    if gt_cap > 1:
        assert want["stats"]["ties"] > 0                                                                  # equal best IoUs
    assert want["ap"] > 0.0


def _hand_records(yf, rng, n, cap):
    recs = np.zeros((n, cap), yf.DET_DTYPE)
    recs["frame"] = 77                                                     # not read: a record's frame is its place
    recs["conf"] = rng.choice(np.float32([0.71, 0.8, 0.9, 1.0, 1.0, -0.0, 0.0, np.nan, -2.5, np.inf]), (n, cap))
    cx, cy = rng.integers(0, 300, (n, cap)), rng.integers(0, 300, (n, cap))
    recs["x1"], recs["y1"], recs["x2"], recs["y2"] = cx, cy, cx + rng.integers(-2, 60, (n, cap)), cy + rng.integers(-2, 60, (n, cap))
    return recs


@pytest.mark.parametrize("thr", [0.5, 0.0, 1.0, -1.0])
def test_match_hand_built_counts_around_a_pass(yf, torch_cuda, images, thr):
    """0, 1, 63, 64, 65 and 147 records (one pass of 64, two, three), counts below zero and above cap, ground-truth counts likewise"""
    rng = np.random.default_rng(17)
    counts = np.array([0, 1, 63, 64, 65, 147, -3, 1000, 128, 129], np.int32)
    n, gt_cap = counts.shape[0], 7
    recs = _hand_records(yf, rng, n, CAP)
    gt_counts = np.array([3, 7, 7, 0, 7, 7, 5, 7, -2, 400], np.int32)
    gt = es.truths_near(rng, recs, counts, CAP, gt_cap, gt_counts)
    gt.view(np.float64).reshape(n, gt_cap, 4)[4, 2] = (np.nan, 0.0, np.inf, 50.0)
    run = Run(torch_cuda, images, recs, counts, CAP, gt, gt_counts, gt_cap)
    run.match(thr)
    run.average_precision()
    want = es.check_against_restatement(run.got(), recs, counts, CAP, gt, gt_counts, gt_cap, thr)
    assert want["detections"] == 0 + 1 + 63 + 64 + 65 + 147 + 0 + 147 + 128 + 129 and run.inputs_untouched()
    # d_best and d_curve are optional: without them the flags and the result are the same
    again = Run(torch_cuda, images, recs, counts, CAP, gt, gt_counts, gt_cap)
    again.match(thr, best=False)
    again.average_precision(curve=False)
    got = again.got()
    assert (got["best"] == -9).all() and (got["curve"] == -9.0).all()
    assert np.array_equal(got["tp"], run.got()["tp"]) and es.same_bits(got["ap"], want["ap"])


def test_match_at_cap_1200(yf, torch_cuda, images):
    """8 frames of up to 1200 records from the decode of 20x20 heads (frame 0: all 1200, one shared confidence)"""
    torch = torch_cuda
    n, cap, gt_cap = 8, images.CAND160, 16
    rng = np.random.default_rng(61)
    d_heads = torch.from_numpy(synthetic_heads160(rng, n)).cuda()
    d_dets = torch.zeros((n, cap, 28), dtype=torch.uint8, device="cuda")
    d_counts = torch.zeros((n,), dtype=torch.int32, device="cuda")
    images.decode160_device(d_heads.data_ptr(), n, d_dets.data_ptr(), d_counts.data_ptr(), cap, w_scale=2.56, h_scale=2.26)
    dets, counts = to_host(yf, d_dets, d_counts, cap)
    assert counts[0] == cap and 2000 < counts.sum() <= 9600
    gt_counts = np.array([16, 16, 0, 5, 16, 1, 9, 16], np.int32)
    gt = es.truths_near(rng, dets, counts, cap, gt_cap, gt_counts)
    run = Run(torch, images, dets, counts, cap, gt, gt_counts, gt_cap)
    run.match(0.5)
    run.average_precision()
    want = es.check_against_restatement(run.got(), dets, counts, cap, gt, gt_counts, gt_cap, 0.5)
    assert want["true_positives"] > 0 and want["stats"]["taken"] > 0 and run.inputs_untouched()


def _confidences(rng, kind, shape):
    if kind == "equal":
        return np.full(shape, 0.75, np.float32)
    if kind == "two":
        return rng.choice(np.float32([0.9, 0.8]), shape)
    if kind == "int8":                                                     # what a decode gives: at most 256 values, heavy ties across frames
        table = (1.0 / (1.0 + np.exp(-np.arange(-128, 128) * 0.1))).astype(np.float32)
        return table[rng.integers(0, 256, shape)]
    bits = rng.integers(0, 2 ** 32, shape, dtype=np.uint64).astype(np.uint32)        # any float32, NaN, -0.0 and infinities included
    return bits.view(np.float32)


def _ap_case(yf, torch, images, m, kind, seed, n=16, num_gt=None):
    rng = np.random.default_rng(seed)
    counts = es.spread(rng, m, n, CAP)
    recs = np.zeros((n, CAP), yf.DET_DTYPE)
    recs["conf"] = _confidences(rng, kind, (n, CAP))
    flags = (rng.random((n, CAP)) < 0.3).astype(np.uint8) * rng.choice(np.uint8([1, 1, 255]), (n, CAP))      # any non-zero byte is a hit
    gt_counts = np.zeros(n, np.int32) if num_gt == 0 else rng.integers(0, 9, n).astype(np.int32)
    run = Run(torch, images, recs, counts, CAP, np.zeros((n, 8), es.GT), gt_counts, 8)
    run.d_tp.copy_(torch.from_numpy(flags))
    run.average_precision()
    got = run.got()
    confs = [[float(c) for c in recs["conf"][f, :counts[f]]] for f in range(n)]
    ap, curve, hits = es.ap_restated(confs, [flags[f, :counts[f]].tolist() for f in range(n)], int(gt_counts.sum()))
    want = dict(ap=ap, curve=curve, true_positives=hits, detections=m, ground_truths=int(gt_counts.sum()))
    es.check_result(got, want)
    assert run.inputs_untouched() and np.array_equal(got["tp"], flags)
    return want


def test_average_precision_of_0_1_and_2_records(yf, torch_cuda, images):
    for m in (0, 1, 2):
        for seed in range(4):
            want = _ap_case(yf, torch_cuda, images, m, "two", 10 * m + seed)
            if m <= 1:
                assert want["ap"] == 0.0                                   # the term of i = 0 is missing


@pytest.mark.parametrize("kind", ["equal", "two", "random", "int8"])
def test_average_precision_around_the_sort_tile(yf, torch_cuda, images, kind):
    """one record below, at and one above the tile of the sort (the binding's constant), and several tiles with a ragged end"""
    tile = images.EVAL_SORT_TILE
    n = -(-(3 * tile + 70) // CAP) + 3
    for k, m in enumerate((tile - 1, tile, tile + 1, 3 * tile + 69)):
        want = _ap_case(yf, torch_cuda, images, m, kind, 900 + k, n=n)
        assert 0 < want["true_positives"] < m and want["ap"] > 0.0


def test_average_precision_without_ground_truth(yf, torch_cuda, images):
    want = _ap_case(yf, torch_cuda, images, 700, "int8", 5, num_gt=0)
    assert want["ground_truths"] == 0 and want["true_positives"] > 0      # recall divides by max(1, 0)


def test_workspace_too_small_is_refused(yf, torch_cuda, images, synthetic):
    dets, counts = synthetic
    n = 16
    run = Run(torch_cuda, images, dets[:n], counts[:n], CAP, np.zeros((n, 1), es.GT), np.ones(n, np.int32), 1)
    with pytest.raises(images.ImagesError, match="work_bytes"):
        run.average_precision(work_bytes=run.work_bytes - 1)
    got = run.got()
    assert (run.d_result == -9.0).all().item() and (got["curve"] == -9.0).all() and not run.d_work.any().item()


def test_graph_capture(yf, torch_cuda, images, synthetic):
    torch = torch_cuda
    dets, counts = synthetic
    n, gt_cap = 128, 7
    rng = np.random.default_rng(71)
    gt_counts = _gt_counts(rng, n, gt_cap)
    gt = es.truths_near(rng, dets[:n], counts[:n], CAP, gt_cap, gt_counts)
    run = Run(torch, images, dets[:n], counts[:n], CAP, gt, gt_counts, gt_cap)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            run.match(0.5, stream=s.cuda_stream)
            run.average_precision(stream=s.cuda_stream)
    torch.cuda.synchronize()
    assert (run.d_tp == 0xA5).all().item() and (run.d_result == -9.0).all().item()         # captured, not run
    g.replay()
    es.check_against_restatement(run.got(), dets[:n], counts[:n], CAP, gt, gt_counts, gt_cap, 0.5)


def _check_evaluate(images, network, imgs, records, **kw):
    """records: per image the tuples (frame, anchor, row, col, q_conf, conf, x1, y1, x2, y2) the path decodes, before suppression.  The
    model scores itself: the ground truth is its own suppressed boxes; then the same shifted by a few pixels."""
    kept = [suppress(rr, 0.4) for rr in records]
    truths = [np.array([[r[6], r[7], r[8], r[9]] for r in rr], np.float64).reshape(-1, 4) for rr in kept]
    shifted = [t + 6.0 for t in truths]
    assert sum(len(t) for t in truths) > 0

    def preds(recs):
        return [[[int(r[6]), int(r[7]), int(r[8]), int(r[9]), float(np.float32(r[5]))] for r in rr] for rr in recs]

    results = {}
    for name, gts, nms, conf_iou in (("self", truths, 0.4, 0.5), ("unsuppressed", truths, None, 0.5), ("self 0.9", truths, 0.4, 0.9),
                                     ("shifted 0.9", shifted, 0.4, 0.9)):
        got = images.evaluate(network, imgs, gts, "bgr", conf_iou=conf_iou, iou_threshold=nms, **kw)
        want = es.score_restated(preds(kept if nms is not None else records), [t.tolist() for t in gts], conf_iou)
        es.check_result(dict(got, curve=None), want)
        assert got["precision"] == want["true_positives"] / (want["detections"] + 1e-16)
        assert got["recall"] == want["true_positives"] / max(1, want["ground_truths"])
        results[name] = got
    # every kept box finds itself; a shift of a few pixels loses true positives at a strict threshold
    assert results["self"]["true_positives"] == results["self"]["ground_truths"] == results["self"]["detections"]
    assert results["shifted 0.9"]["true_positives"] < results["self 0.9"]["true_positives"]
    assert results["unsuppressed"]["detections"] >= results["self"]["detections"]


def test_evaluate_on_the_reference_images(yf, network, oracle, torch_cuda, images, ptq):
    imgs = real_images(ptq)
    frames = np.stack([expect_frame(ptq, im, 0, 56) for im in imgs])
    heads = oracle.run(frames)
    records = [oracle.decode_py(heads[i], i, w_scale=im.shape[1] / 56., h_scale=im.shape[0] / 56.) for i, im in enumerate(imgs)]
    _check_evaluate(images, network, imgs, records)
    assert images.evaluate(network, [], [])["detections"] == 0


def test_evaluate_at_160(yf, network, torch_cuda, images, ptq):
    """the records of the 160x160 path as its own entry point decodes them (checked against the host build in test_boxes160_gpu)"""
    imgs = real_images(ptq)
    b = Batch(torch_cuda, images, imgs, "bgr", out=160)
    b.run_decode(images, network)
    records, _ = b.records(yf)
    _check_evaluate(images, network, imgs, records, size=160)


def test_evaluate_on_the_fp16_network(yf, network, torch_cuda, images, ptq):
    """... and of the fp16 network (checked against the host build in test_images_float_gpu)"""
    network.fp16_init()
    imgs = real_images(ptq)
    b = F16Batch(torch_cuda, images, imgs, "bgr")
    b.run_decode(images, network)
    dets, counts = to_host(yf, b.d_dets, b.d_counts, b.cap)
    records = [tuples(dets[i, :min(int(counts[i]), b.cap)]) for i in range(b.n)]
    _check_evaluate(images, network, imgs, records, dtype="fp16")
