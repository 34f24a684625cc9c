"""IoU suppression of decoded records on the MI355X (yf_images_nms_device): every frame's output equals the restatement of
YoloFaceDetector.non_max_suppression (yoloface/tensorflow/yoloface_test.py:165-190, stable tie order; tests/images_support.py) applied to that
frame's input records, byte for byte and in keep order -- on the reference's 27 images against the oracle's records, on seeded synthetic
heads in all three decode modes and four thresholds, in place, with cap below the count, and through images.detect()."""
import numpy as np
import pytest

from images_support import Batch, check_nms, expect_frame, real_images, sentinels, suppress, synthetic_heads, to_host, tuples
from images_support import images_after_network, ptq, torch_cuda          # noqa: F401 (fixtures; `images` is images_after_network)

pytestmark = pytest.mark.gpu

THRESHOLDS = (0.0, 0.4, 0.5, 1.0)
I32_MIN = -2 ** 31


def _nms(images, d_dets, d_counts, n, cap, thr, d_out, d_oc):
    images.nms_device(d_dets.data_ptr(), d_counts.data_ptr(), n, cap, thr, d_out.data_ptr(), d_oc.data_ptr())


def test_real_images_against_the_oracle(yf, network, oracle, torch_cuda, images, ptq):
    torch = torch_cuda
    imgs = real_images(ptq)
    b = Batch(torch, images, imgs, "bgr")
    b.run_decode(images, network)
    torch.cuda.synchronize()
    frames = np.stack([expect_frame(ptq, im, 0, 56) for im in imgs])
    heads = oracle.run(frames)
    assert np.array_equal(b.d_heads.cpu().numpy(), heads)
    want_in = [oracle.decode_py(heads[i], i, w_scale=im.shape[1] / 56., h_scale=im.shape[0] / 56.) for i, im in enumerate(imgs)]
    dets_in, counts_in = to_host(yf, b.d_dets, b.d_counts, b.cap)
    assert [tuples(dets_in[i, :counts_in[i]]) for i in range(b.n)] == want_in
    lost_at = {}
    for thr in THRESHOLDS:
        d_out, d_oc = sentinels(torch, b.n, b.cap)
        _nms(images, b.d_dets, b.d_counts, b.n, b.cap, thr, d_out, d_oc)
        out, oc = to_host(yf, d_out, d_oc, b.cap)
        got = [tuples(out[i, :oc[i]]) for i in range(b.n)]
        assert got == [suppress(w, thr) for w in want_in], thr
        lost_at[thr] = sum(len(w) for w in want_in) - sum(len(g) for g in got)
        # slots beyond the kept count are not written
        raw = d_out.cpu().numpy()
        assert all((raw[i, oc[i]:] == 0xA5).all() for i in range(b.n))
    assert sum(len(w) for w in want_in) > 0
    assert lost_at[0.4] > 0, "no image lost a record at 0.4: suppression did not happen"
    assert lost_at[0.0] >= lost_at[0.4] >= lost_at[1.0]


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_synthetic_heads_every_mode_and_threshold(yf, network, torch_cuda, images, mode):
    torch = torch_cuda
    n, cap = 4096, 147
    rng = np.random.default_rng(100 + mode)
    heads = synthetic_heads(rng, n)
    d_heads = torch.from_numpy(heads).cuda()
    d_dets = torch.zeros((n, cap, 28), dtype=torch.uint8, device="cuda")
    d_counts = torch.zeros((n,), dtype=torch.int32, device="cuda")
    # the first half through the per-image-scale decode (sizes up to 16384: scales up to 292.6), the second half through the network's
    # decode at a scale that puts the PY edges beyond int32 (INT32_MIN) and the FW edges through their clamps
    desc = np.zeros(n // 2, images.IMAGE_DTYPE)
    desc["height"], desc["width"] = rng.integers(1, 16385, n // 2), rng.integers(1, 16385, n // 2)
    desc["row_stride"] = desc["width"] * 3
    d_desc = torch.from_numpy(desc.view(np.uint8).copy()).cuda()
    images.decode_ragged_device(d_heads.data_ptr(), d_desc.data_ptr(), n // 2, d_dets.data_ptr(), d_counts.data_ptr(), cap, mode=mode)
    half = n // 2
    network.decode_device(d_heads[half:].data_ptr(), n - half, d_dets[half:].data_ptr(), d_counts[half:].data_ptr(), cap, mode=mode,
                          w_scale=6.0e7, h_scale=5.0e7)
    dets_in, counts_in = to_host(yf, d_dets, d_counts, cap)
    assert (counts_in[::64] == 147).all() and counts_in.min() >= 0
    tied = dets_in[0, :147]
    assert (tied["q_conf"] == tied["q_conf"][0]).all()
    if mode == 0:
        edges = np.stack([dets_in[half:][e] for e in ("x1", "y1", "x2", "y2")])
        assert (edges == I32_MIN).any() and (edges != I32_MIN).any()
    saved = d_dets.clone()
    for thr in THRESHOLDS:
        d_out, d_oc = sentinels(torch, n, cap)
        _nms(images, d_dets, d_counts, n, cap, thr, d_out, d_oc)
        lost = check_nms(yf, dets_in, counts_in, d_out, d_oc, cap, thr)
        if thr < 1.0:
            assert lost > 0
    assert torch.equal(saved, d_dets)                       # out of place: the input is not touched


def test_in_place_cap_below_count_and_odd_counts(yf, network, torch_cuda, images):
    torch = torch_cuda
    n, cap = 4096, 147
    heads = synthetic_heads(np.random.default_rng(7), n)
    d_heads = torch.from_numpy(heads).cuda()
    d_dets = torch.zeros((n, cap, 28), dtype=torch.uint8, device="cuda")
    d_counts = torch.zeros((n,), dtype=torch.int32, device="cuda")
    network.decode_device(d_heads.data_ptr(), n, d_dets.data_ptr(), d_counts.data_ptr(), cap, w_scale=7.3, h_scale=8.1)
    dets_in, counts_in = to_host(yf, d_dets, d_counts, cap)
    # in place equals out of place
    d_out, d_oc = sentinels(torch, n, cap)
    _nms(images, d_dets, d_counts, n, cap, 0.4, d_out, d_oc)
    images.nms_device(d_dets.data_ptr(), d_counts.data_ptr(), n, cap, 0.4)
    torch.cuda.synchronize()
    assert torch.equal(d_counts, d_oc)
    a, _ = to_host(yf, d_dets, d_counts, cap)
    b, oc = to_host(yf, d_out, d_oc, cap)
    for f in range(n):
        assert a[f, :oc[f]].tobytes() == b[f, :oc[f]].tobytes(), f
    check_nms(yf, dets_in, counts_in, d_out, d_oc, cap, 0.4)
    # counts below zero and above cap: the first min(max(count, 0), cap) records
    odd = counts_in.copy()
    odd[1::5] = -3
    odd[2::5] = 1000
    odd[3::5] = np.minimum(odd[3::5], 1)
    d_odd = torch.from_numpy(odd).cuda()
    d_src = torch.from_numpy(dets_in.view(np.uint8).reshape(n, cap, 28).copy()).cuda()
    d_out, d_oc = sentinels(torch, n, cap)
    _nms(images, d_src, d_odd, n, cap, 0.4, d_out, d_oc)
    check_nms(yf, dets_in, odd, d_out, d_oc, cap, 0.4)
    # cap below the count: the decode writes 20 records of a frame that has more, the suppression runs over those 20
    c20 = 20
    d20 = torch.zeros((n, c20, 28), dtype=torch.uint8, device="cuda")
    k20 = torch.zeros((n,), dtype=torch.int32, device="cuda")
    network.decode_device(d_heads.data_ptr(), n, d20.data_ptr(), k20.data_ptr(), c20, w_scale=7.3, h_scale=8.1)
    in20, cnt20 = to_host(yf, d20, k20, c20)
    assert (cnt20 > c20).any()
    d_out, d_oc = sentinels(torch, n, c20)
    _nms(images, d20, k20, n, c20, 0.4, d_out, d_oc)
    check_nms(yf, in20, cnt20, d_out, d_oc, c20, 0.4)
    # the largest cap, and records that are not a decode's (any conf bits, ties and all, -0.0 and NaN included)
    big = images.NMS_MAX_CAP
    rng = np.random.default_rng(12)
    recs = np.zeros((64, big), yf.DET_DTYPE)
    recs["frame"] = np.arange(64)[:, None]
    recs["conf"] = rng.choice(np.float32([0.8, 0.9, 1.0, -0.0, 0.0, np.nan, -2.5, np.inf]), (64, big))
    cx, cy = rng.integers(0, 200, (64, big)), rng.integers(0, 200, (64, big))
    recs["x1"], recs["y1"], recs["x2"], recs["y2"] = cx, cy, cx + rng.integers(-2, 30, (64, big)), cy + rng.integers(-2, 30, (64, big))
    cnt = rng.integers(0, big + 1, 64).astype(np.int32)
    cnt[0] = big
    d_recs = torch.from_numpy(recs.view(np.uint8).reshape(64, big, 28).copy()).cuda()
    d_cnt = torch.from_numpy(cnt).cuda()
    d_out, d_oc = sentinels(torch, 64, big)
    _nms(images, d_recs, d_cnt, 64, big, 0.3, d_out, d_oc)
    check_nms(yf, recs, cnt, d_out, d_oc, big, 0.3)


def test_zero_frames_and_100000(yf, network, torch_cuda, images):
    torch = torch_cuda
    cap = 147
    # n = 0: nothing launched, nothing written
    d_dets, d_counts = sentinels(torch, 1, cap)
    d_out, d_oc = sentinels(torch, 1, cap)
    _nms(images, d_dets, d_counts, 0, cap, 0.4, d_out, d_oc)
    torch.cuda.synchronize()
    assert (d_out == 0xA5).all().item() and (d_oc == -7).all().item()
    # 100 000 frames: the heads of 4096 frames repeated; every frame's output is its own frame's suppression (frame field included)
    n, base = 100000, 4096
    heads = synthetic_heads(np.random.default_rng(21), base)
    d_heads = torch.from_numpy(np.concatenate([heads] * (n // base + 1))[:n]).cuda()
    d_dets = torch.zeros((n, cap, 28), dtype=torch.uint8, device="cuda")
    d_counts = torch.zeros((n,), dtype=torch.int32, device="cuda")
    network.decode_device(d_heads.data_ptr(), n, d_dets.data_ptr(), d_counts.data_ptr(), cap, w_scale=7.3, h_scale=8.1)
    dets_in, counts_in = to_host(yf, d_dets, d_counts, cap)
    d_out, d_oc = sentinels(torch, n, cap)
    _nms(images, d_dets, d_counts, n, cap, 0.4, d_out, d_oc)
    out, oc = to_host(yf, d_out, d_oc, cap)
    sample = list(range(0, n, 37)) + list(range(n - 64, n))
    check_nms(yf, dets_in, counts_in, d_out, d_oc, cap, 0.4, frames=sample)
    # the same heads give the same records up to the frame field
    first = out[:base].copy()
    for r in range(1, n // base):
        blk = out[r * base:(r + 1) * base].copy()
        assert np.array_equal(oc[r * base:(r + 1) * base], oc[:base])
        blk["frame"] -= r * base
        for f in np.nonzero(oc[:base])[0][:200]:
            assert blk[f, :oc[f]].tobytes() == first[f, :oc[f]].tobytes()


def test_graph_capture(yf, network, torch_cuda, images):
    torch = torch_cuda
    n, cap = 512, 147
    heads = synthetic_heads(np.random.default_rng(31), n)
    d_heads = torch.from_numpy(heads).cuda()
    d_dets = torch.zeros((n, cap, 28), dtype=torch.uint8, device="cuda")
    d_counts = torch.zeros((n,), dtype=torch.int32, device="cuda")
    network.decode_device(d_heads.data_ptr(), n, d_dets.data_ptr(), d_counts.data_ptr(), cap, w_scale=5.0, h_scale=6.0)
    dets_in, counts_in = to_host(yf, d_dets, d_counts, cap)
    d_out, d_oc = sentinels(torch, n, cap)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            images.nms_device(d_dets.data_ptr(), d_counts.data_ptr(), n, cap, 0.4, d_out.data_ptr(), d_oc.data_ptr(), stream=s.cuda_stream)
    torch.cuda.synchronize()
    assert (d_oc == -7).all().item()                         # captured, not run
    g.replay()
    torch.cuda.synchronize()
    check_nms(yf, dets_in, counts_in, d_out, d_oc, cap, 0.4)


def test_detect_with_and_without_suppression(yf, network, oracle, torch_cuda, images, ptq):
    imgs = real_images(ptq)
    frames = np.stack([expect_frame(ptq, im, 0, 56) for im in imgs])
    heads = oracle.run(frames)
    recs = [oracle.decode_py(heads[i], i, w_scale=im.shape[1] / 56., h_scale=im.shape[0] / 56.) for i, im in enumerate(imgs)]
    plain = images.detect(network, imgs, "bgr")
    assert [bx.tolist() for bx in plain] == [[[r[6], r[7], r[8], r[9]] for r in rr] for rr in recs]
    for thr in (0.4, 0.0):
        boxes = images.detect(network, imgs, "bgr", iou_threshold=thr)
        want = [[[r[6], r[7], r[8], r[9]] for r in suppress(rr, thr)] for rr in recs]
        assert [bx.tolist() for bx in boxes] == want, thr
        assert all(bx.dtype == np.int32 and bx.shape[1] == 4 for bx in boxes)
    assert sum(len(b) for b in images.detect(network, imgs, "bgr", iou_threshold=0.4)) < sum(len(b) for b in plain)
