"""Boxes at 160x160 on the MI355X: the decode of 20x20 heads (yf_images_decode160_device) against the oracle's yfo_decode_py, the
suppression of up to 1200 records per frame (yf_images_nms_wide_device) against the restatement of yoloface_test.py:165-190
(tests/images_support.py) and against the 256-record kernel, the image path images -> 160x160 frames -> heads -> records on the reference's
27 images, graph capture, and images.detect(size=160).  Every comparison is exact."""
import numpy as np
import pytest

from images_support import Batch, check_nms, expect_frame, real_images, sentinels, suppress, synthetic_heads160, to_host, tuples
from images_support import images_after_network, ptq, torch_cuda          # noqa: F401 (fixtures; `images` is images_after_network)

pytestmark = pytest.mark.gpu

THRESHOLDS = (0.0, 0.4, 0.5, 1.0)
CAND = 1200


def _decode(torch, images, heads, cap, ws, hs):
    n = heads.shape[0]
    d_heads = torch.from_numpy(heads).cuda()
    d_dets, d_counts = sentinels(torch, n, cap)
    images.decode160_device(d_heads.data_ptr(), n, d_dets.data_ptr(), d_counts.data_ptr(), cap, w_scale=ws, h_scale=hs)
    return d_heads, d_dets, d_counts


@pytest.mark.parametrize("cap", [1200, 100])
def test_decode160_uniform_against_the_oracle(yf, network, oracle, torch_cuda, images, cap):
    torch = torch_cuda
    n = 1024
    heads = synthetic_heads160(np.random.default_rng(160), n)
    ws, hs = float(np.float32(410 / 160.)), float(np.float32(362 / 160.))
    _, d_dets, d_counts = _decode(torch, images, heads, cap, ws, hs)
    dets, counts = to_host(yf, d_dets, d_counts, cap)
    raw = dets.view(np.uint8).reshape(n, cap, 28)
    assert (counts[::64] == CAND).all()
    for i in range(n):
        full = oracle.decode_py(heads[i], i, w_scale=ws, h_scale=hs, max_dets=CAND)
        want = oracle.decode_py(heads[i], i, w_scale=ws, h_scale=hs, max_dets=cap)
        assert counts[i] == len(full), (i, counts[i], len(full))                 # the true count, which may exceed cap
        k = min(len(full), cap)
        assert tuples(dets[i, :k]) == want, i
        assert (raw[i, k:] == 0xA5).all(), i                                     # slots beyond min(count, cap) keep their sentinel
    idx = np.arange(n)
    dense, sparse = counts[(idx % 3 != 1) & (idx % 64 != 0)], counts[(idx % 3 == 1) & (idx % 64 != 0)]
    assert 500 < dense.min() and dense.max() < 760 and sparse.max() < 64 and (counts > cap).any() == (cap < CAND)


def _oracle_chain(oracle, ptq, imgs, variant=0):
    frames = np.stack([expect_frame(ptq, im, 0, 160) for im in imgs])
    heads = oracle.run(frames, variant=variant)
    recs = [oracle.decode_py(heads[i], i, w_scale=float(np.float32(im.shape[1] / 160.)), h_scale=float(np.float32(im.shape[0] / 160.)),
                              max_dets=CAND)
            for i, im in enumerate(imgs)]
    return frames, heads, recs


def _real_batch_check(yf, network, oracle, torch, images, ptq, variant):
    """the 27 real images and one deliberately invalid descriptor in one ragged batch; returns the batch and the oracle's records"""
    imgs = real_images(ptq)
    buf, desc = images.pack_images(imgs + [imgs[0]], "bgr")
    bad = len(imgs)
    desc["row_stride"][bad] = desc["width"][bad] * 3 - 1                    # stride below a row: status 1
    b = Batch(torch, images, None, "bgr", 160, desc=desc, buf=buf)
    b.run_decode(images, network)
    torch.cuda.synchronize()
    assert b.d_status.cpu().numpy().tolist() == [0] * bad + [1]
    frames, heads, recs = _oracle_chain(oracle, ptq, imgs, variant)
    got_frames = b.d_frames.cpu().numpy()
    assert np.array_equal(got_frames[:bad], frames)
    assert (got_frames[bad] == -128).all()
    assert np.array_equal(b.d_heads.cpu().numpy()[:bad], heads)
    dets, counts = to_host(yf, b.d_dets, b.d_counts, b.cap)
    assert counts[bad] == 0
    for i in range(bad):
        assert counts[i] == len(recs[i]) and tuples(dets[i, :counts[i]]) == recs[i], i
    return b, imgs, recs, dets, counts


def test_real_images_to_records_and_suppression(yf, network, oracle, torch_cuda, images, ptq):
    torch = torch_cuda
    b, imgs, recs, dets, counts = _real_batch_check(yf, network, oracle, torch, images, ptq, 0)
    assert sum(len(r) for r in recs) > 0, "no image has records"
    # the same records from the heads alone: with the status array, and without it on the valid images
    d_dets, d_counts = sentinels(torch, b.n, b.cap)
    images.decode160_ragged_device(b.d_heads.data_ptr(), b.d_desc.data_ptr(), b.n, d_dets.data_ptr(), d_counts.data_ptr(), b.cap,
                                   d_status=b.d_status.data_ptr())
    again, cnt = to_host(yf, d_dets, d_counts, b.cap)
    assert np.array_equal(cnt, counts) and all(again[i, :cnt[i]].tobytes() == dets[i, :cnt[i]].tobytes() for i in range(b.n))
    images.decode160_ragged_device(b.d_heads.data_ptr(), b.d_desc.data_ptr(), b.n - 1, d_dets.data_ptr(), d_counts.data_ptr(), b.cap)
    again, cnt = to_host(yf, d_dets, d_counts, b.cap)
    assert np.array_equal(cnt, counts)
    lost_at = {}
    for thr in THRESHOLDS:
        d_out, d_oc = sentinels(torch, b.n, b.cap)
        images.nms_wide_device(b.d_dets.data_ptr(), b.d_counts.data_ptr(), b.n, b.cap, thr, d_out.data_ptr(), d_oc.data_ptr())
        lost_at[thr] = check_nms(yf, dets, counts, d_out, d_oc, b.cap, thr)
        out, oc = to_host(yf, d_out, d_oc, b.cap)
        assert [tuples(out[i, :oc[i]]) for i in range(len(imgs))] == [suppress(r, thr) for r in recs], thr
    assert lost_at[0.4] > 0, "no image lost a record at 0.4: suppression did not happen"
    assert lost_at[0.0] >= lost_at[0.4] >= lost_at[1.0]


def test_rounding_is_honoured(yf, network, oracle, torch_cuda, images, ptq):
    network.set_requant_rounding(yf.YF_ROUND_TIES_UP)
    try:
        _real_batch_check(yf, network, oracle, torch_cuda, images, ptq, oracle_variant("U"))
    finally:
        network.set_requant_rounding(yf.YF_ROUND_TFLITE_REF)


def oracle_variant(name):
    from oracle.oracle import VARIANTS
    return VARIANTS[name]


def test_uniform_image_path_equals_ragged(yf, network, torch_cuda, images, ptq):
    torch = torch_cuda
    n, H, W = 64, 362, 410
    real = real_images(ptq)[0]
    g = torch.Generator(device="cuda").manual_seed(5)
    noise = torch.randint(-24, 25, (n, H, W, 3), device="cuda", generator=g, dtype=torch.int16)
    px = (torch.from_numpy(real).cuda().to(torch.int16)[None] + noise).clamp(0, 255).to(torch.uint8).contiguous()
    fs, rs, cap = H * W * 3, W * 3, CAND
    mk = lambda: (torch.empty((n, 160, 160, 3), dtype=torch.int8, device="cuda"), torch.empty((n, 20, 20, 18), dtype=torch.int8, device="cuda"),
                  *sentinels(torch, n, cap))
    f_u, h_u, d_u, c_u = mk()
    images.run_decode160_device(network, px.data_ptr(), px.numel(), "bgr", H, W, rs, fs, n, f_u.data_ptr(), h_u.data_ptr(), d_u.data_ptr(),
                                c_u.data_ptr(), cap)
    desc = np.zeros(n, images.IMAGE_DTYPE)
    desc["offset"], desc["height"], desc["width"], desc["row_stride"] = np.arange(n) * fs, H, W, rs
    d_desc = torch.from_numpy(desc.view(np.uint8)).cuda()
    f_r, h_r, d_r, c_r = mk()
    st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    images.run_decode160_ragged_device(network, px.data_ptr(), px.numel(), "bgr", d_desc.data_ptr(), n, f_r.data_ptr(), h_r.data_ptr(),
                                       d_r.data_ptr(), c_r.data_ptr(), cap, st.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(f_u, f_r) and torch.equal(h_u, h_r) and torch.equal(c_u, c_r) and torch.equal(d_u, d_r)
    assert (st == 0).all().item() and int(c_u.sum().item()) > 0
    assert np.array_equal(f_u[0].cpu().numpy(), expect_frame(ptq, px[0].cpu().numpy(), 0, 160))


def _records(yf, rng, n, cap, counts):
    """records that are not a decode's: tied and special confidences, overlapping boxes in a 410 x 362 picture"""
    recs = np.zeros((n, cap), yf.DET_DTYPE)
    recs["frame"] = np.arange(n)[:, None]
    recs["anchor"], recs["row"], recs["col"] = rng.integers(0, 3, (n, cap)), rng.integers(0, 20, (n, cap)), rng.integers(0, 20, (n, cap))
    pool = np.concatenate([np.float32([0.8, 0.9, 1.0, 1.0, -0.0, 0.0, np.nan, -2.5, np.inf]), np.linspace(0.7, 1.0, 23, dtype=np.float32)])
    recs["conf"] = rng.choice(pool, (n, cap))
    cx, cy = rng.integers(0, 410, (n, cap)), rng.integers(0, 362, (n, cap))
    recs["x1"], recs["y1"] = cx, cy
    recs["x2"], recs["y2"] = cx + rng.integers(-2, 90, (n, cap)), cy + rng.integers(-2, 90, (n, cap))
    return recs, np.asarray(counts, np.int32)


def _up(torch, recs, counts):
    n, cap = recs.shape
    return torch.from_numpy(recs.view(np.uint8).reshape(n, cap, 28).copy()).cuda(), torch.from_numpy(np.asarray(counts, np.int32).copy()).cuda()


def test_nms_wide_on_decoded_records(yf, network, oracle, torch_cuda, images):
    """the records of the decode test's heads: 256 frames (86 of them dense, four with all 1200 records tied), every threshold"""
    torch = torch_cuda
    n, cap = 256, CAND
    heads = synthetic_heads160(np.random.default_rng(161), n)
    _, d_dets, d_counts = _decode(torch, images, heads, cap, float(np.float32(410 / 160.)), float(np.float32(362 / 160.)))
    dets_in, counts_in = to_host(yf, d_dets, d_counts, cap)
    idx = np.arange(n)
    assert (counts_in[::64] == CAND).all() and (counts_in[(idx % 3 == 1) & (idx % 64 != 0)] <= 64).all() and (counts_in[2::3] > 256).all()
    saved = d_dets.clone()
    for thr in THRESHOLDS:
        d_out, d_oc = sentinels(torch, n, cap)
        images.nms_wide_device(d_dets.data_ptr(), d_counts.data_ptr(), n, cap, thr, d_out.data_ptr(), d_oc.data_ptr())
        frames = None if thr == 0.4 else range(0, n, 2)
        lost = check_nms(yf, dets_in, counts_in, d_out, d_oc, cap, thr, frames)
        assert lost > 0 or thr >= 1.0
    assert torch.equal(saved, d_dets)                       # out of place: the input is not touched
    # in place equals out of place
    d_out, d_oc = sentinels(torch, n, cap)
    images.nms_wide_device(d_dets.data_ptr(), d_counts.data_ptr(), n, cap, 0.4, d_out.data_ptr(), d_oc.data_ptr())
    images.nms_wide_device(d_dets.data_ptr(), d_counts.data_ptr(), n, cap, 0.4)
    a, ac = to_host(yf, d_dets, d_counts, cap)
    b, oc = to_host(yf, d_out, d_oc, cap)
    assert np.array_equal(ac, oc)
    for f in range(n):
        assert a[f, :oc[f]].tobytes() == b[f, :oc[f]].tobytes(), f
        assert a[f, oc[f]:counts_in[f]].tobytes() == dets_in[f, oc[f]:counts_in[f]].tobytes(), f        # beyond the kept count: not written


def test_nms_wide_exact_counts_odd_counts_and_small_caps(yf, network, torch_cuda, images):
    torch = torch_cuda
    rng = np.random.default_rng(162)
    sizes = [0, 1, 63, 64, 65, 255, 256, 257, 1199, 1200]
    # frames with exactly these many records, in an order that mixes one-wave and workgroup frames inside the groups of four
    counts = sizes + sizes[::-1] + [1200, 3, 64, 700, 65, 65, 0, 1200, 2, 9, 1, 300]
    recs, counts = _records(yf, rng, len(counts), CAND, counts)
    d_recs, d_cnt = _up(torch, recs, counts)
    for thr in THRESHOLDS:
        d_out, d_oc = sentinels(torch, recs.shape[0], CAND)
        images.nms_wide_device(d_recs.data_ptr(), d_cnt.data_ptr(), recs.shape[0], CAND, thr, d_out.data_ptr(), d_oc.data_ptr())
        check_nms(yf, recs, counts, d_out, d_oc, CAND, thr)
    # negative counts, counts above cap, and in place on them
    odd = counts.copy()
    odd[1::5] = -3
    odd[2::5] = 5000
    d_odd = torch.from_numpy(odd).cuda()
    d_out, d_oc = sentinels(torch, recs.shape[0], CAND)
    images.nms_wide_device(d_recs.data_ptr(), d_odd.data_ptr(), recs.shape[0], CAND, 0.4, d_out.data_ptr(), d_oc.data_ptr())
    check_nms(yf, recs, odd, d_out, d_oc, CAND, 0.4)
    d_copy = d_recs.clone()
    images.nms_wide_device(d_copy.data_ptr(), d_odd.data_ptr(), recs.shape[0], CAND, 0.4)
    a, ac = to_host(yf, d_copy, d_odd, CAND)
    b, oc = to_host(yf, d_out, d_oc, CAND)
    assert np.array_equal(ac, oc) and all(a[f, :oc[f]].tobytes() == b[f, :oc[f]].tobytes() for f in range(recs.shape[0]))
    # cap below the count: the decode writes 100 records of frames that have more, the suppression runs over those 100
    cap = 100
    heads = synthetic_heads160(np.random.default_rng(163), 128)
    _, d100, k100 = _decode(torch, images, heads, cap, 2.5, 2.25)
    in100, cnt100 = to_host(yf, d100, k100, cap)
    assert (cnt100 > cap).any()
    d_out, d_oc = sentinels(torch, 128, cap)
    images.nms_wide_device(d100.data_ptr(), k100.data_ptr(), 128, cap, 0.4, d_out.data_ptr(), d_oc.data_ptr())
    check_nms(yf, in100, cnt100, d_out, d_oc, cap, 0.4)
    # n = 0: nothing launched, nothing written; n not a multiple of four
    d_out, d_oc = sentinels(torch, 1, CAND)
    images.nms_wide_device(d_recs.data_ptr(), d_cnt.data_ptr(), 0, CAND, 0.4, d_out.data_ptr(), d_oc.data_ptr())
    torch.cuda.synchronize()
    assert (d_out == 0xA5).all().item() and (d_oc == -7).all().item()
    for n in (1, 2, 3, 5):
        d_out, d_oc = sentinels(torch, recs.shape[0], CAND)
        images.nms_wide_device(d_recs.data_ptr(), d_cnt.data_ptr(), n, CAND, 0.5, d_out.data_ptr(), d_oc.data_ptr())
        check_nms(yf, recs, counts, d_out, d_oc, CAND, 0.5, frames=range(n))
        assert (d_oc[n:] == -7).all().item() and (d_out[n:] == 0xA5).all().item()


@pytest.mark.parametrize("cap", [256, 147, 20, 1])
def test_nms_wide_equals_the_256_record_kernel(yf, network, torch_cuda, images, cap):
    torch = torch_cuda
    n = 2048
    rng = np.random.default_rng(164 + cap)
    counts = rng.integers(-2, cap + 40, n)
    counts[::7] = cap
    counts[1::7] = rng.integers(0, 10, counts[1::7].shape)
    recs, counts = _records(yf, rng, n, cap, counts)
    d_recs, d_cnt = _up(torch, recs, counts)
    for thr in THRESHOLDS:
        o1, c1 = sentinels(torch, n, cap)
        o2, c2 = sentinels(torch, n, cap)
        images.nms_device(d_recs.data_ptr(), d_cnt.data_ptr(), n, cap, thr, o1.data_ptr(), c1.data_ptr())
        images.nms_wide_device(d_recs.data_ptr(), d_cnt.data_ptr(), n, cap, thr, o2.data_ptr(), c2.data_ptr())
        torch.cuda.synchronize()
        assert torch.equal(c1, c2), thr
        assert torch.equal(o1, o2), thr                    # identical bytes, the untouched slots included
    assert cap == 1 or int((c1 < torch.clamp(d_cnt, 0, cap)).sum().item()) > 0          # a single record has nothing to lose


def test_graph_capture_of_decode_and_suppression(yf, network, torch_cuda, images):
    torch = torch_cuda
    n, cap = 96, CAND
    heads = synthetic_heads160(np.random.default_rng(165), n)
    ws, hs = 2.5, 2.25
    d_heads, d_dets, d_counts = _decode(torch, images, heads, cap, ws, hs)            # the direct calls (and the one-time table upload)
    d_out, d_oc = sentinels(torch, n, cap)
    images.nms_wide_device(d_dets.data_ptr(), d_counts.data_ptr(), n, cap, 0.4, d_out.data_ptr(), d_oc.data_ptr())
    torch.cuda.synchronize()
    g_dets, g_counts = sentinels(torch, n, cap)
    g_out, g_oc = sentinels(torch, n, cap)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            images.decode160_device(d_heads.data_ptr(), n, g_dets.data_ptr(), g_counts.data_ptr(), cap, w_scale=ws, h_scale=hs, stream=s.cuda_stream)
            images.nms_wide_device(g_dets.data_ptr(), g_counts.data_ptr(), n, cap, 0.4, g_out.data_ptr(), g_oc.data_ptr(), stream=s.cuda_stream)
    torch.cuda.synchronize()
    assert (g_counts == -7).all().item() and (g_oc == -7).all().item()         # captured, not run
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(g_counts, d_counts) and torch.equal(g_dets, d_dets)
    assert torch.equal(g_oc, d_oc) and torch.equal(g_out, d_out)
    assert int(d_oc.sum().item()) > 0


def test_detect_at_160_and_at_56(yf, network, oracle, torch_cuda, images, ptq):
    imgs = real_images(ptq)
    _, _, recs = _oracle_chain(oracle, ptq, imgs)
    plain = images.detect(network, imgs, "bgr", size=160)
    assert [bx.tolist() for bx in plain] == [[[r[6], r[7], r[8], r[9]] for r in rr] for rr in recs]
    boxes = images.detect(network, imgs, "bgr", size=160, iou_threshold=0.4)
    assert [bx.tolist() for bx in boxes] == [[[r[6], r[7], r[8], r[9]] for r in suppress(rr, 0.4)] for rr in recs]
    assert all(bx.dtype == np.int32 and bx.shape[1] == 4 for bx in boxes)
    assert 0 < sum(len(b) for b in boxes) < sum(len(b) for b in plain)
    for kw in (dict(), dict(iou_threshold=0.4), dict(cap=20)):
        a, b = images.detect(network, imgs, "bgr", **kw), images.detect(network, imgs, "bgr", size=56, **kw)
        assert [x.tolist() for x in a] == [x.tolist() for x in b], kw
