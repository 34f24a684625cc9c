"""Tiled detection on the MI355X: the merge of the tiles' records (yf_images_gather_tiles_device) on seeded records against the host build
and the plain-Python statement of tests/tiles_support.py, byte for byte with the untouched slots still holding their sentinel; and end to
end -- a mosaic whose tiles are photographs against `detect` of the photographs, overlapping tiles and the whole-image tile against the
chain existing ragged run -> tiles_support's merge -> images_support.nms_restated, `evaluate(tile=...)` against tests/eval_support.py's
statement on those merged records, and the overflow of out_cap.  Every comparison is exact.  A `first` that is not well formed is not
run here: tests/test_tiles_sanitize.py does that on the host build."""
import os

import numpy as np
import pytest

import eval_support as es
import tiles_support as ts
from conftest import ROOT
from images_support import Batch, expect_frame, expect_kept, real_images, sentinels, to_host
from images_support import images_after_network, ptq, torch_cuda          # noqa: F401 (fixtures; `images` is images_after_network)

pytestmark = pytest.mark.gpu


# ---- the gather alone ----
def _up(torch, dets, counts, tiles, first):
    t, cap = dets.shape
    return (torch.from_numpy(dets.view(np.uint8).reshape(t, cap, 28).copy()).cuda(), torch.from_numpy(counts.copy()).cuda(),
            torch.from_numpy(tiles.view(np.uint8).copy()).cuda(), torch.from_numpy(first.copy()).cuda())


def _gather(torch, images, d, t, cap, n, out_cap, stream=None):
    """-> (bytes uint8[n, out_cap, 28], totals int32[n]) as the device left them in sentinel-filled buffers"""
    d_dets, d_counts, d_tiles, d_first = d
    d_out, d_oc = sentinels(torch, n, out_cap)
    wb = images.gather_tiles_workspace(t)
    d_work = torch.empty(max(wb, 16), dtype=torch.uint8, device="cuda")
    images.gather_tiles_device(d_dets.data_ptr(), d_counts.data_ptr(), t, cap, d_tiles.data_ptr(), d_first.data_ptr(), n, d_out.data_ptr(),
                               d_oc.data_ptr(), out_cap, d_work.data_ptr(), wb, stream=stream)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()[:n], d_oc.cpu().numpy()[:n]


@pytest.mark.parametrize("cap", [1, 147, 1200])
def test_gather_equals_the_host_build_and_the_restatement(network, torch_cuda, images, cap):
    torch = torch_cuda
    host = ts.tiles_host()
    dets, counts, tiles, first = ts.seeded_tiles(np.random.default_rng(800 + cap), cap)
    assert {0, -1, ts.I32_MIN, cap, cap + 1} <= set(counts.tolist()) and ts.TILES_PER_IMAGE[:9] == [0, 1, 63, 64, 65, 255, 256, 257, 1000]
    t, n = dets.shape[0], len(first) - 1
    assert images.gather_tiles_workspace(t) == (4 * t + 15) // 16 * 16
    d = _up(torch, dets, counts, tiles, first)
    merged = ts.merge_restated(dets, counts, cap, tiles, first)               # once; every out_cap cuts it
    for out_cap in ts.cuts(cap):
        want = np.full((n, out_cap, 28), 0xA5, np.uint8)
        for i, m in enumerate(merged):
            k = min(m.shape[0], out_cap)
            want[i, :k] = m[:k].view(np.uint8).reshape(k, 28)
        totals = np.array([m.shape[0] for m in merged], np.int32)
        got, got_totals = _gather(torch, images, d, t, cap, n, out_cap)
        assert np.array_equal(got_totals, totals), out_cap                    # the true totals, which may exceed out_cap
        assert np.array_equal(got, want), out_cap                             # bytes, and the sentinel in every slot beyond min(total, out_cap)
        h_got, h_totals = ts.host_gather(host, dets, counts, cap, tiles, first, out_cap)
        assert np.array_equal(h_got, got) and np.array_equal(h_totals, got_totals), out_cap


def test_gather_edges_at_the_last_column(network, torch_cuda, images):
    """INT32_MIN moves by the origin, INT32_MAX and INT32_MAX - 5 saturate at x0 = 16383; y0 = 0 leaves y alone"""
    torch = torch_cuda
    dets = np.zeros((1, 4), ts.DET)
    dets["x1"][0] = [ts.I32_MIN, ts.I32_MAX, ts.I32_MAX - 5, 7]
    dets["x2"][0] = [ts.I32_MAX - 16383, ts.I32_MAX - 16384, -16383, ts.I32_MIN + 1]
    dets["y1"][0] = [ts.I32_MIN, ts.I32_MAX, ts.I32_MAX - 5, 7]
    dets["frame"], dets["conf"] = 99, 0.75
    tiles = np.array([(0, 16383, 0, 1, 1)], ts.TILE)
    first, counts = np.array([0, 0, 1], np.int32), np.array([4], np.int32)
    got, totals = _gather(torch, images, _up(torch, dets, counts, tiles, first), 1, 4, 2, 4)
    rec = got.view(ts.DET).reshape(2, 4)
    assert totals.tolist() == [0, 4] and (got[0] == 0xA5).all()
    assert rec["x1"][1].tolist() == [ts.I32_MIN + 16383, ts.I32_MAX, ts.I32_MAX, 16390]
    assert rec["x2"][1].tolist() == [ts.I32_MAX, ts.I32_MAX - 1, 0, ts.I32_MIN + 16384]
    assert rec["y1"][1].tolist() == dets["y1"][0].tolist() and (rec["frame"][1] == 1).all() and (rec["conf"][1] == np.float32(0.75)).all()


def test_gather_launches_nothing_and_refuses(network, torch_cuda, images):
    torch = torch_cuda
    lib = images.load()
    dets, counts, tiles, first = ts.seeded_tiles(np.random.default_rng(810), 5, per_image=[3, 0, 70])
    t, n, cap, out_cap = dets.shape[0], 3, 5, 40
    d_dets, d_counts, d_tiles, d_first = d = _up(torch, dets, counts, tiles, first)
    # n = 0, and t = 0 under n = 3: nothing is launched, nothing is written
    d_out, d_oc = sentinels(torch, n, out_cap)
    wb = images.gather_tiles_workspace(t)
    d_work = torch.full((wb + 32,), 0x5A, dtype=torch.uint8, device="cuda")
    call = lambda t_, n_, work, bytes_: lib.yf_images_gather_tiles_device(d_dets.data_ptr(), d_counts.data_ptr(), t_, cap, d_tiles.data_ptr(),
                                                                          d_first.data_ptr(), n_, d_out.data_ptr(), d_oc.data_ptr(), out_cap,
                                                                          work, bytes_, None)
    untouched = lambda: (torch.cuda.synchronize(), (d_out == 0xA5).all().item() and (d_oc == -7).all().item() and (d_work == 0x5A).all().item())[1]
    assert call(t, 0, d_work.data_ptr(), wb) == 0 and untouched()
    assert call(0, n, d_work.data_ptr(), 0) == n and untouched()
    assert images.gather_tiles_workspace(0) == 0
    # one byte short, and a workspace that is not 16-byte aligned: refused before anything is launched
    assert call(t, n, d_work.data_ptr(), wb - 1) == 0 and "work_bytes" in (lib.yf_images_last_error_text() or b"").decode() and untouched()
    assert call(t, n, d_work.data_ptr() + 4, wb) == 0 and "aligned" in (lib.yf_images_last_error_text() or b"").decode() and untouched()
    for bad_cap, bad_out in ((0, out_cap), (1201, out_cap), (cap, 0), (cap, 1201)):
        assert lib.yf_images_gather_tiles_device(d_dets.data_ptr(), d_counts.data_ptr(), t, bad_cap, d_tiles.data_ptr(), d_first.data_ptr(), n,
                                                 d_out.data_ptr(), d_oc.data_ptr(), bad_out, d_work.data_ptr(), wb, None) == 0
    assert untouched()
    # ... and the same arguments accepted
    got, totals = _gather(torch, images, d, t, cap, n, out_cap)
    want, want_totals = ts.expect_gather(dets, counts, cap, tiles, first, out_cap)
    assert np.array_equal(got, want) and np.array_equal(totals, want_totals)


def test_gather_is_capturable(network, torch_cuda, images):
    torch = torch_cuda
    dets, counts, tiles, first = ts.seeded_tiles(np.random.default_rng(811), 9, per_image=[5, 300, 0, 2])
    t, n, cap, out_cap = dets.shape[0], 4, 9, 64
    d_dets, d_counts, d_tiles, d_first = _up(torch, dets, counts, tiles, first)
    d_out, d_oc = sentinels(torch, n, out_cap)
    wb = images.gather_tiles_workspace(t)
    d_work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            images.gather_tiles_device(d_dets.data_ptr(), d_counts.data_ptr(), t, cap, d_tiles.data_ptr(), d_first.data_ptr(), n,
                                       d_out.data_ptr(), d_oc.data_ptr(), out_cap, d_work.data_ptr(), wb, stream=s.cuda_stream)
    torch.cuda.synchronize()
    assert (d_oc == -7).all().item()                                          # captured, not run
    g.replay()
    torch.cuda.synchronize()
    want, totals = ts.expect_gather(dets, counts, cap, tiles, first, out_cap)
    assert np.array_equal(d_out.cpu().numpy(), want) and np.array_equal(d_oc.cpu().numpy(), totals)


# ---- end to end ----
MOSAIC = list(range(9))                # the first nine golden real frames; each yields a record (asserted on the oracle below)
PW, PH = 410, 362


def _photographs(ptq):
    real = np.fromfile(os.path.join(ROOT, "tests", "golden", "real_frames_56.bin"), np.int8).reshape(-1, 56, 56, 3)
    rgb56 = (real.astype(np.int16) + 128).astype(np.uint8)
    return [np.ascontiguousarray(ptq.resize_linear_u8(rgb56[i], PW, PH)[..., ::-1]) for i in MOSAIC]


def test_mosaic_of_photographs_equals_detect_of_the_photographs(network, oracle, torch_cuda, images, ptq):
    photos = _photographs(ptq)
    # without the code under test: the oracle's decode of the nine prepared frames finds records in at least three photographs
    heads = oracle.run(np.stack([expect_frame(ptq, im, 0, 56) for im in photos]))
    ws, hs = float(np.float32(PW / 56.)), float(np.float32(PH / 56.))
    found = [len(oracle.decode_py(heads[i], i, w_scale=ws, h_scale=hs)) for i in range(9)]
    assert sum(k > 0 for k in found) >= 3, found
    canvas = np.zeros((3 * PH, 3 * PW, 3), np.uint8)
    for k, im in enumerate(photos):
        canvas[(k // 3) * PH:(k // 3 + 1) * PH, (k % 3) * PW:(k % 3 + 1) * PW] = im
    assert canvas.shape == (1086, 1230, 3)
    tiles, _, first = images.plan_tiles([canvas.shape[:2]], "bgr", (PH, PW), None, False)
    assert first.tolist() == [0, 9] and [(int(q["x0"]), int(q["y0"])) for q in tiles] == [((k % 3) * PW, (k // 3) * PH) for k in range(9)]
    boxes = images.detect(network, photos, "bgr")
    assert [len(b) for b in boxes] == found
    want = np.concatenate([b + np.array([(k % 3) * PW, (k // 3) * PH] * 2, np.int32) for k, b in enumerate(boxes)])
    got = images.detect_tiled(network, [canvas], (PH, PW), stride=None, whole=False, iou_threshold=None)
    assert len(got) == 1 and got[0].dtype == np.int32 and got[0].tolist() == want.tolist()
    # above out_cap: the image and its total are named
    with pytest.raises(images.ImagesError, match=f"image 0 has {sum(found)} merged records"):
        images.detect_tiled(network, [canvas], (PH, PW), whole=False, out_cap=sum(found) - 1)
    assert images.detect_tiled(network, [], 56) == []
    with pytest.raises(images.ImagesError, match="stride"):
        images.plan_tiles([(10, 10)], "bgr", 8, 9)


def _canvases(ptq):
    """three ragged canvases of pasted photographs: 2 x 2 on black, a row of three sizes on grey, one photograph alone"""
    imgs = real_images(ptq)
    a = np.zeros((724, 820, 3), np.uint8)
    for k, (y, x) in ((0, (0, 0)), (2, (0, 410)), (7, (362, 0)), (10, (362, 410))):
        a[y:y + imgs[k].shape[0], x:x + imgs[k].shape[1]] = imgs[k]
    b = np.full((470, 1040, 3), 128, np.uint8)
    x = 7
    for k in (1, 3, 4):
        h, w = imgs[k].shape[:2]
        b[11:11 + h, x:x + w] = imgs[k]
        x += w + 5
    return [a, b, imgs[12]]


def _tile_records(yf, torch, images, network, buf, tile_desc, size, dtype):
    """the per-tile records of the existing ragged run on the tile descriptors -> (DET [t, cap], counts)"""
    if dtype == "int8":
        b = Batch(torch, images, None, "bgr", size, desc=tile_desc, buf=buf)
        images.set_decode_tables(*network.decode_tables())
        b.run_decode(images, network)
        return to_host(yf, b.d_dets, b.d_counts, b.cap)
    t, cap = tile_desc.shape[0], 147
    d_px, d_desc = torch.from_numpy(buf).cuda(), torch.from_numpy(tile_desc.view(np.uint8).copy()).cuda()
    d_frames = torch.empty((t, 56, 56, 3), dtype=torch.float16, device="cuda")
    d_logits = torch.empty((t, 7, 7, 18), dtype=torch.float32, device="cuda")
    d_dets, d_counts = sentinels(torch, t, cap)
    d_status = torch.empty(t, dtype=torch.int32, device="cuda")
    images.run_decode_f16_ragged_device(network, d_px.data_ptr(), buf.nbytes, "bgr", d_desc.data_ptr(), t, d_frames.data_ptr(),
                                        d_logits.data_ptr(), d_dets.data_ptr(), d_counts.data_ptr(), cap, d_status.data_ptr())
    return to_host(yf, d_dets, d_counts, cap)


@pytest.mark.parametrize("size,dtype", [(56, "int8"), (160, "int8"), (56, "fp16")])
def test_overlap_and_whole_equal_the_chain(yf, network, torch_cuda, images, ptq, size, dtype):
    torch = torch_cuda
    if dtype == "fp16":
        network.fp16_init()
    canvases = _canvases(ptq)
    tile, stride = ((380, 420), (250, 300)) if size == 56 else ((400, 450), (300, 330))
    buf, tile_desc, tiles, first = images.pack_tiles(canvases, "bgr", tile, stride, True)
    assert first[-1] == tiles.shape[0] > 3 + len(canvases) and (np.diff(first) > 1).all()
    assert all(tiles[first[i]]["height"] == c.shape[0] and tiles[first[i]]["width"] == c.shape[1] for i, c in enumerate(canvases))   # whole first
    dets, counts = _tile_records(yf, torch, images, network, buf, tile_desc, size, dtype)
    cap = dets.shape[1]
    merged = ts.merge_restated(dets, counts, cap, tiles, first)
    assert sum((counts[first[i]:first[i + 1]] > 0).sum() >= 2 for i in range(3)) >= 2, "no canvas has records in two tiles"
    assert max(m.shape[0] for m in merged) <= 1200
    plain = images.detect_tiled(network, canvases, tile, stride, True, iou_threshold=None, size=size, dtype=dtype)
    assert [b.tolist() for b in plain] == [np.stack([m["x1"], m["y1"], m["x2"], m["y2"]], axis=1).reshape(-1, 4).tolist() for m in merged]
    kept = [expect_kept(m, m.shape[0], max(m.shape[0], 1), 0.4) for m in merged]
    boxes = images.detect_tiled(network, canvases, tile, stride, True, iou_threshold=0.4, size=size, dtype=dtype)
    assert [b.tolist() for b in boxes] == [np.stack([m["x1"], m["y1"], m["x2"], m["y2"]], axis=1).reshape(-1, 4).tolist() for m in kept]
    assert sum(len(b) for b in boxes) < sum(len(b) for b in plain), "overlapping tiles lost nothing to the suppression"
    # evaluate on the merged records: ground truths near the kept boxes of every canvas
    truths = [[[float(r["x1"]) - 2, float(r["y1"]) + 1, float(r["x2"]) + 3, float(r["y2"])] for r in k[:3]] + [[5.0, 5.0, 30.0, 40.0]] for k in kept]
    for thr, recs in ((0.4, kept), (None, merged)):
        preds = [[[int(r["x1"]), int(r["y1"]), int(r["x2"]), int(r["y2"]), float(r["conf"])] for r in rr] for rr in recs]
        want = es.score_restated(preds, truths, 0.5)
        got = images.evaluate(network, canvases, truths, "bgr", conf_iou=0.5, iou_threshold=thr, size=size, dtype=dtype, tile=tile,
                              stride=stride, whole=True)
        es.check_result(dict(got, curve=None), want)
        assert want["true_positives"] > 0
