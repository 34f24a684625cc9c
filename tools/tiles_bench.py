#!/usr/bin/env python3
"""Tiled detection on full-HD canvases: what each launch costs and what tiling buys (GPU TOOL; bench.py is not involved).
The batch is 64 canvases of 1920x1080 BGR, mosaics of the real images of tests/images_support.py (eight photographs per canvas on grey,
one per 480x540 cell at a seeded offset).  It runs at size=160 with tile 320x320, stride 240 and the whole-image tile: 41 tiles per canvas.

    launches  device events around every call of the sequence images.detect_tiled runs -- prepare (yf_images_prepare_ragged_device), the
              network (yf_network_run_device_hw: its band kernels in one call), decode (yf_images_decode160_ragged_device), gather
              (yf_images_gather_tiles_device: prefix + copy) and the wide suppression (out of place, so every launch does the same work) --
              median over the timed calls.  The gather is stated as a share of the network call over the same tiles in the same run, for
              the real content and for the worst case: every candidate of every tile fires (1200 records per tile) and out_cap cuts.
              The kernels one by one: run this under `rocprofv3 --kernel-trace --stats` in a run of its own (--only launches).
    accuracy  images.evaluate (recall, ap) on the canvases with the pasted photographs' own untiled boxes (detect at size=56, suppressed at
              0.4), translated to the canvas, as ground truth: untiled size=56, untiled size=160, tiled.  The photographs are 56x56 frames
              upscaled, so this is a consistency figure -- does the tiled path find in a large picture what the detector finds in each
              photograph alone -- and not an accuracy claim on real large photographs.

    python tools/tiles_bench.py [--only launches|accuracy] [--iters 20] [--warmup 3] [--canvases 64]
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CW, CH, CELL_W, CELL_H = 1920, 1080, 480, 540
TILE, STRIDE, SIZE, OUT_CAP = 320, 240, 160, 1200


def canvases(photos, count, rng):
    """-> (canvases, pastes): pastes[i] = [(photo index, x, y)] of canvas i"""
    out, pastes = [], []
    for _ in range(count):
        c = np.full((CH, CW, 3), 128, np.uint8)
        placed = []
        for cell in range(8):
            k = int(rng.integers(0, len(photos)))
            h, w = photos[k].shape[:2]
            x = (cell % 4) * CELL_W + int(rng.integers(0, CELL_W - w + 1))
            y = (cell // 4) * CELL_H + int(rng.integers(0, CELL_H - h + 1))
            c[y:y + h, x:x + w] = photos[k]
            placed.append((k, x, y))
        out.append(c)
        pastes.append(placed)
    return out, pastes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--canvases", type=int, default=64)
    args = ap.parse_args()
    import torch
    from images_support import real_images
    yf = importlib.import_module("stm32h7-yolo_amd")
    images = importlib.import_module("stm32h7-yolo_amd.images")
    ptq = importlib.import_module("stm32h7-yolo_amd.ptq")
    net = yf.Network(device=0).init()
    lib = images.load()
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    photos = real_images(ptq)
    canv, pastes = canvases(photos, args.canvases, np.random.default_rng(1920))
    n = len(canv)
    print(f"# libyf_images build {(lib.yf_images_build_id() or b'').decode()}, network build {net.build_id}; {torch.cuda.get_device_name(0)}")
    print(f"# {n} canvases of {CW}x{CH} BGR, 8 photographs each; size {SIZE}, tile {TILE}x{TILE}, stride {STRIDE}, whole image first, "
          f"out_cap {OUT_CAP}, iou_threshold 0.4")

    if not args.only or args.only == "launches":
        buf, tile_desc, tiles, first = images.pack_tiles(canv, "bgr", TILE, STRIDE, True)
        t, cap = tiles.shape[0], images.CAND160
        print(f"# {t} tiles ({t // n} per canvas); {args.iters} timed calls after {args.warmup} warm-up, median of per-call device events")
        dev = "cuda"
        d_px, d_desc = torch.from_numpy(buf).to(dev), torch.from_numpy(tile_desc.view(np.uint8)).to(dev)
        d_tiles, d_first = torch.from_numpy(tiles.view(np.uint8)).to(dev), torch.from_numpy(first).to(dev)
        d_frames = torch.empty((t, SIZE, SIZE, 3), dtype=torch.int8, device=dev)
        d_heads = torch.empty((t, 20, 20, 18), dtype=torch.int8, device=dev)
        d_dets = torch.empty((t, cap, 28), dtype=torch.uint8, device=dev)
        d_counts = torch.empty(t, dtype=torch.int32, device=dev)
        d_status = torch.empty(t, dtype=torch.int32, device=dev)
        d_out = torch.empty((n, OUT_CAP, 28), dtype=torch.uint8, device=dev)
        d_totals = torch.empty(n, dtype=torch.int32, device=dev)
        d_kept = torch.empty_like(d_out)
        d_kept_counts = torch.empty_like(d_totals)
        wb = images.gather_tiles_workspace(t)
        d_work = torch.empty(wb, dtype=torch.uint8, device=dev)
        images.set_decode_tables(*net.decode_tables())

        def timed(fn):
            for _ in range(args.warmup):
                fn()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.iters)]
            for a, e in ev:
                a.record(stream)
                fn()
                e.record(stream)
            torch.cuda.synchronize()
            return float(np.median([a.elapsed_time(e) for a, e in ev])) * 1e3

        prepare = lambda: images.prepare_ragged_device(d_px.data_ptr(), buf.nbytes, "bgr", d_desc.data_ptr(), t, SIZE, d_frames.data_ptr(),
                                                       d_status.data_ptr(), stream=s)
        network = lambda: net.run_device_hw(SIZE, SIZE, d_frames.data_ptr(), d_heads.data_ptr(), t, s)
        decode = lambda: images.decode160_ragged_device(d_heads.data_ptr(), d_desc.data_ptr(), t, d_dets.data_ptr(), d_counts.data_ptr(), cap,
                                                        d_status=d_status.data_ptr(), stream=s)
        gather = lambda: images.gather_tiles_device(d_dets.data_ptr(), d_counts.data_ptr(), t, cap, d_tiles.data_ptr(), d_first.data_ptr(), n,
                                                    d_out.data_ptr(), d_totals.data_ptr(), OUT_CAP, d_work.data_ptr(), wb, stream=s)
        nms = lambda: images.nms_wide_device(d_out.data_ptr(), d_totals.data_ptr(), n, OUT_CAP, 0.4, d_kept.data_ptr(), d_kept_counts.data_ptr(),
                                             stream=s)
        t_prep, t_net, t_dec = timed(prepare), timed(network), timed(decode)

        def report(name):
            t_g, t_n = timed(gather), timed(nms)
            c, tot, k = d_counts.cpu().numpy(), d_totals.cpu().numpy(), d_kept_counts.cpu().numpy()
            print(f"{name:6s} records {int(c.sum()):8d} in {int((c > 0).sum()):5d} of {t} tiles; merged max {int(tot.max()):6d} per canvas, "
                  f"kept {int(k.sum()):6d}")
            print(f"{name:6s} gather {t_g:8.2f} us = {100 * t_g / t_net:5.2f} % of the network call; nms_wide {t_n:8.2f} us")

        print(f"real   prepare {t_prep:8.2f} us, network (band kernels) {t_net:8.2f} us, decode {t_dec:8.2f} us")
        report("real")
        h = np.random.default_rng(3).integers(-128, 128, (t, 20, 20, 18), dtype=np.int16)
        h[..., 4::6] = 120
        d_heads.copy_(torch.from_numpy(h.astype(np.int8)))
        decode()
        report("worst")

    if not args.only or args.only == "accuracy":
        own = images.detect(net, photos, "bgr", iou_threshold=0.4, size=56)
        truths = [np.concatenate([own[k] + np.array([x, y, x, y], np.int32) for k, x, y in placed]).astype(np.float64) for placed in pastes]
        print(f"# ground truth: {sum(len(g) for g in truths)} boxes, the photographs' own detect(size=56, iou_threshold=0.4) boxes translated")
        for name, kw in (("untiled size=56", dict(size=56)), ("untiled size=160", dict(size=160)),
                         ("tiled", dict(size=SIZE, tile=TILE, stride=STRIDE, whole=True))):
            r = images.evaluate(net, canv, truths, "bgr", conf_iou=0.5, iou_threshold=0.4, **kw)
            print(f"{name:17s} recall {r['recall']:.4f}  ap {r['ap']:.4f}  detections {r['detections']:6d}  true positives {r['true_positives']:5d}")
    net.destroy()


if __name__ == "__main__":
    main()
