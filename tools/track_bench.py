#!/usr/bin/env python3
"""The tracker on the GPU: what one launch of yf_images_track_device costs (GPU TOOL; bench.py is not involved).  Device events around
every call, warm-up first, the median of the timed calls, as tools/redact_bench.py does; beside each figure the suppression
(yf_images_nms_device into buffers of its own) on the same records and the network launch (yf_network_run_device over 4096 frames) in the
same run.  The figures are written to profiles/track_bench.txt (--out); the notes below them in the committed file were added by hand.

    real      4096 pictures of 410x362 with real content (the 27 real frames of tests/golden upscaled to that size, repeated): the ragged
              run at 56x56 and the suppression at 0.4 leave the records.  4096 streams x 1 step, the state carried from call to call
              (every box is seen again: all matches) and from the empty state (all births: the state is zeroed before every timed call,
              outside the events); then the same 4096 frames as 64 streams x 64 steps, where a stream sees another picture at every step.
    worst     64 detections per frame that never match, with full tables: disjoint boxes that lie elsewhere at every step, max_misses at
              INT32_MAX, so after the first step every table holds 64 tracks, every step computes 64 x 64 IoUs, matches nothing and drops
              its 64 detections.  4096 streams x 1 step and 64 streams x 64 steps.

    python tools/track_bench.py [--iters 30] [--warmup 5] [--out profiles/track_bench.txt]
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 410, 362


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_bench.txt"))
    args = ap.parse_args()
    import torch
    yf = importlib.import_module("stm32h7-yolo_amd")
    images = importlib.import_module("stm32h7-yolo_amd.images")
    ptq = importlib.import_module("stm32h7-yolo_amd.ptq")
    binding = importlib.import_module("stm32h7-yolo_amd.binding")
    net = yf.Network(device=0).init()
    lib = images.load()
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    dev = "cuda"
    n, cap, out_cap = 4096, 147, 64
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"# libyf_images build {(lib.yf_images_build_id() or b'').decode()}, network build {net.build_id}; {torch.cuda.get_device_name(0)}")
    say(f"# {args.iters} timed calls after {args.warmup} warm-up, median of per-call device events")

    def timed(fn, before=None):
        """the median (us) of the call; `before` runs ahead of every call, outside the events"""
        for _ in range(args.warmup):
            if before:
                before()
            fn()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.iters)]
        for a, b in ev:
            if before:
                before()
            a.record(stream)
            fn()
            b.record(stream)
        torch.cuda.synchronize()
        return float(np.median([a.elapsed_time(b) for a, b in ev])) * 1e3

    real = np.fromfile(os.path.join(ROOT, "tests", "golden", "real_frames_56.bin"), np.int8).reshape(-1, 56, 56, 3)
    rgb56 = (real.astype(np.int16) + 128).astype(np.uint8)
    photos = [np.ascontiguousarray(ptq.resize_linear_u8(f, W, H)[..., ::-1]) for f in rgb56]
    size = (H * W * 3 + 15) // 16 * 16
    desc = np.zeros(n, images.IMAGE_DTYPE)
    desc["offset"], desc["height"], desc["width"], desc["row_stride"] = np.arange(n, dtype=np.int64) * size, H, W, W * 3
    nbytes = int(desc["offset"][-1]) + H * W * 3
    buf = np.zeros(nbytes, np.uint8)
    for i in range(n):
        o = int(desc["offset"][i])
        buf[o:o + H * W * 3] = photos[i % len(photos)].reshape(-1)
    d_px, d_desc = torch.from_numpy(buf).to(dev), torch.from_numpy(desc.view(np.uint8)).to(dev)
    d_frames = torch.empty((n, 56, 56, 3), dtype=torch.int8, device=dev)
    d_heads = torch.empty((n, 7, 7, 18), dtype=torch.int8, device=dev)
    d_dets = torch.empty((n, cap, 28), dtype=torch.uint8, device=dev)
    d_counts = torch.empty(n, dtype=torch.int32, device=dev)
    d_status = torch.empty(n, dtype=torch.int32, device=dev)
    d_nms, d_nms_counts = torch.empty_like(d_dets), torch.empty_like(d_counts)
    d_out = torch.empty((n, out_cap, 28), dtype=torch.uint8, device=dev)
    d_info = torch.empty((n, out_cap, 16), dtype=torch.uint8, device=dev)
    d_oc = torch.empty(n, dtype=torch.int32, device=dev)
    d_state = torch.zeros((n, images.TRACK_STATE_BYTES), dtype=torch.uint8, device=dev)
    images.set_decode_tables(*net.decode_tables())
    network = lambda: net.run_device(d_frames.data_ptr(), d_heads.data_ptr(), n, s)
    nms = lambda: images.nms_device(d_dets.data_ptr(), d_counts.data_ptr(), n, cap, 0.4, d_nms.data_ptr(), d_nms_counts.data_ptr(), stream=s)

    def track(streams, steps, params, dd=None, dc=None, dcap=cap):
        dd, dc = d_dets if dd is None else dd, d_counts if dc is None else dc
        return lambda: images.track_device(dd.data_ptr(), dc.data_ptr(), streams, steps, "time", dcap, params, d_state.data_ptr(), d_out.data_ptr(),
                                           d_info.data_ptr(), d_oc.data_ptr(), out_cap, d_status.data_ptr(), s)

    def line(name, what, t, t_nms, t_net):
        torch.cuda.synchronize()
        say(f"{name:5s} {what:58s} track {t:8.2f} us = {t / t_nms:6.2f} x the suppression, {100 * t / t_net:6.2f} % of the network call; "
            f"emitted {int(d_oc.sum().item())}, status bits {int(d_status.cpu().numpy().max())}")

    # ---- real content ----
    images.run_decode_ragged_device(net, d_px.data_ptr(), nbytes, "bgr", d_desc.data_ptr(), n, d_frames.data_ptr(), d_heads.data_ptr(),
                                    d_dets.data_ptr(), d_counts.data_ptr(), cap, d_status.data_ptr(), stream=s)
    images.nms_device(d_dets.data_ptr(), d_counts.data_ptr(), n, cap, 0.4, stream=s)
    torch.cuda.synchronize()
    counts = d_counts.cpu().numpy()
    t_net, t_nms = timed(network), timed(nms)
    say(f"real  {n} x {W}x{H}, {int(np.clip(counts, 0, cap).sum())} records after the suppression (at most {int(counts.max())} per frame); "
        f"network call {t_net:8.2f} us, suppression of the same records again {t_nms:8.2f} us")
    default = (0.3, 1, 5)
    d_state.zero_()
    line("real", "4096 streams x 1 step, state carried (all matches)", timed(track(n, 1, default)), t_nms, t_net)
    line("real", "4096 streams x 1 step, from the empty state (all births)", timed(track(n, 1, default), before=d_state.zero_), t_nms, t_net)
    d_state.zero_()
    line("real", "64 streams x 64 steps, state carried", timed(track(64, 64, default)), t_nms, t_net)
    line("real", "64 streams x 64 steps, from the empty state", timed(track(64, 64, default), before=d_state.zero_), t_nms, t_net)

    # ---- worst case ----  frame f: 64 disjoint 6x6 boxes on a grid of pitch 8 whose origin moves by 1000 pixels with every frame and step
    wcap = 64
    dets = np.zeros((n, wcap), binding.DET_DTYPE)
    k = np.arange(wcap)
    for f in range(n):
        x, y = (k % 8) * 8 + 1000 * (f % 7), (k // 8) * 8 + 1000 * (f // 64 % 5)
        dets[f]["x1"], dets[f]["y1"], dets[f]["x2"], dets[f]["y2"], dets[f]["conf"] = x, y, x + 5, y + 5, 0.9
    d_wdets = torch.from_numpy(dets.view(np.uint8).reshape(n, wcap, 28)).to(dev)
    d_wcounts = torch.full((n,), wcap, dtype=torch.int32, device=dev)
    t_wnms = timed(lambda: images.nms_device(d_wdets.data_ptr(), d_wcounts.data_ptr(), n, wcap, 0.4, d_nms.data_ptr(), d_nms_counts.data_ptr(), stream=s))
    say(f"worst {n} frames of 64 disjoint records; suppression of the same records {t_wnms:8.2f} us")
    never = (0.3, 1, 2 ** 31 - 1)
    # tables filled by boxes that lie nowhere near: one step over a frame of the same kind, shifted
    fill = dets.copy()
    for name in ("x1", "x2"):
        fill[name] += 100000
    d_fill = torch.from_numpy(fill.view(np.uint8).reshape(n, wcap, 28)).to(dev)

    def full_tables(streams):
        def go():
            d_state.zero_()
            images.track_device(d_fill.data_ptr(), d_wcounts.data_ptr(), streams, 1, "time", wcap, never, d_state.data_ptr(), d_out.data_ptr(),
                                d_info.data_ptr(), d_oc.data_ptr(), out_cap, d_status.data_ptr(), s)
        return go
    line("worst", "4096 streams x 1 step, full tables, nothing matches", timed(track(n, 1, never, d_wdets, d_wcounts, wcap), before=full_tables(n)),
         t_wnms, t_net)
    line("worst", "64 streams x 64 steps, full tables, nothing matches", timed(track(64, 64, never, d_wdets, d_wcounts, wcap), before=full_tables(64)),
         t_wnms, t_net)
    net.destroy()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
