#!/usr/bin/env python3
"""The tracker with a motion model on the GPU: what one launch of yf_images_track_motion_device costs beside yf_images_track_device on
the same records (GPU TOOL; bench.py is not involved).  The inputs are tools/track_bench.py's; for each input three calls are timed,
interleaved in one run -- round after round the new entry at the suggested gains (192, 128, 256, 0), the new entry at (256, 0, 256, 0),
which computes the base tracker's bytes, and the base entry, each on a state of its own --, device events around every call, warm-up
first, the median of the timed calls.  The figures and the two ratios are written to profiles/track_motion_bench.txt (--out); the notes
below them in the committed file were added by hand.  Reported, not gated: there is no earlier number for this operation.

    real      4096 pictures of 410x362 with real content (the 27 real frames of tests/golden upscaled to that size, repeated): the ragged
              run at 56x56 and the suppression at 0.4 leave the records.  4096 streams x 1 step with the state carried from call to call,
              then the same 4096 frames as 64 streams x 64 steps.
    worst     64 detections per frame that never match, with full tables (refilled before every timed call, outside the events):
              4096 streams x 1 step and 64 streams x 64 steps.

    python tools/track_motion_bench.py [--iters 30] [--warmup 5] [--out profiles/track_motion_bench.txt]
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 410, 362


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_motion_bench.txt"))
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
    say(f"# {args.iters} timed rounds after {args.warmup} warm-up, the three calls interleaved in every round, median of per-call device events")

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
    d_out = torch.empty((n, out_cap, 28), dtype=torch.uint8, device=dev)
    d_info = torch.empty((n, out_cap, 16), dtype=torch.uint8, device=dev)
    d_oc = torch.empty(n, dtype=torch.int32, device=dev)
    images.set_decode_tables(*net.decode_tables())
    images.run_decode_ragged_device(net, d_px.data_ptr(), nbytes, "bgr", d_desc.data_ptr(), n, d_frames.data_ptr(), d_heads.data_ptr(),
                                    d_dets.data_ptr(), d_counts.data_ptr(), cap, d_status.data_ptr(), stream=s)
    images.nms_device(d_dets.data_ptr(), d_counts.data_ptr(), n, cap, 0.4, stream=s)
    torch.cuda.synchronize()
    counts = d_counts.cpu().numpy()
    say(f"real  {n} x {W}x{H}, {int(np.clip(counts, 0, cap).sum())} records after the suppression (at most {int(counts.max())} per frame)")

    # the three calls, each with a state of its own: (name, entry, the gains behind the base params, the bytes of a stream's state)
    kinds = [("motion (192, 128, 256, 0)", images.track_motion_device, images.MOTION_GAINS + (0,), images.TRACK_MOTION_STATE_BYTES),
             ("motion (256, 0, 256, 0)", images.track_motion_device, (256, 0, 256, 0), images.TRACK_MOTION_STATE_BYTES),
             ("base entry", images.track_device, (), images.TRACK_STATE_BYTES)]
    states = [torch.zeros((n, nb), dtype=torch.uint8, device=dev) for _, _, _, nb in kinds]

    def call(k, streams, steps, base, dd, dc, dcap):
        _, entry, gains, _ = kinds[k]
        entry(dd.data_ptr(), dc.data_ptr(), streams, steps, "time", dcap, tuple(base) + gains, states[k].data_ptr(), d_out.data_ptr(),
              d_info.data_ptr(), d_oc.data_ptr(), out_cap, d_status.data_ptr(), s)

    def measure(name, what, streams, steps, base, dd, dc, dcap, before=None):
        """round after round the three calls; `before(k)` runs ahead of call k, outside the events"""
        for st in states:
            st.zero_()
        ev = [[] for _ in kinds]
        for it in range(args.warmup + args.iters):
            for k in range(len(kinds)):
                if before:
                    before(k)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                call(k, streams, steps, base, dd, dc, dcap)
                b.record(stream)
                if it >= args.warmup:
                    ev[k].append((a, b))
        torch.cuda.synchronize()
        t = [float(np.median([a.elapsed_time(b) for a, b in e])) * 1e3 for e in ev]
        say(f"{name:5s} {what:52s} " + "; ".join(f"{kinds[k][0]} {t[k]:8.2f} us" for k in range(3))
            + f"; ratios to the base entry {t[0] / t[2]:5.2f} and {t[1] / t[2]:5.2f}")

    default = (0.3, 1, 5)
    measure("real", "4096 streams x 1 step, state carried", n, 1, default, d_dets, d_counts, cap)
    measure("real", "64 streams x 64 steps, state carried", 64, 64, default, d_dets, d_counts, cap)

    # ---- worst case ----  frame f: 64 disjoint 6x6 boxes on a grid of pitch 8 whose origin moves by 1000 pixels with every frame and step
    wcap = 64
    dets = np.zeros((n, wcap), binding.DET_DTYPE)
    k = np.arange(wcap)
    for f in range(n):
        x, y = (k % 8) * 8 + 1000 * (f % 7), (k // 8) * 8 + 1000 * (f // 64 % 5)
        dets[f]["x1"], dets[f]["y1"], dets[f]["x2"], dets[f]["y2"], dets[f]["conf"] = x, y, x + 5, y + 5, 0.9
    d_wdets = torch.from_numpy(dets.view(np.uint8).reshape(n, wcap, 28)).to(dev)
    d_wcounts = torch.full((n,), wcap, dtype=torch.int32, device=dev)
    never = (0.3, 1, 2 ** 31 - 1)
    fill = dets.copy()
    for name in ("x1", "x2"):
        fill[name] += 100000
    d_fill = torch.from_numpy(fill.view(np.uint8).reshape(n, wcap, 28)).to(dev)

    def full_tables(streams):
        def go(k):                                                  # tables filled by boxes that lie nowhere near, born in one step
            states[k].zero_()
            call(k, streams, 1, never, d_fill, d_wcounts, wcap)
        return go
    measure("worst", "4096 streams x 1 step, full tables, nothing matches", n, 1, never, d_wdets, d_wcounts, wcap, before=full_tables(n))
    measure("worst", "64 streams x 64 steps, full tables, nothing matches", 64, 64, never, d_wdets, d_wcounts, wcap, before=full_tables(64))
    torch.cuda.synchronize()
    say(f"# after the last call: emitted {int(d_oc.sum().item())}, status bits {int(d_status.cpu().numpy().max())}")
    net.destroy()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
