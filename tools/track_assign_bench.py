#!/usr/bin/env python3
"""The optimal assignment on the GPU: what one launch of yf_images_track_motion_assign_device with YF_ASSIGN_OPTIMAL costs beside the
greedy motion entry, yf_images_track_motion_device, on the same records (GPU TOOL; bench.py is not involved).  For each input the two
calls are timed, interleaved in one run -- round after round the new entry, then the greedy entry, both at the suggested gains
(192, 128, 256, 0), each on a state of its own --, device events around every call, warm-up first, the median of the timed calls.  The
figures and the ratio are written to profiles/track_assign_bench.txt (--out); the notes below them in the committed file were added by
hand.  Reported, not gated: there is no earlier number for this operation.

    real      4096 pictures of 410x362 with real content (the 27 real frames of tests/golden upscaled to that size, repeated): the ragged
              run at 56x56 and the suppression at 0.4 leave the records.  4096 streams x 1 step with the state carried from call to call,
              then the same 4096 frames as 64 streams x 64 steps.
    never     64 detections per frame that never match, with full tables (refilled before every timed call, outside the events): no
              eligible pair, the search is skipped.  4096 streams x 1 step and 64 streams x 64 steps.
    dense     64 tracks at one box and 64 detections at one box beside it: every pair eligible with the same weight, 2080 rounds of the
              search per step (tables refilled before every timed call).  4096 streams x 1 step and 64 streams x 64 steps.

Then, on the host with the plain-Python statement (ptq.track_motion_step), the frames on which the two matches report different tracks:
on the real records as 64 streams x 64 steps, and on a synthetic sequence of two faces that pass each other.

    python tools/track_assign_bench.py [--iters 30] [--warmup 5] [--out profiles/track_assign_bench.txt]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_assign_bench.txt"))
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
    say(f"# {args.iters} timed rounds after {args.warmup} warm-up, the two calls interleaved in every round, median of per-call device events")

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

    # the two calls, each with a state of its own: (name, entry)
    gains = images.MOTION_GAINS + (0,)

    def optimal(dd, dc, streams, steps, layout, dcap, params, *rest):
        return images.track_motion_assign_device(dd, dc, streams, steps, layout, dcap, params, "optimal", *rest)
    kinds = [("optimal", optimal), ("greedy", images.track_motion_device)]
    states = [torch.zeros((n, images.TRACK_MOTION_STATE_BYTES), dtype=torch.uint8, device=dev) for _ in kinds]

    def call(k, streams, steps, base, dd, dc, dcap):
        kinds[k][1](dd.data_ptr(), dc.data_ptr(), streams, steps, "time", dcap, tuple(base) + gains, states[k].data_ptr(), d_out.data_ptr(),
                    d_info.data_ptr(), d_oc.data_ptr(), out_cap, d_status.data_ptr(), s)

    def measure(name, what, streams, steps, base, dd, dc, dcap, before=None):
        """round after round the two calls; `before(k)` runs ahead of call k, outside the events"""
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
        say(f"{name:5s} {what:52s} " + "; ".join(f"{kinds[k][0]} {t[k]:9.2f} us" for k in range(2)) + f"; ratio to the greedy entry {t[0] / t[1]:6.2f}")

    default = (0.3, 1, 5)
    measure("real", "4096 streams x 1 step, state carried", n, 1, default, d_dets, d_counts, cap)
    measure("real", "64 streams x 64 steps, state carried", 64, 64, default, d_dets, d_counts, cap)

    # ---- nothing matches ----  frame f: 64 disjoint 6x6 boxes on a grid of pitch 8 whose origin moves by 1000 pixels with every frame and step
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
    measure("never", "4096 streams x 1 step, full tables, nothing matches", n, 1, never, d_wdets, d_wcounts, wcap, before=full_tables(n))
    measure("never", "64 streams x 64 steps, full tables, nothing matches", 64, 64, never, d_wdets, d_wcounts, wcap, before=full_tables(64))
    torch.cuda.synchronize()
    say(f"# after the last call: emitted {int(d_oc.sum().item())}, status bits {int(d_status.cpu().numpy().max())}")

    # ---- dense ----  64 tracks born at one box, then 64 detections at one box two pixels beside it: all 4096 pairs eligible, one weight
    for name, box in (("fill", (10, 10, 49, 59)), ("dets", (12, 10, 51, 59))):
        for e, v in zip(("x1", "y1", "x2", "y2"), box):
            (fill if name == "fill" else dets)[e] = v
    d_fill.copy_(torch.from_numpy(fill.view(np.uint8).reshape(n, wcap, 28)))
    d_wdets.copy_(torch.from_numpy(dets.view(np.uint8).reshape(n, wcap, 28)))
    measure("dense", "4096 streams x 1 step, 64 x 64 equal weights", n, 1, never, d_wdets, d_wcounts, wcap, before=full_tables(n))
    measure("dense", "64 streams x 64 steps, 64 x 64 equal weights", 64, 64, never, d_wdets, d_wcounts, wcap, before=full_tables(64))
    torch.cuda.synchronize()
    emitted, misses = d_oc.cpu().numpy(), d_info.cpu().numpy().view(images.TRACK_INFO_DTYPE).reshape(n, out_cap)["misses"]
    say(f"# after the last call: every frame emits {int(emitted[:4096].min())} .. {int(emitted[:4096].max())} tracks, misses at most {int(misses.max())}")

    # ---- on the host: the frames on which the two matches report different tracks ----
    recs, cnt = d_dets.cpu().numpy().view(binding.DET_DTYPE).reshape(n, cap), np.clip(counts, 0, cap)

    def differing(frames_of, streams, steps, params):
        frames = 0
        issued = {}
        for st in range(streams):
            state = {a: ptq.track_motion_empty_state() for a in ptq.ASSIGNS}
            for t in range(steps):
                out = {}
                for a in ptq.ASSIGNS:
                    state[a], out[a], _ = ptq.track_motion_step(state[a], frames_of(st, t), params, frame=0, assign=a)
                frames += out["greedy"] != out["optimal"]
            for a in ptq.ASSIGNS:
                issued[a] = issued.get(a, 0) + state[a]["issued"]
        return frames, issued
    frames, issued = differing(lambda st, t: recs[t * 64 + st, :cnt[t * 64 + st]].tolist(), 64, 64, default + gains)
    say(f"differ real  64 streams x 64 steps of the real records: {frames} of 4096 frames differ; ids issued {issued}")

    def crossing(st, t):                                            # P moves right by 40 a step, Q left by 5; stream 1: a pan by 33 a step
        if st == 0:
            px, qx = -150 + 40 * t + (3 if t % 3 == 0 else 0), 150 - 5 * t
            boxes = [(px, 0, px + 99, 99), (qx, 3, qx + 99, 102)]
        else:
            boxes = [(-33 * t, 0, -33 * t + 99, 99), (58 - 33 * t, 0, 157 - 33 * t, 99)]
        return [(0, 0, 0, 0, 0, 0.9, *b) for b in boxes]
    for g in ((256, 0, 256, 0), gains):
        frames, issued = differing(crossing, 2, 12, default + g)
        say(f"differ synth two faces passing (12 steps) and a pan (12 steps) at gains {g}: {frames} of 24 frames differ; ids issued {issued}")
    net.destroy()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
