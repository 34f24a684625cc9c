#!/usr/bin/env python3
"""Time of the boxes at 160x160 (decode160_kernel, nms_wide_kernel of libyf_images.so) at batch 1024, next to the three band kernels of the
160x160 network launch (GPU TOOL; bench.py is not involved).  Workloads:
    real   1024 images of 410x362 BGR built like tests/test_images_gpu.py::test_uniform_equals_ragged's batch (the reference's first sample
           image with 64 seeded noise patterns): images -> 160x160 frames -> heads -> records (yf_images_run_decode160_device), then
           yf_images_nms_wide_device at the threshold
    cmp    the same records through nms_wide_kernel and, re-packed at cap 147 where every count allows it, through the 256-record nms_kernel
    worst  every candidate of every frame firing at one shared q_conf (1200 records per frame, pure tie order): decode160, then nms_wide
The suppression is timed out of place (every launch reads the same records).  Device events around each launch give a median here; kernel
times: run one workload under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/boxes160_bench.py --only W` and
summarise the trace with `python tools/boxes160_bench.py --summarize DIR`.

    python tools/boxes160_bench.py [--only real|cmp|worst] [--iters 50] [--warmup 5] [--threshold 0.4] [--worst-iters 3]
"""
import argparse
import csv
import glob
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summarize(path):
    """median / min per kernel of every *kernel_trace.csv below `path`"""
    times = {}
    for f in glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            times.setdefault(row["Kernel_Name"], []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    print(f"{'kernel':90s} {'n':>5s} {'median us':>10s} {'min us':>10s}")
    for name in sorted(times):
        t = times[name]
        print(f"{name[:90]:90s} {len(t):5d} {np.median(t):10.2f} {min(t):10.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--worst-iters", type=int, default=3)
    ap.add_argument("--threshold", type=float, default=0.4)
    ap.add_argument("--summarize", default="")
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize)
    import torch
    yf = importlib.import_module("stm32h7-yolo_amd")
    images = importlib.import_module("stm32h7-yolo_amd.images")
    ptq = importlib.import_module("stm32h7-yolo_amd.ptq")
    net = yf.Network(device=0).init()
    lib = images.load()
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    n, cap = 1024, images.CAND160
    print(f"# libyf_images build {(lib.yf_images_build_id() or b'').decode()}, network build {net.build_id}; {torch.cuda.get_device_name(0)}")
    print(f"# batch {n}, cap {cap}, iou_threshold {args.threshold}; {args.iters} timed launches after {args.warmup} warm-up "
          f"({args.worst_iters} after 1 for the worst case's suppression), median of per-launch device events")
    dets = torch.zeros((n, cap, 28), dtype=torch.uint8, device="cuda")
    counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    out = torch.empty_like(dets)
    out_counts = torch.empty_like(counts)
    heads = torch.zeros((n, 20, 20, 18), dtype=torch.int8, device="cuda")

    def time(fn, iters=args.iters, warmup=args.warmup):
        for _ in range(warmup):
            fn()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
        for a, e in ev:
            a.record(stream)
            fn()
            e.record(stream)
        torch.cuda.synchronize()
        return float(np.median([a.elapsed_time(e) for a, e in ev])) * 1e3

    def ok(rc):
        assert rc == n, lib.yf_images_last_error_text()

    def decode():
        ok(lib.yf_images_decode160_device(heads.data_ptr(), n, 410 / 160., 362 / 160., dets.data_ptr(), counts.data_ptr(), cap, s))

    def nms_wide():
        ok(lib.yf_images_nms_wide_device(dets.data_ptr(), counts.data_ptr(), n, cap, args.threshold, out.data_ptr(), out_counts.data_ptr(), s))

    def totals():
        c, k = counts.cpu().numpy(), out_counts.cpu().numpy()
        return f"records in {int(c.sum())} (max {int(c.max())} per frame), kept {int(k.sum())}"

    if args.only in ("", "real", "cmp"):
        H, W = 362, 410
        real = np.fromfile(os.path.join(ROOT, "tests", "golden", "real_frames_56.bin"), np.int8).reshape(-1, 56, 56, 3)
        img0 = np.ascontiguousarray(ptq.resize_linear_u8((real[0].astype(np.int16) + 128).astype(np.uint8), W, H)[..., ::-1])
        g = torch.Generator(device="cuda").manual_seed(5)
        base = torch.from_numpy(img0).cuda()
        noise = torch.randint(-24, 25, (64, H, W, 3), device="cuda", generator=g, dtype=torch.int16)
        variants = (base.to(torch.int16)[None] + noise).clamp(0, 255).to(torch.uint8)
        px = variants[torch.arange(n, device="cuda") % 64].contiguous()
        frames = torch.empty((n, 160, 160, 3), dtype=torch.int8, device="cuda")

        def path():
            ok(lib.yf_images_run_decode160_device(net.handle, px.data_ptr(), px.numel(), 0, H, W, W * 3, H * W * 3, n, frames.data_ptr(),
                                                  heads.data_ptr(), dets.data_ptr(), counts.data_ptr(), cap, s))
        if args.only != "cmp":
            print(f"real   prepare(160) + network + decode160 {time(path):8.2f} us")
            print(f"real   decode160 {time(decode):8.2f} us")
            t = time(nms_wide)
            print(f"real   nms_wide  {t:8.2f} us; {totals()}")
        else:
            path()
        if args.only in ("", "cmp"):
            t_wide = time(nms_wide)
            c = counts.cpu().numpy()
            if c.max() <= 147:
                d147 = dets[:, :147].contiguous()
                o147 = torch.empty_like(d147)

                def nms_256():
                    ok(lib.yf_images_nms_device(d147.data_ptr(), counts.data_ptr(), n, 147, args.threshold, o147.data_ptr(), out_counts.data_ptr(), s))
                print(f"cmp    the same records: nms_wide (cap 1200) {t_wide:8.2f} us, nms_kernel (re-packed at cap 147) {time(nms_256):8.2f} us")
            else:
                print(f"cmp    nms_wide {t_wide:8.2f} us; a frame has {int(c.max())} records: no re-pack at cap 147")
    if args.only in ("", "worst"):
        rng = np.random.default_rng(3)
        h = rng.integers(-128, 128, (n, 20, 20, 18), dtype=np.int16)
        h[..., 4::6] = 120
        heads.copy_(torch.from_numpy(h.astype(np.int8)))
        print(f"worst  decode160 {time(decode):8.2f} us")
        t = time(nms_wide, args.worst_iters, 1)
        print(f"worst  nms_wide  {t:8.2f} us; {totals()}")
    net.destroy()


if __name__ == "__main__":
    main()
