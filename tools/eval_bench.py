#!/usr/bin/env python3
"""Time of the scoring of records against ground truth (yf_images_match_device: match_kernel; yf_images_average_precision_device: its 20
launches) at batch 4096, next to the network launch of the same run (GPU TOOL; bench.py is not involved).  Two workloads:
    real   the real-content batch of tests/test_images_gpu.py::test_uniform_equals_ragged (4096 images of 410x362 BGR: the reference's first
           sample image with 64 seeded noise patterns), images -> frames -> network + fused decode -> suppression at 0.4; the ground truth of a
           frame is its own kept boxes (up to 8), so the model scores itself
    worst  every candidate of every frame firing at one shared q_conf (147 records per frame, 602112 in all, pure tie order), 8 ground truths
           per frame taken from the frame's own records
Every timed call reads the same records and flags.  Device events around each call give a median here (they include the launch gaps of the
20 launches); kernel times: run one workload under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python
tools/eval_bench.py --only W` in a run of its own and summarise the trace with `python tools/eval_bench.py --summarize DIR`.

    python tools/eval_bench.py [--only real|worst] [--iters 50] [--warmup 5] [--threshold 0.5]
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
    """launches, median / min per launch and the sum of the medians per call (launches / calls) of every kernel in the traces below `path`"""
    times = {}
    for f in glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            times.setdefault(row["Kernel_Name"], []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    print(f"{'kernel':84s} {'n':>5s} {'median us':>10s} {'min us':>10s}")
    for name in sorted(times):
        t = times[name]
        print(f"{name[:84]:84s} {len(t):5d} {np.median(t):10.2f} {min(t):10.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--summarize", default="")
    ap.add_argument("--only", default="")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--threshold", type=float, default=0.5)
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
    n, cap, gt_cap = 4096, 147, 8
    print(f"# libyf_images build {(lib.yf_images_build_id() or b'').decode()}, network build {net.build_id}; {torch.cuda.get_device_name(0)}")
    print(f"# batch {n}, cap {cap}, gt_cap {gt_cap}, match threshold {args.threshold}; {args.iters} timed calls after {args.warmup} warm-up, "
          "median of per-call device events")
    dets = torch.zeros((n, cap, 28), dtype=torch.uint8, device="cuda")
    counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    tp = torch.zeros((n, cap), dtype=torch.uint8, device="cuda")
    best = torch.zeros((n, cap), dtype=torch.int32, device="cuda")
    work_bytes = images.average_precision_workspace(n, cap)
    work = torch.empty(work_bytes, dtype=torch.uint8, device="cuda")
    result = torch.zeros(4, dtype=torch.float64, device="cuda")
    print(f"# average precision workspace {work_bytes} bytes")

    def time(fn):
        for _ in range(args.warmup):
            fn()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.iters)]
        for a, e in ev:
            a.record(stream)
            fn()
            e.record(stream)
        torch.cuda.synchronize()
        return float(np.median([a.elapsed_time(e) for a, e in ev])) * 1e3

    def truths(pick):
        """ground truths from the records on the device: pick(m) -> the slots of a frame of m records whose boxes become its ground truth"""
        torch.cuda.synchronize()
        recs = dets.cpu().numpy().view(yf.DET_DTYPE).reshape(n, cap)
        c = np.clip(counts.cpu().numpy(), 0, cap)
        gt = np.zeros((n, gt_cap), images.GT_DTYPE)
        gt_counts = np.zeros(n, np.int32)
        for f in range(n):
            slots = pick(int(c[f]))
            gt_counts[f] = len(slots)
            for j, r in enumerate(slots):
                gt[f, j] = tuple(float(recs[f, r][e]) for e in ("x1", "y1", "x2", "y2"))
        return torch.from_numpy(gt.view(np.float64).reshape(n, gt_cap, 4)).cuda(), torch.from_numpy(gt_counts).cuda()

    def report(name, d_gt, d_gt_counts):
        def match():
            rc = lib.yf_images_match_device(dets.data_ptr(), counts.data_ptr(), n, cap, d_gt.data_ptr(), d_gt_counts.data_ptr(), gt_cap,
                                            args.threshold, tp.data_ptr(), best.data_ptr(), s)
            assert rc == n, lib.yf_images_last_error_text()

        def average_precision():
            rc = lib.yf_images_average_precision_device(dets.data_ptr(), counts.data_ptr(), tp.data_ptr(), n, cap, d_gt_counts.data_ptr(), gt_cap,
                                                        work.data_ptr(), work_bytes, result.data_ptr(), None, s)
            assert rc == n, lib.yf_images_last_error_text()
        t_match = time(match)
        t_ap = time(average_precision)
        r = result.cpu().numpy().view(images.EVAL_RESULT_DTYPE)[0]
        print(f"{name:6s} records {int(r['detections']):7d}, ground truths {int(r['ground_truths']):6d}, true positives "
              f"{int(r['true_positives']):6d}, ap {float(r['ap']):.6f}: match {t_match:8.2f} us, average precision {t_ap:8.2f} us")
        return t_match, t_ap

    H, W = 362, 410
    frames = torch.empty((n, 56, 56, 3), dtype=torch.int8, device="cuda")
    heads = torch.empty((n, 7, 7, 18), dtype=torch.int8, device="cuda")
    if not args.only or args.only == "real":
        real = np.fromfile(os.path.join(ROOT, "tests", "golden", "real_frames_56.bin"), np.int8).reshape(-1, 56, 56, 3)
        img0 = np.ascontiguousarray(ptq.resize_linear_u8((real[0].astype(np.int16) + 128).astype(np.uint8), W, H)[..., ::-1])
        g = torch.Generator(device="cuda").manual_seed(5)
        base = torch.from_numpy(img0).cuda()
        noise = torch.randint(-24, 25, (64, H, W, 3), device="cuda", generator=g, dtype=torch.int16)
        variants = (base.to(torch.int16)[None] + noise).clamp(0, 255).to(torch.uint8)
        px = variants[torch.arange(n, device="cuda") % 64].contiguous()

        def path():
            rc = lib.yf_images_run_decode_device(net.handle, px.data_ptr(), px.numel(), 0, H, W, W * 3, H * W * 3, n, frames.data_ptr(),
                                                 heads.data_ptr(), 0, dets.data_ptr(), counts.data_ptr(), cap, s)
            assert rc == n, lib.yf_images_last_error_text()

        def network():
            net.run_device(frames.data_ptr(), heads.data_ptr(), n, s)
        t_path = time(path)
        t_net = time(network)
        print(f"real   prepare + network with fused decode {t_path:8.2f} us; the network launch alone {t_net:8.2f} us")
        images.nms_device(dets.data_ptr(), counts.data_ptr(), n, cap, 0.4, stream=s)
        t_match, t_ap = report("real", *truths(lambda m: range(min(m, gt_cap))))
        print(f"real   match + average precision = {100.0 * (t_match + t_ap) / t_net:.1f} % of the network launch")
    if not args.only or args.only == "worst":
        rng = np.random.default_rng(3)
        h = rng.integers(-128, 128, (n, 7, 7, 18), dtype=np.int16)
        h[..., 4::6] = 120
        heads.copy_(torch.from_numpy(h.astype(np.int8)))
        net.decode_device(heads.data_ptr(), n, dets.data_ptr(), counts.data_ptr(), cap, w_scale=W / 56., h_scale=H / 56., stream=s)
        report("worst", *truths(lambda m: range(0, m, max(1, m // gt_cap))[:gt_cap]))
    net.destroy()


if __name__ == "__main__":
    main()
