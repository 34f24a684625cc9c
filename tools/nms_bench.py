#!/usr/bin/env python3
"""Time of the IoU suppression (yf_images_nms_device, nms_kernel) at batch 4096, next to the network launch (GPU TOOL; bench.py is not
involved).  Two workloads:
    real   the real-content batch of tests/test_images_gpu.py::test_uniform_equals_ragged (4096 images of 410x362 BGR: the reference's first
           sample image with 64 seeded noise patterns), images -> frames -> network + fused decode (yf_images_run_decode_device), then NMS
    worst  every candidate of every frame firing at one shared q_conf (147 records per frame, pure tie order), then NMS
Each launch reads the same records and writes a separate output (out of place), so every timed launch does the same work.  Device events
around each launch give a median here; kernel times: run this under `rocprofv3 --kernel-trace --stats` in a run of its own.

    python tools/nms_bench.py [--only real|worst] [--iters 50] [--warmup 5] [--threshold 0.4]
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--threshold", type=float, default=0.4)
    args = ap.parse_args()
    import torch
    yf = importlib.import_module("stm32h7-yolo_amd")
    images = importlib.import_module("stm32h7-yolo_amd.images")
    ptq = importlib.import_module("stm32h7-yolo_amd.ptq")
    net = yf.Network(device=0).init()
    lib = images.load()
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    n, cap = 4096, 147
    print(f"# libyf_images build {(lib.yf_images_build_id() or b'').decode()}, network build {net.build_id}; {torch.cuda.get_device_name(0)}")
    print(f"# batch {n}, cap {cap}, iou_threshold {args.threshold}; {args.iters} timed launches after {args.warmup} warm-up, "
          "median of per-launch device events")
    dets = torch.zeros((n, cap, 28), dtype=torch.uint8, device="cuda")
    counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    out = torch.empty_like(dets)
    out_counts = torch.empty_like(counts)

    def time(fn):
        for i in range(args.warmup):
            fn()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.iters)]
        for a, e in ev:
            a.record(stream)
            fn()
            e.record(stream)
        torch.cuda.synchronize()
        return float(np.median([a.elapsed_time(e) for a, e in ev])) * 1e3

    def nms():
        rc = lib.yf_images_nms_device(dets.data_ptr(), counts.data_ptr(), n, cap, args.threshold, out.data_ptr(), out_counts.data_ptr(), s)
        assert rc == n, lib.yf_images_last_error_text()

    def report(name):
        t = time(nms)
        c, k = counts.cpu().numpy(), out_counts.cpu().numpy()
        print(f"{name:6s} records in {int(c.sum()):7d} (max {int(c.max())} per frame), kept {int(k.sum()):7d}: nms {t:7.2f} us")

    if not args.only or args.only == "real":
        # the batch of test_uniform_equals_ragged
        H, W = 362, 410
        real = np.fromfile(os.path.join(ROOT, "tests", "golden", "real_frames_56.bin"), np.int8).reshape(-1, 56, 56, 3)
        img0 = np.ascontiguousarray(ptq.resize_linear_u8((real[0].astype(np.int16) + 128).astype(np.uint8), W, H)[..., ::-1])
        g = torch.Generator(device="cuda").manual_seed(5)
        base = torch.from_numpy(img0).cuda()
        noise = torch.randint(-24, 25, (64, H, W, 3), device="cuda", generator=g, dtype=torch.int16)
        variants = (base.to(torch.int16)[None] + noise).clamp(0, 255).to(torch.uint8)
        px = variants[torch.arange(n, device="cuda") % 64].contiguous()
        frames = torch.empty((n, 56, 56, 3), dtype=torch.int8, device="cuda")
        heads = torch.empty((n, 7, 7, 18), dtype=torch.int8, device="cuda")

        def network():
            rc = lib.yf_images_run_decode_device(net.handle, px.data_ptr(), px.numel(), 0, H, W, W * 3, H * W * 3, n, frames.data_ptr(),
                                                 heads.data_ptr(), 0, dets.data_ptr(), counts.data_ptr(), cap, s)
            assert rc == n, lib.yf_images_last_error_text()
        t_net = time(network)
        print(f"real   prepare + network with fused decode {t_net:7.2f} us")
        report("real")
    if not args.only or args.only == "worst":
        heads = torch.full((n, 7, 7, 18), 0, dtype=torch.int8, device="cuda")
        rng = np.random.default_rng(3)
        h = rng.integers(-128, 128, (n, 7, 7, 18), dtype=np.int16)
        h[..., 4::6] = 120
        heads.copy_(torch.from_numpy(h.astype(np.int8)))
        net.decode_device(heads.data_ptr(), n, dets.data_ptr(), counts.data_ptr(), cap, w_scale=410 / 56., h_scale=362 / 56., stream=s)
        report("worst")
    net.destroy()


if __name__ == "__main__":
    main()
