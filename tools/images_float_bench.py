#!/usr/bin/env python3
"""Time of the fp16 image path (prepare_f16_kernel, decode_f32_kernel of libyf_images.so) at batch 4096 of 410x362 BGR, beside the int8
path's kernels in the same run (GPU TOOL; bench.py is not involved).  Workloads:
    prep    the int8 prepare and the fp16 prepare of the same images (uniform batch)
    decode  decode_ragged_kernel on the int8 heads of the batch, decode_f32_kernel (per-image scales) on the fp16 network's logits of the
            batch, on logits whose 147 candidates all fire (worst case) and on logits of which none fires (the confidence pass alone),
            and the fp16 network launch they follow
    path    images -> frames -> network -> records, int8 (yf_images_run_decode_device) and fp16 (yf_images_run_decode_f16_device)
Device events around each launch give a median here; kernel times: run one workload under
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/images_float_bench.py --only W` and summarise the trace with
`python tools/images_float_bench.py --summarize DIR`.

    python tools/images_float_bench.py [--only prep|decode|path] [--n 4096] [--iters 50] [--warmup 5]
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
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--summarize", default="")
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize)
    import torch
    yf = importlib.import_module("stm32h7-yolo_amd")
    images = importlib.import_module("stm32h7-yolo_amd.images")
    ptq = importlib.import_module("stm32h7-yolo_amd.ptq")
    net = yf.Network(device=0).init()
    net.fp16_init()
    lib = images.load()
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    n, cap, H, W = args.n, 147, 362, 410
    print(f"# libyf_images build {(lib.yf_images_build_id() or b'').decode()}, network build {net.build_id}; {torch.cuda.get_device_name(0)}")
    print(f"# batch {n} of {W}x{H} BGR, cap {cap}; {args.iters} timed launches after {args.warmup} warm-up, median of per-launch device events")

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

    def ok(rc):
        assert rc == n, lib.yf_images_last_error_text()

    # the batch of tests/test_images_gpu.py::test_uniform_equals_ragged: the reference's first sample image with 64 seeded noise patterns
    real = np.fromfile(os.path.join(ROOT, "tests", "golden", "real_frames_56.bin"), np.int8).reshape(-1, 56, 56, 3)
    img0 = np.ascontiguousarray(ptq.resize_linear_u8((real[0].astype(np.int16) + 128).astype(np.uint8), W, H)[..., ::-1])
    g = torch.Generator(device="cuda").manual_seed(5)
    noise = torch.randint(-24, 25, (64, H, W, 3), device="cuda", generator=g, dtype=torch.int16)
    variants = (torch.from_numpy(img0).cuda().to(torch.int16)[None] + noise).clamp(0, 255).to(torch.uint8)
    px = variants[torch.arange(n, device="cuda") % 64].contiguous()
    geom = (px.data_ptr(), px.numel(), 0, H, W, W * 3, H * W * 3, n)
    f8 = torch.empty((n, 56, 56, 3), dtype=torch.int8, device="cuda")
    f16 = torch.empty((n, 56, 56, 3), dtype=torch.float16, device="cuda")
    heads = torch.empty((n, 7, 7, 18), dtype=torch.int8, device="cuda")
    logits = torch.empty((n, 7, 7, 18), dtype=torch.float32, device="cuda")
    dets = torch.zeros((n, cap, 28), dtype=torch.uint8, device="cuda")
    counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    desc = np.zeros(n, images.IMAGE_DTYPE)
    desc["offset"], desc["height"], desc["width"], desc["row_stride"] = np.arange(n) * H * W * 3, H, W, W * 3
    d_desc = torch.from_numpy(desc.view(np.uint8)).cuda()

    def path8():
        ok(lib.yf_images_run_decode_device(net.handle, *geom, f8.data_ptr(), heads.data_ptr(), 0, dets.data_ptr(), counts.data_ptr(), cap, s))

    def path16():
        ok(lib.yf_images_run_decode_f16_device(net.handle, *geom, f16.data_ptr(), logits.data_ptr(), dets.data_ptr(), counts.data_ptr(), cap, s))

    if args.only in ("", "prep"):
        t8 = time(lambda: ok(lib.yf_images_prepare_device(*geom, 56, f8.data_ptr(), s)))
        t16 = time(lambda: ok(lib.yf_images_prepare_f16_device(*geom, f16.data_ptr(), s)))
        print(f"prep   int8 prepare {t8:8.2f} us, fp16 prepare {t16:8.2f} us, ratio {t16 / t8:.3f}")
    if args.only in ("", "decode"):
        path8()
        path16()
        torch.cuda.synchronize()

        def dec8():
            ok(lib.yf_images_decode_ragged_device(heads.data_ptr(), d_desc.data_ptr(), n, 0, dets.data_ptr(), counts.data_ptr(), cap, s))

        def dec32(lg):
            return lambda: ok(lib.yf_images_decode_f32_ragged_device(lg.data_ptr(), d_desc.data_ptr(), None, n, dets.data_ptr(), counts.data_ptr(), cap, s))
        t_net = time(lambda: net.fp16_run_device(f16.data_ptr(), logits.data_ptr(), n, s))
        t8 = time(dec8)
        fired8 = int(counts.sum().item())
        t32 = time(dec32(logits))
        fired32 = int(counts.sum().item())
        worst = logits.clone()
        worst[..., 4::6] = 5.0
        t_worst = time(dec32(worst))
        fired_worst = int(counts.sum().item())
        none = logits.clone()
        none[..., 4::6] = -5.0
        t_none = time(dec32(none))
        print(f"decode fp16 network launch {t_net:8.2f} us")
        print(f"decode decode_ragged_kernel (int8 heads, {fired8} records) {t8:8.2f} us")
        print(f"decode decode_f32_kernel real content ({fired32} records) {t32:8.2f} us = {100 * t32 / t_net:.1f} % of the network launch")
        print(f"decode decode_f32_kernel worst case ({fired_worst} records) {t_worst:8.2f} us = {100 * t_worst / t_net:.1f} % of the network launch")
        print(f"decode decode_f32_kernel nothing fires (the confidence pass alone) {t_none:8.2f} us")
    if args.only in ("", "path"):
        t8, t16 = time(path8), time(path16)
        print(f"path   int8 images -> boxes {t8:8.2f} us = {n / t8:.2f} M images/s; fp16 images -> boxes {t16:8.2f} us = {n / t16:.2f} M images/s")
    net.destroy()


if __name__ == "__main__":
    main()
