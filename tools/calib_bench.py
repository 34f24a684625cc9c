#!/usr/bin/env python3
"""Frames per second of the calibration evaluation: yf_calib_observe_device (libyf_calib.so) at 4096 frames resident in HBM, beside the host
build of the same arithmetic (libyf_calib_host.so) on 1 and 16 threads and the float64 restatement (oracle/np_restatement.py, NpModel.run_float)
on one thread.

The device figure is the median of --launches timed calls (at least 20) after --warmup untimed ones, each call bracketed by HIP events on the
stream it runs on: evaluation and merge launch together, logits written.  The host figures are a wall clock around one call.  What is printed
is what was measured; if the kernel is not faster than the host build on 16 threads, the last line says so.

    python tools/calib_bench.py > profiles/calib_bench.txt
"""
import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def device_rate(a, calib, torch, yfw, x):
    cal = calib.Calibration(yfw)
    d_x = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    for _ in range(a.warmup):
        cal.observe(d_x)
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.launches):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        cal.observe(d_x)
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    dev_ranges = cal.ranges()
    dev_fps = a.frames / (statistics.median(ms) / 1e3)
    print(f"device: {torch.cuda.get_device_name(0)}, libyf_calib.so build id {cal._lib.yf_calib_build_id().decode()}")
    print(f"yf_calib_observe_device, {a.frames} frames from HBM, logits written, {a.launches} launches after {a.warmup} warm-up, HIP events:")
    print(f"  median {statistics.median(ms):.3f} ms  (min {min(ms):.3f}, max {max(ms):.3f})  ->  {dev_fps:,.0f} frames/s")
    cal.destroy()
    return dev_fps, dev_ranges


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-frames", type=int, default=512)
    ap.add_argument("--restatement-frames", type=int, default=8)
    a = ap.parse_args()
    if a.launches < 20:
        ap.error("--launches: at least 20")
    import torch
    calib = importlib.import_module("stm32h7-yolo_amd.calib")
    model_file = importlib.import_module("stm32h7-yolo_amd.model_file")
    yfw = open(os.path.join(ROOT, "stm32h7-yolo_amd", "model", "yoloface_fp32.yfw"), "rb").read()
    x = np.random.default_rng(4096).integers(-128, 128, (a.frames, 56, 56, 3), dtype=np.int8)

    dev_fps = dev_ranges = None
    if torch.cuda.is_available():
        dev_fps, dev_ranges = device_rate(a, calib, torch, yfw, x)
    else:
        print("no GPU in this run: the rate of yf_calib_observe_device was NOT measured; the host figures follow")

    hx = x[:a.host_frames]
    host_fps = {}
    for threads in (1, 16):
        calib.host_run(yfw, hx[:threads], threads)                         # (loads the library, starts the threads once)
        t = time.perf_counter()
        r, _ = calib.host_run(yfw, hx, threads)
        host_fps[threads] = a.host_frames / (time.perf_counter() - t)
        print(f"host build (libyf_calib_host.so), {a.host_frames} frames, {threads:2d} thread(s), wall clock: {host_fps[threads]:,.0f} frames/s")
    same = dev_ranges is None or calib.host_run(yfw, x, 16)[0] == dev_ranges
    if dev_ranges is not None:
        print(f"ranges of the {a.frames} frames, device against host build: {'bit-equal' if same else 'DIFFERENT'}")

    from oracle.np_restatement import NpModel
    npm = NpModel(os.path.join(ROOT, "oracle", "model", "yoloface_int8.yfm"))
    convs = [(w, b) for w, b, _ in model_file.read_yfw(yfw)]
    t = time.perf_counter()
    for f in x[:a.restatement_frames]:
        npm.run_float(f, float_convs=convs)
    print(f"float64 restatement (NpModel.run_float), {a.restatement_frames} frames, one thread, wall clock: "
          f"{a.restatement_frames / (time.perf_counter() - t):,.0f} frames/s")
    if dev_fps is None:
        return 0
    ratio = dev_fps / host_fps[16]
    print(f"kernel / host build on 16 threads: {ratio:.1f}x" + ("" if ratio > 1 else "  -- the kernel is NOT faster than the host build on 16 threads"))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
