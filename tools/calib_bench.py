#!/usr/bin/env python3
"""Frames per second of the calibration evaluation: yf_calib_observe_device (libyf_calib.so) at 4096 frames resident in HBM, beside the host
build of the same arithmetic (libyf_calib_host.so) on 1 and 16 threads and the float64 restatement (oracle/np_restatement.py, NpModel.run_float)
on one thread.

The device figure is the median of --launches timed calls (at least 20) after --warmup untimed ones, each call bracketed by HIP events on the
stream it runs on: evaluation and merge launch together, logits written.  The host figures are a wall clock around one call.  What is printed
is what was measured; if the kernel is not faster than the host build on 16 threads, the last line says so.

    python tools/calib_bench.py > profiles/calib_bench.txt

--size H W times the general launch instead (yf_calib_observe_hw_device: frames of H x W, the activations in global memory), in frames and
in output elements per second -- a frame of H x W is (H / 8) * (W / 8) / 49 times the work of a 56x56 one --, with the slab count and the
scratch it holds; at --size 56 56 the LDS kernel is timed beside it in the same run.  (The LDS kernel beside the parent commit's build:
tools/calib_histogram_bench.py --parent-lib.)

    python tools/calib_bench.py --size 160 160 --frames 1024

--simulate times one launch of the simulating form (yf_calib_simulate_device, or yf_calib_simulate_hw_device with --size: csrc/yf_calib_sim.h)
beside observe in the same run, on the same frames: every entry disabled, every entry enabled, and every entry enabled with reference logits
(records and totals written).  --parent-lib DIR/libyf_calib.so (built from the parent commit) has that build's observe timed in the same
process, in rounds that alternate with this build's: the existing kernels did not move.

    python tools/calib_bench.py --simulate [--size 160 160 --frames 1024] [--parent-lib DIR/libyf_calib.so]

--ab DIR/libyf_calib.so (built from the parent commit) times the observing, the comparing and the histogram form of both builds in one process,
LDS kernels at 56x56 and slab kernels at 56x56 (4096 frames) and at 160x160 (1024 frames): --rounds rounds (at least 5) per build, each the
median of --launches launches.  Every round has a handle of its own in either build, all created up front in alternation, and the build that
goes first alternates from round to round: where a handle's buffers lie and who follows whom moves a median by more than repeated launches on
one handle scatter, and both belong to the parent's own scatter.  Compare takes the tensors of calib.report_tensors (random int8 values), with
totals; histogram 2048 bins on the ranges observed.  A round median of this build passes inside the span of the parent's round medians, or
above it by no more than that span's width; the exit status is 1 if any fails.

    python tools/calib_bench.py --ab DIR/libyf_calib.so
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


def stage_elements(calib):
    """output elements of the 26 stages per 56x56 frame, from the graph's shapes: what one frame's evaluation computes"""
    model_file = importlib.import_module("stm32h7-yolo_amd.model_file")
    shapes = model_file.load_graph()["tensors"]
    produced = (51, 53, 55, 56, 58, 60, 62, 63, 65, 67, 69, 72, 74, 76, 78, 79, 81, 83, 85, 87, 89, 91, 94, 96, 98, 100)   # each stage's first tensor
    return sum(int(np.prod(shapes[t]["shape"][1:])) for t in produced)


def timed_observe(a, torch, cal, d_x, general):
    for _ in range(a.warmup):
        cal.observe(d_x, general=general)
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.launches):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        cal.observe(d_x, general=general)
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    return statistics.median(ms), min(ms), max(ms)


def general_rate(a, calib, torch, yfw):
    h, w = a.size
    x = np.random.default_rng(4096).integers(-128, 128, (a.frames, h, w, 3), dtype=np.int8)
    cal = calib.Calibration(yfw)
    d_x = torch.from_numpy(x).cuda()
    per_frame = stage_elements(calib) * (h // 8) * (w // 8) // 49
    print(f"device: {torch.cuda.get_device_name(0)}, libyf_calib.so build id {cal._lib.yf_calib_build_id().decode()}")
    med, lo, hi = timed_observe(a, torch, cal, d_x, True)
    print(f"yf_calib_observe_hw_device at {h}x{w}, {a.frames} frames from HBM, logits written, {a.launches} launches after {a.warmup} warm-up, HIP events:")
    print(f"  median {med:.3f} ms  (min {lo:.3f}, max {hi:.3f})  ->  {a.frames / med * 1e3:,.0f} frames/s, "
          f"{a.frames * per_frame / med * 1e3 / 1e9:.2f} G output elements/s ({per_frame} per frame)")
    print(f"  workgroups (= slabs): {cal.workgroups(h, w)}; scratch held: {cal.scratch_bytes} bytes")
    same = calib.host_run(yfw, x[:64], 16)[0] == _ranges_of(cal, d_x[:64])
    print(f"ranges of the first 64 frames, device against host build: {'bit-equal' if same else 'DIFFERENT'}")
    if (h, w) == (56, 56):
        med2, lo2, hi2 = timed_observe(a, torch, cal, d_x, False)
        print(f"yf_calib_observe_device (the LDS kernel), the same frames, the same run:")
        print(f"  median {med2:.3f} ms  (min {lo2:.3f}, max {hi2:.3f})  ->  {a.frames / med2 * 1e3:,.0f} frames/s, "
              f"{a.frames * per_frame / med2 * 1e3 / 1e9:.2f} G output elements/s")
        print(f"  general / LDS time: {med / med2:.2f}x")
    cal.destroy()
    return 0 if same else 1


def _ranges_of(cal, d_x):
    cal.reset()
    cal.observe(d_x, logits=False, general=True)
    return cal.ranges()


def simulate_rate(a, calib, torch, yfw):
    import ctypes
    h, w = a.size or (56, 56)
    hw = bool(a.size)
    n = a.frames
    d_x = torch.from_numpy(np.random.default_rng(4096).integers(-128, 128, (n, h, w, 3), dtype=np.int8)).cuda()
    d_l = torch.empty((n, h // 8, w // 8, 18), dtype=torch.float32, device="cuda")
    d_ref = torch.empty_like(d_l)
    d_s = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
    d_t = torch.zeros((48,), dtype=torch.uint8, device="cuda")
    cal = calib.Calibration(yfw)
    lib, hd, stream = cal._lib, cal.handle, torch.cuda.current_stream().cuda_stream
    yfm = open(os.path.join(ROOT, "oracle", "model", "yoloface_int8.yfm"), "rb").read()
    none, full = calib.empty_table(), calib.simulation_table(yfm)
    size = (h, w) if hw else ()

    def observe_of(library, handle):
        fn = library.yf_calib_observe_hw_device if hw else library.yf_calib_observe_device
        def call():
            if fn(handle, *size, d_x.data_ptr(), n, d_l.data_ptr(), stream) != n:
                sys.exit("calib_bench: observe failed")
        return call

    def simulate_of(table, ref):
        fn = lib.yf_calib_simulate_hw_device if hw else lib.yf_calib_simulate_device
        def call():
            rc = fn(hd, *size, d_x.data_ptr(), n, table.ctypes.data, d_ref.data_ptr() if ref else None, d_l.data_ptr(), d_s.data_ptr() if ref else None,
                    d_t.data_ptr() if ref else None, stream)
            if rc != n:
                sys.exit(f"calib_bench: simulate failed: {cal._text()}")
        return call

    def timed(call):
        for _ in range(a.warmup):
            call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.launches):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            call()
            t1.record()
            t1.synchronize()
            ms.append(t0.elapsed_time(t1))
        return statistics.median(ms), min(ms), max(ms)

    name = f"yf_calib_simulate{'_hw' if hw else ''}_device"
    print(f"device: {torch.cuda.get_device_name(0)}, libyf_calib.so build id {lib.yf_calib_build_id().decode()}")
    print(f"One launch at {h}x{w} ({'the general kernels' if hw else 'the LDS kernels'}) over {n} random frames resident in HBM, {a.launches} launches after "
          f"{a.warmup} warm-up, HIP events, median (min, max) in ms")
    builds = [("this build", observe_of(lib, hd))]
    parent = None
    if a.parent_lib:
        parent = ctypes.CDLL(a.parent_lib)
        vp, ci = ctypes.c_void_p, ctypes.c_int
        parent.yf_calib_create.restype, parent.yf_calib_create.argtypes = vp, [ctypes.c_char_p, ctypes.c_size_t, ci]
        parent.yf_calib_observe_device.restype, parent.yf_calib_observe_device.argtypes = ctypes.c_long, [vp, vp, ctypes.c_long, vp, vp]
        parent.yf_calib_observe_hw_device.restype, parent.yf_calib_observe_hw_device.argtypes = ctypes.c_long, [vp, ci, ci, vp, ctypes.c_long, vp, vp]
        parent.yf_calib_destroy.restype, parent.yf_calib_destroy.argtypes = None, [vp]
        parent.yf_calib_build_id.restype = ctypes.c_char_p
        ph = parent.yf_calib_create(yfw, len(yfw), 0)
        if not ph:
            sys.exit("calib_bench: yf_calib_create of the parent library failed")
        builds.append(("parent commit", observe_of(parent, ph)))
        print(f"  libyf_calib.so of the parent commit: build id {parent.yf_calib_build_id().decode()}, loaded beside this build's; rounds alternate")
    results = {k: [] for k, _ in builds}
    for _ in range(3 if parent else 1):
        for k, call in builds:
            results[k].append(timed(call))
    for k, _ in builds:
        for r, (med, lo, hi) in enumerate(results[k]):
            print(f"  observe (evaluation + merge, logits written), {k:13s} round {r + 1}   {med:.3f}  ({lo:.3f}, {hi:.3f})")
    obs = statistics.median(m for m, _, _ in results["this build"])
    builds[0][1]()
    torch.cuda.synchronize()
    d_ref.copy_(d_l)
    for label, table, ref in (("every entry disabled, logits written", none, False), ("every entry enabled, logits written", full, False),
                              ("every entry enabled, logits, records and totals", full, True)):
        med, lo, hi = timed(simulate_of(table, ref))
        print(f"  {name}, {label:48s} {med:.3f}  ({lo:.3f}, {hi:.3f})   {med / obs:.2f}x observe")
    if parent:
        parent.yf_calib_destroy(ph)
    cal.destroy()
    return 0


AB_SHAPES = (("LDS", 56, 56, 4096, False), ("slab", 56, 56, 4096, True), ("slab", 160, 160, 1024, True))


def ab_rate(a, calib, torch, yfw):
    import ctypes
    yf = importlib.import_module("stm32h7-yolo_amd")
    yfm = open(os.path.join(ROOT, "oracle", "model", "yoloface_int8.yfm"), "rb").read()
    network = yf.load()
    tensors = calib.report_tensors(lambda op: network.yf_network_dump_offset(int(op)), yfm)
    cal = calib.Calibration(yfw)
    parent = ctypes.CDLL(a.ab)
    vp = ctypes.c_void_p
    parent.yf_calib_create.restype, parent.yf_calib_create.argtypes = vp, [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int]
    parent.yf_calib_destroy.restype, parent.yf_calib_destroy.argtypes = None, [vp]
    parent.yf_calib_build_id.restype = parent.yf_calib_last_error_text.restype = ctypes.c_char_p
    calib.declare_device(parent)
    builds = (("this build", cal._lib, []), ("parent commit", parent, []))
    for _ in range(a.rounds):                                              # a handle per round and build, created in alternation
        for k, lib, handles in builds:
            handles.append(lib.yf_calib_create(yfw, len(yfw), cal.device))
            if not handles[-1]:
                sys.exit(f"calib_bench: yf_calib_create failed ({k}): {lib.yf_calib_last_error_text().decode()}")
    stream, bins, rng = torch.cuda.current_stream().cuda_stream, 2048, np.random.default_rng(4096)
    print(f"device: {torch.cuda.get_device_name(0)}")
    for k, lib, _ in builds:
        print(f"libyf_calib.so, {k}: build id {lib.yf_calib_build_id().decode()}")
    print(f"Both libraries in one process.  Per entry and shape {a.rounds} rounds per build, each round on a handle of its own, the build that goes first "
          f"alternating; a round is the median of {a.launches} launches after {a.warmup} warm-up, each launch between two HIP events on its stream, "
          f"frames resident in HBM.")
    print(f"observe: evaluation + merge, logits written.  compare: the {len(tensors)} tensors of calib.report_tensors, random int8 values, with totals.  "
          f"histogram: {bins} bins on the ranges observed.")
    print("pass: every round of this build inside the span of the parent's rounds, or above it by no more than the span's width")

    def timed(call):
        for _ in range(a.warmup):
            call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.launches):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            call()
            t1.record()
            t1.synchronize()
            ms.append(t0.elapsed_time(t1))
        return statistics.median(ms)

    failed = 0
    for kernels, h, w, n, hw in AB_SHAPES:
        d_x = torch.from_numpy(rng.integers(-128, 128, (n, h, w, 3), dtype=np.int8)).cuda()
        d_l = torch.empty((n, h // 8, w // 8, 18), dtype=torch.float32, device="cuda")
        elements = [calib.elements_at(t["elements"], h, w) for t in tensors]
        offsets = np.concatenate([[0], np.cumsum(elements)])
        d_q = torch.from_numpy(rng.integers(-128, 128, (n, int(offsets[-1])), dtype=np.int8)).cuda()
        entries = calib._qtensors([calib.Entry(t["tensor"], t["scale"], t["zero_point"], d_q.data_ptr() + int(o), int(offsets[-1]))
                                   for t, o in zip(tensors, offsets)])
        d_stats = torch.zeros((n, len(tensors), 32), dtype=torch.uint8, device="cuda")
        d_totals = torch.zeros((len(tensors), 48), dtype=torch.uint8, device="cuda")
        d_counts = torch.zeros((calib.N_RANGES, bins), dtype=torch.int64, device="cuda")
        cal.reset()
        cal.observe(d_x, logits=False, general=hw)
        minmax = calib._minmax_array(cal.ranges())
        size, sfx = ((h, w), "_hw") if hw else ((), "")
        args = {"observe": (d_x.data_ptr(), n, d_l.data_ptr(), stream),
                "compare": (d_x.data_ptr(), n, entries, len(tensors), d_stats.data_ptr(), d_totals.data_ptr(), stream),
                "histogram": (d_x.data_ptr(), n, minmax.ctypes.data, bins, d_counts.data_ptr(), stream)}
        print(f"\n{kernels} kernels, {h}x{w}, {n} frames: round medians in ms")
        for op, tail in args.items():
            name = f"yf_calib_{op}{sfx}_device"

            def call_of(lib, handle):
                fn = getattr(lib, name)
                def call():
                    if fn(handle, *size, *tail) != n:
                        sys.exit(f"calib_bench: {name} failed: {lib.yf_calib_last_error_text().decode()}")
                return call

            rounds = {k: [] for k, _, _ in builds}
            for r in range(a.rounds):
                for k, lib, handles in builds[::-1 if r % 2 else 1]:
                    rounds[k].append(timed(call_of(lib, handles[r])))
            lo, hi = min(rounds["parent commit"]), max(rounds["parent commit"])
            ok = max(rounds["this build"]) <= hi + (hi - lo)
            failed += not ok
            for k, _, _ in builds:
                print(f"  {name:32s} {k:13s} " + " ".join(f"{m:7.3f}" for m in rounds[k]) + f"   median {statistics.median(rounds[k]):.3f}")
            print(f"  {'':32s} parent span {lo:.3f} .. {hi:.3f} (width {hi - lo:.3f}), this build {min(rounds['this build']):.3f} .. "
                  f"{max(rounds['this build']):.3f}: {'pass' if ok else 'FAIL'}")
        torch.cuda.synchronize()
    for _, lib, handles in builds:
        for handle in handles:
            lib.yf_calib_destroy(handle)
    cal.destroy()
    print(f"\n{'every entry passes' if not failed else f'{failed} entries FAIL'}")
    return 1 if failed else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=2, metavar=("H", "W"))
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-frames", type=int, default=512)
    ap.add_argument("--restatement-frames", type=int, default=8)
    ap.add_argument("--simulate", action="store_true", help="time the simulating form beside observe")
    ap.add_argument("--parent-lib", help="with --simulate: libyf_calib.so built from the parent commit, whose observe is timed beside this build's")
    ap.add_argument("--ab", metavar="PARENT_LIB", help="libyf_calib.so built from the parent commit: observe, compare and histogram of both builds")
    ap.add_argument("--rounds", type=int, default=5, help="with --ab: rounds per build")
    a = ap.parse_args()
    if a.launches < 20:
        ap.error("--launches: at least 20")
    if a.rounds < 5:
        ap.error("--rounds: at least 5")
    import torch
    calib = importlib.import_module("stm32h7-yolo_amd.calib")
    model_file = importlib.import_module("stm32h7-yolo_amd.model_file")
    yfw = open(os.path.join(ROOT, "stm32h7-yolo_amd", "model", "yoloface_fp32.yfw"), "rb").read()
    if a.ab:
        if not torch.cuda.is_available():
            sys.exit("calib_bench: --ab needs a GPU")
        return ab_rate(a, calib, torch, yfw)
    if a.simulate:
        if not torch.cuda.is_available():
            sys.exit("calib_bench: --simulate needs a GPU")
        return simulate_rate(a, calib, torch, yfw)
    if a.size:
        if not torch.cuda.is_available():
            sys.exit("calib_bench: --size needs a GPU")
        return general_rate(a, calib, torch, yfw)
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
