#!/usr/bin/env python3
"""What clipped calibration ranges do to this network, and what the histogram pass costs: the record profiles/calib_histogram.txt holds.

    python tools/calib_histogram_bench.py [--parent-lib DIR/libyf_calib.so] > profiles/calib_histogram.txt

(a) calib.quantisation_report of stm32h7-yolo_amd/model/yoloface_fp32.yfw quantised on the device with ranges minmax, percentile 0.9999,
    percentile 0.999, mse, and percentile 0.999 with the head kept (keep=(0, 100)), over the frames of tests/golden/calib_frames_56_cv.bin; below each table the lowest sqnr_db, the head row
    (tensor 100) and the number of head bytes that differ from the min/max model's heads.
(b) one launch of yf_calib_histogram_device over --bench-frames random frames at 2048 and 16 bins beside one launch of
    yf_calib_observe_device: the median of --launches calls after --warmup, each bracketed by HIP events on its stream.  With --parent-lib
    (libyf_calib.so built from the parent commit) its observe is timed in the same process, in rounds that alternate with this build's.
    --variant-lib LABEL=PATH (repeatable) times the histogram launch of another build of this commit's library beside this one's, e.g. one
    compiled with -DYFC_HIST_PEEL=0 (no pre-count of shared bins: every lane adds for itself).
"""
import argparse
import ctypes
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.quant_report import print_table, timed      # noqa: E402

# (method, percentile, keep); the last one is the remedy where clipping costs the head: the head's own range stays min/max
SETTINGS = (("minmax", None, (0,)), ("percentile", 0.9999, (0,)), ("percentile", 0.999, (0,)), ("mse", None, (0,)), ("percentile", 0.999, (0, 100)))


def tables(torch, yf, calib, x, bins):
    yfw = open(os.path.join(ROOT, "stm32h7-yolo_amd", "model", "yoloface_fp32.yfw"), "rb").read()
    d_x = torch.from_numpy(x).cuda()
    d_out = torch.zeros((x.shape[0], calib.LOGITS), dtype=torch.int8, device="cuda")
    net = yf.Network(device=0)
    base, summary = None, []
    for k, (method, p, keep) in enumerate(SETTINGS):
        name = (method if p is None else f"{method} {p}") + ("" if keep == (0,) else f", keep={keep}")
        yfm = calib.quantize_on_device(yfw, d_x, ranges=method, percentile=p or 0.9999, bins=bins, keep=keep)
        net.init_model(yfm)
        rows = calib.quantisation_report(net, yfw, yfm, x)
        net.run_device(d_x.data_ptr(), d_out.data_ptr(), x.shape[0], torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        heads = d_out.cpu().numpy()
        base = heads if base is None else base
        print(f"\n(a{k + 1}) ranges = {name}" + ("" if method == "minmax" else f", {bins} bins"))
        print_table(rows)
        head, worst = rows[-1], min(rows, key=lambda r: r["sqnr_db"])
        differ = int((heads != base).sum())
        print(f"  head (tensor {head['tensor']}): scale {head['scale']:.8f}, rmse/scale {head['rmse_over_scale']:.3f}, max/scale "
              f"{head['max_abs_error'] / head['scale']:.3f}, sqnr_db {head['sqnr_db']:.2f}, saturated {100.0 * head['saturated']:.4f} %; "
              f"head bytes that differ from the min/max model's: {differ} of {heads.size}")
        summary.append((name, worst["tensor"], worst["sqnr_db"], float(np.mean([r["sqnr_db"] for r in rows])), head["sqnr_db"],
                        head["rmse_over_scale"] * head["scale"], differ))
    net.destroy()
    print("\n(a) in one table: sqnr_db is of the int8 tensor against the float32 tensor, head rmse in the logits' own unit")
    print("  ranges                              lowest sqnr_db (tensor)   mean sqnr_db   head sqnr_db   head rmse    head bytes changed")
    for name, t, lowest, mean, head, rmse, differ in summary:
        print(f"  {name:34s}  {lowest:6.2f} ({t:3d})              {mean:6.2f}         {head:6.2f}         {rmse:.5f}      {differ}")
    return summary


def raw_observe(lib, yfw, device=0):
    """a handle of another build of libyf_calib.so (loaded beside this one) and a call that launches its observe"""
    vp = ctypes.c_void_p
    lib.yf_calib_create.restype, lib.yf_calib_create.argtypes = vp, [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int]
    lib.yf_calib_observe_device.restype, lib.yf_calib_observe_device.argtypes = ctypes.c_long, [vp, vp, ctypes.c_long, vp, vp]
    lib.yf_calib_destroy.restype, lib.yf_calib_destroy.argtypes = None, [vp]
    lib.yf_calib_build_id.restype = ctypes.c_char_p
    h = lib.yf_calib_create(yfw, len(yfw), device)
    if not h:
        sys.exit("calib_histogram_bench: yf_calib_create of the parent library failed")
    return h


def bench(a, torch, calib):
    yfw = open(os.path.join(ROOT, "stm32h7-yolo_amd", "model", "yoloface_fp32.yfw"), "rb").read()
    n = a.bench_frames
    d_x = torch.from_numpy(np.random.default_rng(4096).integers(-128, 128, (n, 56, 56, 3), dtype=np.int8)).cuda()
    d_logits = torch.empty((n, 7, 7, 18), dtype=torch.float32, device="cuda")
    cal = calib.Calibration(yfw)
    cal.observe(d_x)
    ranges = cal.ranges()
    lib, h, stream = cal._lib, cal.handle, torch.cuda.current_stream().cuda_stream
    minmax = calib._minmax_array(ranges)

    def observe_of(library, handle):
        def call():
            if library.yf_calib_observe_device(handle, d_x.data_ptr(), n, d_logits.data_ptr(), stream) != n:
                sys.exit("calib_histogram_bench: yf_calib_observe_device failed")
        return call

    print(f"\n(b) One launch over {n} random frames resident in HBM, {a.launches} launches after {a.warmup} warm-up, HIP events, median (min, max) in ms")
    builds = [("this build", observe_of(lib, h))]
    parent = None
    if a.parent_lib:
        parent = ctypes.CDLL(a.parent_lib)
        parent_handle = raw_observe(parent, yfw)
        builds.append(("parent commit", observe_of(parent, parent_handle)))
        print(f"    libyf_calib.so of the parent commit: build id {parent.yf_calib_build_id().decode()}, loaded beside this build's; rounds alternate")
    results = {name: [] for name, _ in builds}
    for r in range(a.rounds if parent else 1):
        for name, call in builds:
            results[name].append(timed(torch, call, a.launches, a.warmup))
    for name, _ in builds:
        for r, (med, lo, hi) in enumerate(results[name]):
            print(f"    yf_calib_observe_device (evaluation + merge, logits written), {name:13s} round {r + 1}   {med:.3f}  ({lo:.3f}, {hi:.3f})   spread {hi - lo:.3f}")
    if parent:
        p, c = results["parent commit"], results["this build"]
        spread = max(hi - lo for _, lo, hi in p)
        moved = max(abs(cm - pm) for (cm, _, _), (pm, _, _) in zip(c, p))
        print(f"    the parent's largest min-max spread over its own {a.launches} launches: {spread:.3f} ms; the largest difference of this build's median from "
              f"the parent's in the same round: {moved:.3f} ms -- {'within' if moved <= 2 * spread else 'BEYOND'} twice that spread")
    variants = [("this build", lib, h)]
    for spec in a.variant_lib:
        label, _, path = spec.rpartition("=")              # (a label may hold "=" itself)
        other = ctypes.CDLL(path)
        other.yf_calib_histogram_device.restype = ctypes.c_long
        other.yf_calib_histogram_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        variants.append((label, other, raw_observe(other, yfw)))
    for bins in (2048, 16):
        reference = None
        for label, library, handle in variants:
            d_counts = torch.zeros((calib.N_RANGES, bins), dtype=torch.int64, device="cuda").view(torch.uint64)

            def call():
                if library.yf_calib_histogram_device(handle, d_x.data_ptr(), n, minmax.ctypes.data, bins, d_counts.data_ptr(), stream) != n:
                    sys.exit(f"calib_histogram_bench: yf_calib_histogram_device of {label} failed: {cal._text()}")
            med, lo, hi = timed(torch, call, a.launches, a.warmup)
            counts = d_counts.cpu().numpy()
            assert int(counts[0].sum(dtype=np.uint64)) == 9408 * n * (a.launches + a.warmup)      # every launch added every input value once
            reference = counts if reference is None else reference
            assert np.array_equal(counts, reference), label                                       # every build counts the same
            print(f"    yf_calib_histogram_device, {bins:4d} bins, axes of these frames' own ranges, {label:32s} {med:.3f}  ({lo:.3f}, {hi:.3f})")
    cal.destroy()
    for _, library, handle in variants[1:]:
        library.yf_calib_destroy(handle)
    if parent:
        parent.yf_calib_destroy(parent_handle)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default=os.path.join(ROOT, "tests", "golden", "calib_frames_56_cv.bin"))
    ap.add_argument("--bins", type=int, default=2048)
    ap.add_argument("--bench-frames", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", help="libyf_calib.so built from the parent commit: its observe is timed beside this build's")
    ap.add_argument("--variant-lib", action="append", default=[], metavar="LABEL=PATH",
                    help="another build of libyf_calib.so whose histogram launch is timed beside this build's")
    ap.add_argument("--skip-tables", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("calib_histogram_bench: needs a GPU")
    yf = importlib.import_module("stm32h7-yolo_amd")
    calib = importlib.import_module("stm32h7-yolo_amd.calib")
    x = np.fromfile(a.frames, np.int8)
    if x.size == 0 or x.size % calib.FRAME_BYTES:
        sys.exit(f"calib_histogram_bench: {a.frames} holds {x.size} bytes, expected a multiple of {calib.FRAME_BYTES}")
    x = x.reshape(-1, 56, 56, 3)
    print("Histogram calibration: clipped ranges against min/max on the shipped float model, and the cost of the histogram pass, as")
    print(f"tools/calib_histogram_bench.py printed it on: {torch.cuda.get_device_name(0)}, libyf_calib.so build id {calib.load().yf_calib_build_id().decode()}")
    print(f"Frames of part (a): the {x.shape[0]} of {os.path.relpath(a.frames, ROOT)}; they calibrate the model AND measure it.  error = dequantised int8 - float32.")
    if not a.skip_tables:
        tables(torch, yf, calib, x, a.bins)
    bench(a, torch, calib)
    return 0


if __name__ == "__main__":
    sys.exit(main())
