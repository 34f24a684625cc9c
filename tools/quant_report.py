#!/usr/bin/env python3
"""Where an int8 model loses precision: the per-tensor table of calib.quantisation_report for a float model (.yfw) and the int8 model (.yfm)
quantised from it, over a file of frames (int8 [n][56][56][3]).  error = dequantised int8 value - float32 value of the same element.

    python tools/quant_report.py --yfw model.yfw --yfm model.yfm --frames frames.bin

Without --yfw / --yfm it writes the record profiles/quant_report.txt holds: the shipped .yfm against the float weights it was quantised from
(tests/golden/ptq_float_convs.npz), quantize_on_device of the shipped .yfw against that .yfw, both over tests/golden/calib_frames_56_cv.bin,
and the time of a compare launch (all 28 tensors, totals included) beside an observe launch on the same --bench-frames random frames: the
median of --launches calls after --warmup, each bracketed by HIP events on its stream.

    python tools/quant_report.py > profiles/quant_report.txt

--size S reads the frames as int8 [n][S][S][3] (160: the engine's other size) and needs --yfw / --yfm.  At a size other than 56 the table has
the head's row alone (tensor 100, from yf_network_run_device_hw): the engine's per-stage dump exists at 56x56 only.

--sensitivity writes the record profiles/quant_sensitivity.txt holds instead: what each tensor's quantisation alone costs the logits
(calib.sensitivity: the float evaluation with that tensor on its int8 grid, csrc/yf_calib_sim.h) for the shipped pair, for the model
quantised on the device at 56x56 and for one calibrated at 160x160; the wall time of a whole table on --bench-frames frames; how close the
full simulation is to the engine's own head; and what ranges="head" does to section 2 of profiles/quant_report.txt.

    python tools/quant_report.py --sensitivity > profiles/quant_sensitivity.txt

--ranges {minmax,percentile,mse,head}, --percentile and --bins choose the calibration ranges of the model it quantises on the device (section 2;
calib.quantize_on_device: clipped ranges from histograms, ptq.clip_ranges); the default is min/max, the record's.
"""
import argparse
import importlib
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def print_table(rows):
    print("  tensor  op  elements   scale       zp    mean_error    max_abs_error  mean_squared_error  rmse/scale  max/scale  sqnr_db  saturated")
    for r in rows:
        print(f"  {r['tensor']:6d}  {r['op']:2d}  {r['elements']:8d}  {r['scale']:.8f}  {r['zero_point']:4d}  {r['mean_error']:+.6e}  {r['max_abs_error']:.6e}   "
              f"{r['mean_squared_error']:.6e}        {r['rmse_over_scale']:7.3f}    {r['max_abs_error'] / r['scale']:7.3f}   {r['sqnr_db']:6.2f}  "
              f"{100.0 * r['saturated']:.4f} %")
    worst = min(rows, key=lambda r: r["sqnr_db"])
    print(f"  lowest sqnr_db: tensor {worst['tensor']} (op {worst['op']}), {worst['sqnr_db']:.2f} dB; "
          f"largest max/scale: tensor {max(rows, key=lambda r: r['max_abs_error'] / r['scale'])['tensor']}")


def timed(torch, fn, launches, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(launches):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    return statistics.median(ms), min(ms), max(ms)


def bench(a, torch, calib, net, yfw, yfm):
    """one compare launch against one observe launch, the same frames resident in HBM, the int8 tensors from the engine's dump of them"""
    x = np.random.default_rng(4096).integers(-128, 128, (a.bench_frames, 56, 56, 3), dtype=np.int8)
    d_x = torch.from_numpy(x).cuda()
    n, dump_bytes = a.bench_frames, net.dump_bytes()
    d_out = torch.zeros((n, calib.LOGITS), dtype=torch.int8, device="cuda")
    d_dump = torch.zeros((n, dump_bytes), dtype=torch.int8, device="cuda")
    net.run_device(d_x.data_ptr(), d_out.data_ptr(), n, torch.cuda.current_stream().cuda_stream, d_dump.data_ptr())
    tensors = calib.report_tensors(net.dump_offset, yfm)
    entries = calib._qtensors([calib.Entry(t["tensor"], t["scale"], t["zero_point"], d_out.data_ptr() if t["offset"] is None else d_dump.data_ptr() + t["offset"],
                                           calib.LOGITS if t["offset"] is None else dump_bytes) for t in tensors])
    d_stats = torch.zeros((n, len(tensors), 32), dtype=torch.uint8, device="cuda")
    d_totals = torch.zeros((len(tensors), 48), dtype=torch.uint8, device="cuda")
    d_stats1 = torch.zeros((n, 1, 32), dtype=torch.uint8, device="cuda")
    cal = calib.Calibration(yfw)
    stream = torch.cuda.current_stream().cuda_stream
    lib, h = cal._lib, cal.handle
    per_frame = sum(t["elements"] for t in tensors)
    rc = lib.yf_calib_compare_device(h, d_x.data_ptr(), n, entries, len(tensors), d_stats.data_ptr(), d_totals.data_ptr(), stream)
    if rc != n:
        sys.exit(f"quant_report: yf_calib_compare_device: {cal._text()}")
    obs = timed(torch, lambda: cal.observe(d_x), a.launches, a.warmup)
    cmp_all = timed(torch, lambda: lib.yf_calib_compare_device(h, d_x.data_ptr(), n, entries, len(tensors), d_stats.data_ptr(), d_totals.data_ptr(), stream),
                    a.launches, a.warmup)
    cmp_no_totals = timed(torch, lambda: lib.yf_calib_compare_device(h, d_x.data_ptr(), n, entries, len(tensors), d_stats.data_ptr(), None, stream),
                          a.launches, a.warmup)
    cmp_one = timed(torch, lambda: lib.yf_calib_compare_device(h, d_x.data_ptr(), n, ctypes_last(entries, len(tensors)), 1, d_stats1.data_ptr(), None, stream),
                    a.launches, a.warmup)
    cal.destroy()
    print(f"\n3. One launch over {n} random frames resident in HBM, {a.launches} launches after {a.warmup} warm-up, HIP events, median (min, max) in ms")
    print(f"   yf_calib_observe_device (evaluation + merge, logits written)                      {obs[0]:.3f}  ({obs[1]:.3f}, {obs[2]:.3f})")
    print(f"   yf_calib_compare_device, {len(tensors)} tensors, {per_frame} int8 bytes read per frame, with totals   {cmp_all[0]:.3f}  ({cmp_all[1]:.3f}, {cmp_all[2]:.3f})")
    print(f"   the same without the totals launch                                                {cmp_no_totals[0]:.3f}  ({cmp_no_totals[1]:.3f}, {cmp_no_totals[2]:.3f})")
    print(f"   yf_calib_compare_device, the head alone, no totals                                {cmp_one[0]:.3f}  ({cmp_one[1]:.3f}, {cmp_one[2]:.3f})")
    print(f"   compare (28 tensors, totals) / observe: {cmp_all[0] / obs[0]:.2f}x")


def ctypes_last(entries, count):
    one = (type(entries[0]) * 1)()
    one[0] = entries[count - 1]
    return one


def sensitivity_record(a, torch, calib, model_file, net, x, npz_yfw, shipped_yfw, shipped_yfm):
    """the record of profiles/quant_sensitivity.txt"""
    import time
    ptq = importlib.import_module("stm32h7-yolo_amd.ptq")
    d_x = torch.from_numpy(x).cuda()
    print("What each tensor's quantisation costs the logits: the float32 evaluation with the named tensor (or the named convolution's weights and")
    print("bias) on the int8 model's grid and everything else float, against the all-float logits (calib.sensitivity; csrc/yf_calib_sim.h), as")
    print(f"tools/quant_report.py --sensitivity printed it on: {torch.cuda.get_device_name(0)}, libyf_calib.so build id "
          f"{calib.load().yf_calib_build_id().decode()}, libyf_network.so build id {net.build_id}")
    print(f"Frames: the {x.shape[0]} of {os.path.relpath(a.frames, ROOT)}.  rmse and max in LSB of the model's head; clipped: the share of the quantised values")
    print("that fell outside -128..127.  This is float arithmetic on the int8 grid, not the engine's fixed-point requantisation.")

    def table(title, yfw, yfm, frames):
        rows = calib.sensitivity(yfw, yfm, frames)
        print("\n" + title)
        print(calib.format_sensitivity(rows))
        single = rows[:50]
        worst = min(single, key=lambda r: r["sqnr_db"])
        print(f"  the most damaging single tensor: {worst['name']} ({worst['op']}), {worst['sqnr_db']:.2f} dB; tensor 67 alone: "
              f"{single[calib.sim_tensors().index(67)]['sqnr_db']:.2f} dB")
        return rows

    table("1a. oracle/model/yoloface_int8.yfm (the shipped model) on tests/golden/ptq_float_convs.npz (the float weights it came from), 56x56", npz_yfw,
          shipped_yfm, d_x)
    new_yfm = calib.quantize_on_device(shipped_yfw, d_x)
    table("1b. calib.quantize_on_device(stm32h7-yolo_amd/model/yoloface_fp32.yfw, the same frames) on that .yfw, 56x56", shipped_yfw, new_yfm, d_x)
    real = np.fromfile(os.path.join(ROOT, "tests", "golden", "real_frames_56.bin"), np.int8).reshape(-1, 56, 56, 3)
    u = (real.astype(np.int16) + 128).astype(np.uint8)
    x160 = np.stack([ptq.resize_linear_u8(f, 160, 160) for f in u]).reshape(-1, 160, 160, 3)
    d_160 = torch.from_numpy(np.ascontiguousarray((x160.astype(np.int16) - 128).astype(np.int8))).cuda()
    yfm160 = calib.quantize_on_device(shipped_yfw, d_160)
    table(f"1c. the same .yfw calibrated and simulated at 160x160: the {d_160.shape[0]} frames of tests/golden/real_frames_56.bin resized as OpenCV does",
          shipped_yfw, yfm160, d_160)

    big = torch.from_numpy(np.random.default_rng(4096).integers(-128, 128, (a.bench_frames, 56, 56, 3), dtype=np.int8)).cuda()
    calib.sensitivity(npz_yfw, shipped_yfm, d_x)
    torch.cuda.synchronize()
    t = time.perf_counter()
    rows = calib.sensitivity(npz_yfw, shipped_yfm, big)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t
    handles = 2 + sum(1 for r in rows if r["op"] == "WEIGHTS")        # the float weights, every convolution's own, all dequantised
    print("\n2. Time of one simulate launch: tools/calib_bench.py --simulate prints it (beside observe, and beside the parent commit's observe)")
    print(f"\n3. Wall time of one calib.sensitivity call at 56x56 on {a.bench_frames} random frames resident in HBM ({len(rows)} rows: {len(rows) + 1} evaluations, "
          f"{handles} handles created): {wall:.3f} s")

    # 4. the full simulation against the engine's own head on the same frames
    cal = calib.Calibration(ptq.dequantized_yfw(npz_yfw, shipped_yfm))
    ref_cal = calib.Calibration(npz_yfw)
    ref = ref_cal.simulate(d_x, calib.empty_table())[0]
    sim = cal.simulate(d_x, calib.simulation_table(shipped_yfm), ref)[0].cpu().numpy().reshape(x.shape[0], -1)
    cal.destroy(); ref_cal.destroy()
    T = model_file.load_yfm(shipped_yfm)["tensors"][100]
    scale, zp = float(T["scale"][0]), int(T["zp"])
    net.init_model(shipped_yfm)
    d_out = torch.zeros((x.shape[0], calib.LOGITS), dtype=torch.int8, device="cuda")
    net.run_device(d_x.data_ptr(), d_out.data_ptr(), x.shape[0], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    heads = d_out.cpu().numpy().astype(np.int64)
    sim_q = np.rint(sim.astype(np.float64) / scale).astype(np.int64) + zp
    d = sim_q - heads
    flt = ref.cpu().numpy().reshape(x.shape[0], -1).astype(np.float64)
    rms = lambda e: float(np.sqrt(np.mean(e * e)))
    print(f"\n4. The `all` simulation of 1a against the int8 engine's head on the same {x.shape[0]} frames (head scale {scale:.8f}, zero point {zp}):")
    print(f"   simulation - engine: rms {rms(d.astype(np.float64)):.3f} LSB; equal bytes {100.0 * np.mean(d == 0):.1f} %; within one LSB {100.0 * np.mean(np.abs(d) <= 1):.1f} %")
    print(f"   against the float logits: simulation rms {rms(sim - flt) / scale:.3f} LSB, engine rms {rms((heads - zp) * scale - flt) / scale:.3f} LSB")

    print("\n5. Section 2 of profiles/quant_report.txt under each choice of ranges (the model quantised on the device from the shipped .yfw, run on the engine,")
    print("   int8 tensors against float32 tensors): head sqnr_db, mean sqnr_db over the report's tensors, lowest sqnr_db (tensor)")
    for method in ("minmax", "percentile", "mse", "head"):
        yfm = calib.quantize_on_device(shipped_yfw, d_x, ranges=method, percentile=a.percentile, bins=a.bins)
        net.init_model(yfm)
        rep = calib.quantisation_report(net, shipped_yfw, yfm, x)
        low = min(rep, key=lambda r: r["sqnr_db"])
        print(f"   {method:10s}  head {rep[-1]['sqnr_db']:6.2f}   mean {float(np.mean([r['sqnr_db'] for r in rep])):6.2f}   lowest {low['sqnr_db']:6.2f} ({low['tensor']})")
    net.init_model(shipped_yfm)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--yfw")
    ap.add_argument("--yfm")
    ap.add_argument("--frames", default=os.path.join(ROOT, "tests", "golden", "calib_frames_56_cv.bin"))
    ap.add_argument("--bench-frames", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ranges", choices=("minmax", "percentile", "mse", "head"), default="minmax")
    ap.add_argument("--sensitivity", action="store_true", help="write the record of profiles/quant_sensitivity.txt instead")
    ap.add_argument("--percentile", type=float, default=0.9999)
    ap.add_argument("--bins", type=int, default=2048)
    ap.add_argument("--size", type=int, default=56, help="the side of the frames in --frames (56 or 160)")
    a = ap.parse_args()
    if bool(a.yfw) != bool(a.yfm):
        ap.error("--yfw and --yfm go together")
    if a.size != 56 and not a.yfw:
        ap.error("--size: the record without --yfw / --yfm is taken at 56x56")
    import torch
    if not torch.cuda.is_available():
        sys.exit("quant_report: needs a GPU (the engine and the comparison run there)")
    yf = importlib.import_module("stm32h7-yolo_amd")
    calib = importlib.import_module("stm32h7-yolo_amd.calib")
    model_file = importlib.import_module("stm32h7-yolo_amd.model_file")
    x = np.fromfile(a.frames, np.int8)
    if x.size == 0 or x.size % (a.size * a.size * 3):
        sys.exit(f"quant_report: {a.frames} holds {x.size} bytes, expected a multiple of {a.size * a.size * 3}")
    x = x.reshape(-1, a.size, a.size, 3)
    net = yf.Network(device=0)
    if a.yfw:
        yfw, yfm = open(a.yfw, "rb").read(), open(a.yfm, "rb").read()
        net.init_model(yfm)
        print(f"{a.yfm} against {a.yfw} over the {x.shape[0]} frames of {a.frames}")
        if a.size != 56:
            print(f"frames of {a.size}x{a.size}: the head alone -- the engine dumps its stages' tensors at 56x56 only")
        print_table(calib.quantisation_report(net, yfw, yfm, x))
        net.destroy()
        return 0
    z = np.load(os.path.join(ROOT, "tests", "golden", "ptq_float_convs.npz"))
    npz_yfw = model_file.write_yfw([(z[f"w{k}"], z[f"b{k}"], bool(z[f"dw{k}"])) for k in range(24)])
    shipped_yfm = open(os.path.join(ROOT, "oracle", "model", "yoloface_int8.yfm"), "rb").read()
    shipped_yfw = open(os.path.join(ROOT, "stm32h7-yolo_amd", "model", "yoloface_fp32.yfw"), "rb").read()
    if a.sensitivity:
        sensitivity_record(a, torch, calib, model_file, net, x, npz_yfw, shipped_yfw, shipped_yfm)
        net.destroy()
        return 0
    print("Quantisation error per tensor, int8 engine against the float32 evaluation (calib.quantisation_report; csrc/yf_calib_compare.h), as")
    print(f"tools/quant_report.py printed it on: {torch.cuda.get_device_name(0)}, libyf_calib.so build id {calib.load().yf_calib_build_id().decode()}, "
          f"libyf_network.so build id {net.build_id}")
    print(f"Frames: the {x.shape[0]} of {os.path.relpath(a.frames, ROOT)}.  error = dequantised int8 - float32; max/scale is max_abs_error in LSB of the tensor.")
    print("\n1. oracle/model/yoloface_int8.yfm (the shipped model) against tests/golden/ptq_float_convs.npz (the float weights it came from)")
    net.init_model(shipped_yfm)
    print_table(calib.quantisation_report(net, npz_yfw, shipped_yfm, x))
    how = "" if a.ranges == "minmax" else f", ranges={a.ranges}" + (f", percentile={a.percentile}" if a.ranges == "percentile" else "") + f", bins={a.bins}"
    print(f"\n2. calib.quantize_on_device(stm32h7-yolo_amd/model/yoloface_fp32.yfw, the same frames{how}) against that .yfw")
    new_yfm = calib.quantize_on_device(shipped_yfw, torch.from_numpy(x).cuda(), ranges=a.ranges, percentile=a.percentile, bins=a.bins)
    net.init_model(new_yfm)
    print_table(calib.quantisation_report(net, shipped_yfw, new_yfm, x))
    net.init_model(shipped_yfm)
    bench(a, torch, calib, net, npz_yfw, shipped_yfm)
    net.destroy()
    return 0


if __name__ == "__main__":
    sys.exit(main())
