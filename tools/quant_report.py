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

--bias-correction MODE (sequential or once) writes the record profiles/bias_correction.txt holds instead: the time of one channel-sums launch
(calib.Calibration.channel_sums; csrc/yf_calib_chan.h) beside a simulate launch under the same tables, at 56x56 and at 160x160, and, with
--parent-lib DIR/libyf_calib.so (built from the parent commit), that build's simulate and observe in the same run; the wall time of a whole
calib.correct_biases call in each mode; and what the correction does to the shipped pair and to the model quantised on the device -- the
rows of correct_biases' report, the head's SQNR by the full simulation and by the engine before and after, and the engine's per-tensor table
(mean_error among its columns) before and after in MODE -- on min/max ranges and on ranges="mse".

    python tools/quant_report.py --bias-correction sequential [--parent-lib DIR/libyf_calib.so] > profiles/bias_correction.txt

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


def kernel_registers(names):
    """one line per kernel of csrc/yf_calib.hip whose name holds one of `names`: VGPRs, SGPRs, spills, scratch and static LDS as the code object's
    metadata states them (hipcc -S --cuda-device-only with CALIBFLAGS)"""
    import re
    import subprocess
    import tempfile
    libs = importlib.import_module("stm32h7-yolo_amd.libs")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "yf_calib.s")
        cmd = [os.environ.get("HIPCC", os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc"))] + libs.make_var("CALIBFLAGS").split() + ["-S", "--cuda-device-only", os.path.join(libs.CSRC, "yf_calib.hip"), "-o", out]
        try:
            subprocess.check_call(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            text = open(out).read()
        except (OSError, subprocess.CalledProcessError) as e:
            return [f"not read: {e}"]
    lines = []
    for blk in re.findall(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", text, flags=re.S):
        g = lambda k: re.search(r"\.%s:\s+(\S+)" % k, blk).group(1)
        name = re.search(r"yfc_\w+?_kernel", g("name"))
        if name and any(k in name.group(0) for k in names):
            lines.append(f"{name.group(0):28s} {g('vgpr_count'):>3} VGPRs  {g('sgpr_count'):>3} SGPRs  VGPR spill {g('vgpr_spill_count')}  scratch "
                         f"{g('private_segment_fixed_size')} B  static LDS {g('group_segment_fixed_size')} B")
    return lines


def bias_correction_record(a, torch, calib, model_file, net, x, npz_yfw, shipped_yfw):
    """the record of profiles/bias_correction.txt"""
    import ctypes
    import math
    import time
    ptq = importlib.import_module("stm32h7-yolo_amd.ptq")
    lib = calib.load()
    print("Empirical bias correction (calib.correct_biases): per output channel of each convolution the mean of the simulated network's raw output")
    print("against the float network's, folded into the bias; the sums come from yf_calib_channel_sums_device (csrc/yf_calib_chan.h).  As")
    print(f"tools/quant_report.py --bias-correction {a.bias_correction} printed it on: {torch.cuda.get_device_name(0)}, libyf_calib.so build id "
          f"{lib.yf_calib_build_id().decode()}, libyf_network.so build id {net.build_id}")

    # (a) one launch
    vp, ci, cl = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    parent = None
    if a.parent_lib:
        parent = ctypes.CDLL(a.parent_lib)
        parent.yf_calib_create.restype, parent.yf_calib_create.argtypes = vp, [ctypes.c_char_p, ctypes.c_size_t, ci]
        parent.yf_calib_observe_device.restype, parent.yf_calib_observe_device.argtypes = cl, [vp, vp, cl, vp, vp]
        parent.yf_calib_observe_hw_device.restype, parent.yf_calib_observe_hw_device.argtypes = cl, [vp, ci, ci, vp, cl, vp, vp]
        parent.yf_calib_simulate_device.restype, parent.yf_calib_simulate_device.argtypes = cl, [vp, vp, cl, vp, vp, vp, vp, vp, vp]
        parent.yf_calib_simulate_hw_device.restype, parent.yf_calib_simulate_hw_device.argtypes = cl, [vp, ci, ci, vp, cl, vp, vp, vp, vp, vp, vp]
        parent.yf_calib_destroy.restype, parent.yf_calib_destroy.argtypes = None, [vp]
        parent.yf_calib_build_id.restype = ctypes.c_char_p
    shipped_yfm = open(os.path.join(ROOT, "oracle", "model", "yoloface_int8.yfm"), "rb").read()
    tables = (("all entries disabled", calib.empty_table()), ("all entries enabled", calib.simulation_table(shipped_yfm)))
    print(f"\n(a) One launch over random frames resident in HBM, {a.launches} launches after {a.warmup} warm-up, HIP events, median (min, max) in ms.")
    print("    channel sums: per-frame sums, totals and logits written; simulate: logits written, no reference; observe: logits written.")
    if parent:
        print(f"    libyf_calib.so of the parent commit: build id {parent.yf_calib_build_id().decode()}, loaded beside this build's, timed in the same run")
    for h, n in ((56, a.bench_frames), (160, max(a.bench_frames // 4, 1))):
        hw = h != 56
        d_x = torch.from_numpy(np.random.default_rng(n + h).integers(-128, 128, (n, h, h, 3), dtype=np.int8)).cuda()
        cal = calib.Calibration(npz_yfw)
        d_rows = torch.empty((n, calib.CHANNELS), dtype=torch.float64, device="cuda")
        d_sums = torch.empty((calib.CHANNELS,), dtype=torch.float64, device="cuda")
        d_l = torch.empty((n, h // 8, h // 8, 18), dtype=torch.float32, device="cuda")
        stream, X, L = torch.cuda.current_stream().cuda_stream, d_x.data_ptr(), d_l.data_ptr()
        ph = parent.yf_calib_create(npz_yfw, len(npz_yfw), 0) if parent else None
        if parent and not ph:
            sys.exit("quant_report: yf_calib_create of the parent library failed")

        def chan(t):
            tail = (X, n, t.ctypes.data, d_rows.data_ptr(), d_sums.data_ptr(), L, stream)
            rc = lib.yf_calib_channel_sums_hw_device(cal.handle, h, h, *tail) if hw else lib.yf_calib_channel_sums_device(cal.handle, *tail)
            assert rc == n, cal._text()

        def sim(which, handle, t):
            tail = (X, n, t.ctypes.data, None, L, None, None, stream)
            rc = which.yf_calib_simulate_hw_device(handle, h, h, *tail) if hw else which.yf_calib_simulate_device(handle, *tail)
            assert rc == n

        def obs(which, handle):
            rc = which.yf_calib_observe_hw_device(handle, h, h, X, n, L, stream) if hw else which.yf_calib_observe_device(handle, X, n, L, stream)
            assert rc == n

        print(f"\n    {h}x{h}, {n} frames ({'yfc_channel_sums_hw_kernel, the arena in a slab' if hw else 'yfc_channel_sums_kernel, the arena in LDS'})")
        for name, t in tables:
            c = timed(torch, lambda: chan(t), a.launches, a.warmup)
            s = timed(torch, lambda: sim(lib, cal.handle, t), a.launches, a.warmup)
            print(f"    {name:22s} channel sums {c[0]:8.3f}  ({c[1]:.3f}, {c[2]:.3f})   simulate {s[0]:8.3f}  ({s[1]:.3f}, {s[2]:.3f})   ratio {c[0] / s[0]:.2f}x")
            if parent:
                ps = timed(torch, lambda: sim(parent, ph, t), a.launches, a.warmup)
                print(f"    {'':22s} simulate of the parent commit's library {ps[0]:8.3f}  ({ps[1]:.3f}, {ps[2]:.3f})   this build / parent {s[0] / ps[0]:.3f}")
        o = timed(torch, lambda: obs(lib, cal.handle), a.launches, a.warmup)
        print(f"    {'observe':22s} this build {o[0]:8.3f}  ({o[1]:.3f}, {o[2]:.3f})", end="")
        if parent:
            po = timed(torch, lambda: obs(parent, ph), a.launches, a.warmup)
            print(f"   parent commit {po[0]:8.3f}  ({po[1]:.3f}, {po[2]:.3f})   this build / parent {o[0] / po[0]:.3f}", end="")
            parent.yf_calib_destroy(ph)
        print()
        cal.destroy()
        del d_x, d_rows, d_l
    print("    Registers, from the code object's metadata (csrc/yf_calib.hip compiled to assembly with the library's flags):")
    for line in kernel_registers(("channel_sums", "simulate")):
        print("    " + line)

    # (b) a whole call
    big = torch.from_numpy(np.random.default_rng(4096).integers(-128, 128, (a.bench_frames, 56, 56, 3), dtype=np.int8)).cuda()
    cal = calib.Calibration(shipped_yfw)
    cal.observe(big, logits=False)
    big_ranges = cal.ranges()
    cal.destroy()
    print(f"\n(b) Wall time of one calib.correct_biases call at 56x56 on {a.bench_frames} random frames resident in HBM (the shipped .yfw, min/max ranges of the same frames)")
    for mode in calib.BIAS_MODES:
        calib.correct_biases(shipped_yfw, big_ranges, big[:64], mode=mode)
        torch.cuda.synchronize()
        t = time.perf_counter()
        calib.correct_biases(shipped_yfw, big_ranges, big, mode=mode)
        torch.cuda.synchronize()
        print(f"    {mode:10s} {time.perf_counter() - t:.3f} s  ({1 + (24 if mode == 'sequential' else 1)} passes, a handle created and destroyed for each)")
    del big

    # (c) the effect
    d_x = torch.from_numpy(x).cuda()
    first, cout, _ = calib.channel_layout()

    def head_sim(yfw, yfm):
        """the head's SQNR in the full simulation of yfm against the float logits of yfw"""
        ref_cal, cal = calib.Calibration(yfw), calib.Calibration(ptq.dequantized_yfw(yfw, yfm))
        try:
            ref = ref_cal.simulate(d_x, calib.empty_table())[0]
            r = cal.simulate(d_x, calib.simulation_table(yfm), ref)[1][0]
        finally:
            ref_cal.destroy(); cal.destroy()
        return 10.0 * math.log10(float(r["sum_sq_ref"]) / float(r["sum_sq_err"])), float(r["sum_err"]) / int(r["elements"])

    def engine(yfw, yfm):
        net.init_model(yfm)
        return calib.quantisation_report(net, yfw, yfm, x)

    def head_row(rows):
        return [r for r in rows if r["tensor"] == 100][0]

    def effect(title, yfw, ranges):
        print("\n" + title)
        plain = ptq.quantize_model(yfw, ranges)
        models = {None: plain}
        reports = {}
        for mode in calib.BIAS_MODES:
            models[mode], reports[mode] = calib.correct_biases(yfw, ranges, d_x, mode=mode)
        tables = {mode: engine(yfw, m) for mode, m in models.items()}
        print("    head (tensor 100)          simulation sqnr_db  simulation mean_error   engine sqnr_db  engine mean_error  engine mean sqnr_db over the tensors")
        for mode in (None,) + calib.BIAS_MODES:
            s, e = head_sim(yfw, models[mode]), head_row(tables[mode])
            print(f"    {'uncorrected' if mode is None else mode:26s} {s[0]:18.2f}  {s[1]:+21.6e}   {e['sqnr_db']:14.2f}  {e['mean_error']:+17.6e}  "
                  f"{float(np.mean([r['sqnr_db'] for r in tables[mode]])):10.2f}")
        print("    per tensor, the engine against the float evaluation: mean_error uncorrected -> sequential | once, and sqnr_db likewise")
        for r0, r1, r2 in zip(tables[None], tables["sequential"], tables["once"]):
            print(f"    tensor {r0['tensor']:3d}  scale {r0['scale']:.6f}  mean_error {r0['mean_error']:+.5f} -> {r1['mean_error']:+.5f} | {r2['mean_error']:+.5f}"
                  f"   sqnr_db {r0['sqnr_db']:6.2f} -> {r1['sqnr_db']:6.2f} | {r2['sqnr_db']:6.2f}")
        mode = a.bias_correction
        print(f"    the report of correct_biases(mode={mode!r}): the largest and rms |mean_sim - mean_float| over a convolution's channels before its correction,")
        print("    in units of its output's scale")
        for line in calib.format_bias_report(reports[mode]).split("\n"):
            print("    " + line)
        return tables, models

    cal = calib.Calibration(npz_yfw)
    cal.observe(d_x, logits=False)
    npz_ranges = cal.ranges()
    cal.destroy()
    cal = calib.Calibration(shipped_yfw)
    cal.observe(d_x, logits=False)
    observed = cal.ranges()
    counts = cal.histogram(d_x, observed, a.bins).cpu().numpy()
    cal.destroy()
    print(f"\n(c) The effect, over the {x.shape[0]} frames of {os.path.relpath(a.frames, ROOT)} (the frames the ranges and the correction are taken on).  error = dequantised int8 -")
    print("    float32; simulation: the model's dequantised weights under its whole table against the float logits (float arithmetic on the int8 grid);")
    print("    engine: calib.quantisation_report, the int8 network that runs.")
    t1, m1 = effect("(c1) tests/golden/ptq_float_convs.npz (the float weights the shipped model came from), min/max ranges of these frames", npz_yfw, npz_ranges)
    t2, m2 = effect("(c2) stm32h7-yolo_amd/model/yoloface_fp32.yfw (the shipped .yfw), min/max ranges: quantize_on_device's model", shipped_yfw, observed)
    assert m2[None] == calib.quantize_on_device(shipped_yfw, d_x) and m2["sequential"] == calib.quantize_on_device(shipped_yfw, d_x, bias_correction="sequential")
    t3, _ = effect('(c3) the same .yfw on ranges="mse"', shipped_yfw, ptq.clip_ranges(counts, observed, "mse", a.percentile))
    print(f"\n    the engine's own table of (c2), uncorrected and then with mode={a.bias_correction!r}:")
    print_table(t2[None])
    print_table(t2[a.bias_correction])
    print("\nVERDICT.  Head SQNR on the engine, uncorrected -> sequential | once:")
    for name, t in (("c1", t1), ("c2", t2), ("c3", t3)):
        h0, h1, h2 = (head_row(t[m])["sqnr_db"] for m in (None,) + calib.BIAS_MODES)
        print(f"    {name}: {h0:.2f} dB -> {h1:.2f} dB | {h2:.2f} dB   ({'improves' if h1 > h0 else 'does NOT improve'} under sequential, "
              f"{'improves' if h2 > h0 else 'does NOT improve'} under once)")
    print("    These are the frames the ranges and the correction were taken on: no held-out frames are scored here.")
    print("    `once` measures every convolution's offset with the offsets of the convolutions before it still in its input, and then removes those")
    print("    as well: the corrections compound.  It is kept for comparison; `sequential` is the mode to use.")
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
    ap.add_argument("--bias-correction", choices=("sequential", "once"), help="write the record of profiles/bias_correction.txt instead")
    ap.add_argument("--parent-lib", help="with --bias-correction: libyf_calib.so built from the parent commit, timed beside this build's")
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
    if a.bias_correction:
        bias_correction_record(a, torch, calib, model_file, net, x, npz_yfw, shipped_yfw)
        net.destroy()
        return 0
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
