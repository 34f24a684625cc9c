#!/usr/bin/env python3
"""Redaction by blur on the GPU: what the three launches of yf_images_blur_records_device / _yuv_device cost beside the mosaic and the fill
on the same records in the same run (GPU TOOL; bench.py is not involved).  Device events around every call, warm-up first, the calls
interleaved inside one loop, the median [least .. most] of the timed calls, as tools/redact_bench.py does.  A second call blurs the blur,
but it reads and writes the same bytes: every timed call does the same work.

    real      4096 pictures of 410x362 with real content (the 27 real frames of tests/golden upscaled to that size, repeated), as BGR and
              as NV12 surfaces; the ragged run at 56x56 and the suppression at 0.4 leave the records.  Per call: the blur at grid 8 and at
              grid 16, the mosaic at k = 8 (the yardstick: the existing way to hide these faces, which like the blur reads every region
              byte once and writes it once), the fill, and the network call.
    worst     every candidate of every frame firing, unsuppressed: 147 records per frame that overlap heavily.
    bandwidth the touched-lines model of tools/redact_bench.py: the distinct 128-byte lines that hold a byte of the regions, read once and
              written once by the blur, against 6.3 TB/s.
    launches  with --kernel-stats (the kernel_stats.csv of a `rocprofv3 --kernel-trace --stats` run of this tool, a run of its own): the
              average time of each launch -- the scan, the means, the paint, the mosaic, the fill.
    hashes    with --parent-lib (a libyf_images.so built from the parent commit): tools/isa_hashes.py on it and on this build -- the
              kernels that existed before keep their instruction streams.  Needs no GPU: --only hashes.

    python tools/blur_bench.py [--iters 30] [--warmup 5] [--only real|worst|hashes|launches] [--grids 8,16] [--parent-lib PATH]
                               [--kernel-stats CSV] [--out profiles/blur_bench.txt]
"""
import argparse
import csv
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 410, 362
HBM_TBPS = 6.3
COLOUR = 0x00C82D5A
LAUNCHES = ("yfcrop::first_kernel", "yfblur::means_kernel", "yfblur::paint_kernel", "yfredact::mosaic_kernel", "yfredact::mosaic_yuv_kernel",
            "yfredact::fill_kernel", "yfredact::fill_yuv_kernel")


def launches_statement(path):
    """the rows of a rocprofv3 kernel_stats.csv that are this tool's launches"""
    lines = []
    for row in csv.DictReader(open(path)):
        if any(name in row["Name"] for name in LAUNCHES):
            lines.append(f"launch: {row['Name']}: {int(row['Calls'])} launches, average {float(row['AverageNs']) / 1e3:8.2f} us "
                         f"[{float(row['MinNs']) / 1e3:.2f} .. {float(row['MaxNs']) / 1e3:.2f}]")
    return lines or [f"launch: no row of {path} names one of {', '.join(LAUNCHES)}"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--kernel-stats", default="")
    ap.add_argument("--grids", default="8,16", help="the grids of the blur calls (one grid alone: a kernel trace's averages are that grid's)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blur_bench.txt"))
    args = ap.parse_args()
    images = importlib.import_module("stm32h7-yolo_amd.images")
    text = []

    def say(line):
        print(line, flush=True)
        text.append(line)

    if args.parent_lib:
        from tools.draw_bench import hashes_statement
        for line in hashes_statement(images, args.parent_lib):
            say(line)
    if args.kernel_stats:
        for line in launches_statement(args.kernel_stats):
            say(line)
    if args.only in ("hashes", "launches"):
        open(args.out, "w").write("\n".join(text) + "\n")
        return
    import torch
    from images_yuv_support import bgr_to_nv12
    from tools.redact_bench import touched_lines
    yf = importlib.import_module("stm32h7-yolo_amd")
    ptq = importlib.import_module("stm32h7-yolo_amd.ptq")
    binding = importlib.import_module("stm32h7-yolo_amd.binding")
    if not torch.cuda.is_available():
        raise SystemExit("tools/blur_bench.py measures on a GPU; none is visible (--only hashes needs none)")
    net = yf.Network(device=0).init()
    lib = images.load()
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    dev = "cuda"
    n, cap = 4096, 147
    grids = [int(g) for g in args.grids.split(",")]
    say(f"# libyf_images build {(lib.yf_images_build_id() or b'').decode()}, network build {net.build_id}; {torch.cuda.get_device_name(0)}")
    say(f"# {args.iters} timed calls after {args.warmup} warm-up, the calls of a row interleaved in one loop; per call the median "
        f"[least .. most] of device events around all its launches")

    def timed(*fns):
        """(median, least, most) in us of each call, the calls timed in turn inside one loop"""
        for _ in range(args.warmup):
            for fn in fns:
                fn()
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(len(fns) + 1)] for _ in range(args.iters)]
        for row in ev:
            row[0].record(stream)
            for k, fn in enumerate(fns):
                fn()
                row[k + 1].record(stream)
        torch.cuda.synchronize()
        out = []
        for k in range(len(fns)):
            t = np.array([row[k].elapsed_time(row[k + 1]) for row in ev]) * 1e3
            out.append((float(np.median(t)), float(t.min()), float(t.max())))
        return out

    # the pictures, as BGR and as NV12 surfaces of the same content
    real = np.fromfile(os.path.join(ROOT, "tests", "golden", "real_frames_56.bin"), np.int8).reshape(-1, 56, 56, 3)
    rgb56 = (real.astype(np.int16) + 128).astype(np.uint8)
    photos = [np.ascontiguousarray(ptq.resize_linear_u8(f, W, H)[..., ::-1]) for f in rgb56]
    surfaces = [bgr_to_nv12(p) for p in photos]
    size = (H * W * 3 + 15) // 16 * 16
    desc = np.zeros(n, images.IMAGE_DTYPE)
    desc["offset"], desc["height"], desc["width"], desc["row_stride"] = np.arange(n, dtype=np.int64) * size, H, W, W * 3
    nbytes = int(desc["offset"][-1]) + H * W * 3
    buf = np.zeros(nbytes, np.uint8)
    ysize = (H * W * 3 // 2 + 15) // 16 * 16
    ydesc = np.zeros(n, images.YUV_IMAGE_DTYPE)
    ydesc["offset_y"] = np.arange(n, dtype=np.int64) * ysize
    ydesc["offset_uv"], ydesc["height"], ydesc["width"], ydesc["stride_y"], ydesc["stride_uv"] = ydesc["offset_y"] + H * W, H, W, W, W
    ynbytes = int(ydesc["offset_uv"][-1]) + H // 2 * W
    ybuf = np.zeros(ynbytes, np.uint8)
    for i in range(n):
        o = int(desc["offset"][i])
        buf[o:o + H * W * 3] = photos[i % len(photos)].reshape(-1)
        y, uv = surfaces[i % len(surfaces)]
        o = int(ydesc["offset_y"][i])
        ybuf[o:o + H * W] = y.reshape(-1)
        ybuf[o + H * W:o + H * W * 3 // 2] = uv.reshape(-1)
    d_px, d_desc = torch.from_numpy(buf).to(dev), torch.from_numpy(desc.view(np.uint8)).to(dev)
    d_ypx, d_ydesc = torch.from_numpy(ybuf).to(dev), torch.from_numpy(ydesc.view(np.uint8)).to(dev)
    d_frames = torch.empty((n, 56, 56, 3), dtype=torch.int8, device=dev)
    d_heads = torch.empty((n, 7, 7, 18), dtype=torch.int8, device=dev)
    d_dets = torch.empty((n, cap, 28), dtype=torch.uint8, device=dev)
    d_counts = torch.empty(n, dtype=torch.int32, device=dev)
    d_status = torch.empty(n, dtype=torch.int32, device=dev)
    d_first = torch.empty(n + 1, dtype=torch.int32, device=dev)
    images.set_decode_tables(*net.decode_tables())
    network = lambda: net.run_device(d_frames.data_ptr(), d_heads.data_ptr(), n, s)

    def redact(yuv, mode, block):
        fn, px, nb, dd, fmt = ((images.redact_records_yuv_device, d_ypx, ynbytes, d_ydesc, "nv12") if yuv else
                               (images.redact_records_device, d_px, nbytes, d_desc, "bgr"))
        return lambda: fn(px.data_ptr(), nb, fmt, dd.data_ptr(), d_dets.data_ptr(), d_counts.data_ptr(), n, cap, d_first.data_ptr(),
                          d_status.data_ptr(), mode=mode, block=block, colour=COLOUR, stream=s)

    def blur(yuv, grid, d_work, room, records_cap):
        fn, px, nb, dd, fmt = ((images.blur_records_yuv_device, d_ypx, ynbytes, d_ydesc, "nv12") if yuv else
                               (images.blur_records_device, d_px, nbytes, d_desc, "bgr"))
        return lambda: fn(px.data_ptr(), nb, fmt, dd.data_ptr(), d_dets.data_ptr(), d_counts.data_ptr(), n, cap, d_work.data_ptr(), room,
                          records_cap, d_first.data_ptr(), d_status.data_ptr(), grid=grid, colour=COLOUR, stream=s)

    def report(name):
        torch.cuda.synchronize()
        counts = d_counts.cpu().numpy()
        dets = d_dets.cpu().numpy().view(binding.DET_DTYPE).reshape(n, cap)
        total = int(np.clip(counts, 0, cap).sum())
        room = images.blur_workspace(total, 16)                                # the workspace of both grids: exactly the records that exist
        d_work = torch.empty(max(room, 16), dtype=torch.uint8, device=dev)
        say(f"{name:5s} {n} x {W}x{H}, {total} records (at most {int(counts.max())} per frame); workspace {room} bytes")
        for yuv in (False, True):
            calls = tuple((f"blur g = {g}", blur(yuv, g, d_work, room, total)) for g in grids) + (
                ("mosaic k = 8", redact(yuv, "mosaic", 8)), ("fill", redact(yuv, "fill", 0)), ("network", network))
            times = timed(*(fn for _, fn in calls))
            if yuv:
                lines = (touched_lines(ptq, dets, counts, cap, ydesc["offset_y"], W, 1, 0)
                         + touched_lines(ptq, dets, counts, cap, ydesc["offset_uv"], W, 1, 0, rows=H // 2, chroma=True))
            else:
                lines = touched_lines(ptq, dets, counts, cap, desc["offset"], W * 3, 3, 0)
            t_mosaic, t_net = times[-3][0], times[-1][0]
            for (label, _), (t, lo, hi) in zip(calls, times):
                line = f"{name:5s} {'NV12' if yuv else 'BGR ':4s} {label:12s} per call {t:8.2f} us [{lo:8.2f} .. {hi:8.2f}]"
                if label.startswith("blur"):
                    line += (f" = {t / t_mosaic:5.2f} x the mosaic at k = 8, {100 * t / t_net:7.2f} % of the network call; touched lines "
                             f"{lines / 1e6:7.2f} MB, read and written: {2 * lines / (t * 1e-6) / 1e9:6.0f} GB/s "
                             f"({100 * 2 * lines / (t * 1e-6) / 1e12 / HBM_TBPS:4.1f} % of {HBM_TBPS} TB/s)")
                say(line)
        assert int((d_status.cpu().numpy() & 1).sum()) == 0 and int(d_first[n].item()) == total
        del d_work

    if not args.only or args.only == "real":
        images.run_decode_ragged_device(net, d_px.data_ptr(), nbytes, "bgr", d_desc.data_ptr(), n, d_frames.data_ptr(), d_heads.data_ptr(),
                                        d_dets.data_ptr(), d_counts.data_ptr(), cap, d_status.data_ptr(), stream=s)
        images.nms_device(d_dets.data_ptr(), d_counts.data_ptr(), n, cap, 0.4, stream=s)
        report("real")
    if not args.only or args.only == "worst":
        h = np.random.default_rng(3).integers(-128, 128, (n, 7, 7, 18), dtype=np.int16)
        h[..., 4::6] = 120
        d_heads.copy_(torch.from_numpy(h.astype(np.int8)))
        net.decode_device(d_heads.data_ptr(), n, d_dets.data_ptr(), d_counts.data_ptr(), cap, w_scale=W / 56., h_scale=H / 56., stream=s)
        report("worst")
    net.destroy()
    open(args.out, "w").write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
