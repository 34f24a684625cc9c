#!/usr/bin/env python3
"""Rate of libyf_images on NV12 surfaces against the same pictures as packed BGR, in one run (GPU TOOL; bench.py is not involved).  The method
is that of tools/images_bench.py (profiles/images_bench.txt): device events around every launch, warm-up first, the median of the timed
launches, inputs rotating over two buffers per workload and format.  Workloads: 4096 surfaces of 410x362, 4096 of 640x480, 1024 of
1920x1080, and a ragged 4096 of the 27 reference sizes cropped to even sides.

Per workload and format: the prepare alone (time, images/s, GB/s on the touched-lines model) and prepare + network + decode.  The model
counts the distinct 128-byte lines the sampled bytes fall in, computed per image from the tap tables: for BGR the three channels of two
rows and two columns per output pixel, for NV12 the sampled Y bytes and, in the second plane, the chroma pairs of those samples.
The BGR prepare is timed twice (the second figure shows the run-to-run spread inside the process) and, with --parent-lib, once more through
another build of libyf_images.so -- the parent commit's -- loaded beside this one: the existing kernels must not have moved
(tools/ab_libs.py compares builds of libyf_network.so, one process per library; the prepare needs no network, so here both builds share
the process, the buffers and the clock state).
NV12's prepare + network + decode is yf_images_prepare_yuv_*, yf_network_run_device and yf_images_decode_ragged_device (three launches);
BGR's is the run_decode entry of tools/images_bench.py (uniform: the decode fused into the network's launch).

    python tools/images_yuv_bench.py [--iters 60] [--warmup 10] [--only NAME] [--parent-lib PATH/libyf_images.so]
"""
import argparse
import ctypes
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from images_bench import HBM_TBPS, REF_SIZES, taps, touched_lines          # noqa: E402


def touched_lines_yuv(host, desc):
    """distinct 128-byte lines read per batch of surfaces: the Y plane's and the UV plane's, each from its own offset and pitch"""
    cache, total = {}, 0
    for oy, ouv, h, w, sy, suv in zip(*(desc[k].tolist() for k in ("offset_y", "offset_uv", "height", "width", "stride_y", "stride_uv"))):
        if (h, w) not in cache:
            ty, tx = taps(host, h).reshape(-1), taps(host, w).reshape(-1)
            cache[(h, w)] = (np.unique(ty), np.unique(tx), np.unique(ty >> 1),
                             np.unique(((tx >> 1) * 2)[:, None] + np.arange(2)[None, :]))
        rows, cols, crows, ccols = cache[(h, w)]
        total += np.unique((oy + rows[:, None] * sy + cols[None, :]) // 128).size
        total += np.unique((ouv + crows[:, None] * suv + ccols[None, :]) // 128).size
    return total * 128


def workloads():
    even = [(h & ~1, w & ~1) for (w, h) in REF_SIZES]
    yield "uniform 4096 x 410x362", [(362, 410)] * 4096, True
    yield "uniform 4096 x 640x480", [(480, 640)] * 4096, True
    yield "uniform 1024 x 1920x1080", [(1080, 1920)] * 1024, True
    yield "ragged 4096 x 27 even reference sizes", even * (4096 // 27) + even[:4096 % 27], False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--only", default="")
    ap.add_argument("--parent-lib", default="", help="another build of libyf_images.so whose BGR prepare is timed in the same run")
    args = ap.parse_args()
    import torch
    yf = importlib.import_module("stm32h7-yolo_amd")
    images = importlib.import_module("stm32h7-yolo_amd.images")
    net = yf.Network(device=0).init()
    lib = images.load()
    images.set_decode_tables(*net.decode_tables())
    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        parent.yf_images_build_id.restype = ctypes.c_char_p
        for name in ("prepare_device", "prepare_ragged_device"):
            fn = getattr(parent, "yf_images_" + name)
            fn.restype, fn.argtypes = ctypes.c_long, images._ENTRIES[name]
    host = importlib.import_module("stm32h7-yolo_amd.libs").host_library("libyf_images_host.so")
    host.yfi_tap_host.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    print(f"# libyf_images build {(lib.yf_images_build_id() or b'').decode()}, network build {net.build_id}; {torch.cuda.get_device_name(0)}")
    if parent is not None:
        print(f"# parent: libyf_images build {(parent.yf_images_build_id() or b'').decode()}")
    print(f"# {args.iters} timed launches after {args.warmup} warm-up, median of per-launch device events; inputs rotate over 2 buffers per format")

    def time(fn):
        for i in range(args.warmup):
            fn(i)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.iters)]
        for i, (a, e) in enumerate(ev):
            a.record(stream)
            fn(i)
            e.record(stream)
        torch.cuda.synchronize()
        return float(np.median([a.elapsed_time(e) for a, e in ev])) * 1e-3

    for name, dims, uniform in workloads():
        if args.only and args.only not in name:
            continue
        n = len(dims)
        hs, ws = np.array([d[0] for d in dims], np.int64), np.array([d[1] for d in dims], np.int64)
        # BGR: packed rows, images 16-byte aligned one after the other
        bgr = np.zeros(n, images.IMAGE_DTYPE)
        sizes = hs * ws * 3
        offs = np.concatenate([[0], np.cumsum((sizes + 15) // 16 * 16)[:-1]])
        bgr["offset"], bgr["height"], bgr["width"], bgr["row_stride"] = offs, hs, ws, ws * 3
        bgr_bytes = int(offs[-1] + sizes[-1])
        bgr_fs = int(offs[1]) if n > 1 else 0
        # NV12: packed rows, the UV plane straight after the Y plane, surfaces 16-byte aligned one after the other
        yuv = np.zeros(n, images.YUV_IMAGE_DTYPE)
        ysizes = hs * ws * 3 // 2
        yoffs = np.concatenate([[0], np.cumsum((ysizes + 15) // 16 * 16)[:-1]])
        yuv["offset_y"], yuv["offset_uv"], yuv["height"], yuv["width"], yuv["stride_y"], yuv["stride_uv"] = yoffs, yoffs + hs * ws, hs, ws, ws, ws
        yuv_bytes = int(yoffs[-1] + ysizes[-1])
        yuv_fs = int(yoffs[1]) if n > 1 else 0
        h0, w0 = dims[0]
        bufs = {"bgr": [torch.randint(0, 256, (bgr_bytes,), dtype=torch.uint8, device="cuda") for _ in range(2)],
                "nv12": [torch.randint(0, 256, (yuv_bytes,), dtype=torch.uint8, device="cuda") for _ in range(2)]}
        d_bgr = torch.from_numpy(bgr.view(np.uint8).copy()).cuda()
        d_yuv = torch.from_numpy(yuv.view(np.uint8).copy()).cuda()
        frames = torch.empty((n, 56, 56, 3), dtype=torch.int8, device="cuda")
        heads = torch.empty((n, 7, 7, 18), dtype=torch.int8, device="cuda")
        dets = torch.empty((n, 147, 28), dtype=torch.uint8, device="cuda")
        counts = torch.empty(n, dtype=torch.int32, device="cuda")
        status = torch.empty(n, dtype=torch.int32, device="cuda")

        def prep_bgr(i, which=lib):
            b = bufs["bgr"][i % 2].data_ptr()
            if uniform:
                rc = which.yf_images_prepare_device(b, bgr_bytes, 0, h0, w0, w0 * 3, bgr_fs, n, 56, frames.data_ptr(), s)
            else:
                rc = which.yf_images_prepare_ragged_device(b, bgr_bytes, 0, d_bgr.data_ptr(), n, 56, frames.data_ptr(), status.data_ptr(), s)
            assert rc == n, which.yf_images_last_error_text()

        def prep_yuv(i):
            b = bufs["nv12"][i % 2].data_ptr()
            if uniform:
                rc = lib.yf_images_prepare_yuv_device(b, yuv_bytes, images.YF_PIX_NV12, h0, w0, w0, h0 * w0, w0, yuv_fs, n, 56, frames.data_ptr(), s)
            else:
                rc = lib.yf_images_prepare_yuv_ragged_device(b, yuv_bytes, images.YF_PIX_NV12, d_yuv.data_ptr(), n, 56, frames.data_ptr(),
                                                             status.data_ptr(), s)
            assert rc == n, lib.yf_images_last_error_text()

        def full_bgr(i):
            b = bufs["bgr"][i % 2].data_ptr()
            if uniform:
                rc = lib.yf_images_run_decode_device(net.handle, b, bgr_bytes, 0, h0, w0, w0 * 3, bgr_fs, n, frames.data_ptr(), heads.data_ptr(), 0,
                                                     dets.data_ptr(), counts.data_ptr(), 147, s)
            else:
                rc = lib.yf_images_run_decode_ragged_device(net.handle, b, bgr_bytes, 0, d_bgr.data_ptr(), n, frames.data_ptr(), heads.data_ptr(),
                                                            0, dets.data_ptr(), counts.data_ptr(), 147, status.data_ptr(), s)
            assert rc == n, lib.yf_images_last_error_text()

        def full_yuv(i):
            prep_yuv(i)
            net.run_device(frames.data_ptr(), heads.data_ptr(), n, stream=s)
            rc = lib.yf_images_decode_ragged_device(heads.data_ptr(), d_bgr.data_ptr(), n, 0, dets.data_ptr(), counts.data_ptr(), 147, s)
            assert rc == n, lib.yf_images_last_error_text()

        lines = {"bgr": touched_lines(host, bgr), "nv12": touched_lines_yuv(host, yuv)}
        t = {"bgr": time(prep_bgr), "nv12": time(prep_yuv), "bgr again": time(prep_bgr)}
        if parent is not None:
            t["bgr parent"] = time(lambda i: prep_bgr(i, parent))
        full = {"bgr": time(full_bgr), "nv12": time(full_yuv)}
        print(f"{name}")
        for key, nbytes in (("nv12", yuv_bytes), ("bgr", bgr_bytes)):
            gbps = lines[key] / t[key] / 1e9
            print(f"  {key:5s} input {nbytes / 2**30:5.2f} GiB x2  touched {lines[key] / 1e9:6.3f} GB  prepare {t[key] * 1e6:8.1f} us = "
                  f"{n / t[key] / 1e6:6.2f} M img/s = {gbps:6.0f} GB/s ({100 * gbps / (HBM_TBPS * 1e3):4.1f} % of 6.3 TB/s)  "
                  f"prepare+network+decode {full[key] * 1e6:8.1f} us = {n / full[key] / 1e6:6.2f} M img/s")
        extra = f"  bgr prepare again {t['bgr again'] * 1e6:8.1f} us ({100 * (t['bgr again'] / t['bgr'] - 1):+5.2f} %)"
        if parent is not None:
            extra += f"   parent's bgr prepare {t['bgr parent'] * 1e6:8.1f} us ({100 * (t['bgr parent'] / t['bgr'] - 1):+5.2f} % against the first)"
        print(extra + f"   nv12 / bgr prepare time {t['nv12'] / t['bgr']:5.3f}", flush=True)
        del bufs
        torch.cuda.empty_cache()
    net.destroy()


if __name__ == "__main__":
    main()
