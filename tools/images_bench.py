#!/usr/bin/env python3
"""Rate of libyf_images on the GPU (GPU TOOL; bench.py is not involved): images -> frames alone (prepare) and images -> frames -> heads -> records
(prepare + network + decode), in images/s, for four workloads:
    4096 images of 410x362 BGR (the reference dataset's size), 4096 of 640x480, 1024 of 1920x1080, and a ragged 4096 of the 27 reference sizes.
Device events around every launch, warm-up first, at least 50 timed launches, inputs rotating over two buffers per workload (each larger than
256 MiB, so the Infinity Cache does not hold them).  Bandwidth is quoted against a touched-lines model: the distinct 128-byte lines the bytes
a frame samples (two source rows per output row, two columns per output column, three channels) fall in, computed per image from the tap
tables (not FETCH_SIZE, which under-counts on gfx950).  Kernel times: run this under `rocprofv3 --kernel-trace --stats` in a run of its own.

    python tools/images_bench.py [--iters 60] [--warmup 10] [--only NAME]
"""
import argparse
import ctypes
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REF_SIZES = [(410, 362), (389, 450), (410, 356), (299, 410), (331, 410), (327, 410), (410, 391), (410, 330), (301, 410), (410, 450),
             (410, 283), (410, 281), (274, 410), (282, 410), (406, 450), (410, 312), (327, 410), (410, 273), (410, 295), (410, 297),
             (305, 409), (410, 344), (306, 450), (278, 410), (410, 301), (253, 409), (410, 295)]       # (width, height)
HBM_TBPS = 6.3


def taps(host, n_in, out=56):
    t = (ctypes.c_int32 * 4)()
    s = np.empty((out, 2), np.int64)
    for d in range(out):
        host.yfi_tap_host(d, out, n_in, t)
        s[d] = (t[0], t[1])
    return s


def touched_lines(host, desc, C=3):
    """distinct 128-byte lines read per batch (sum over images), from each image's tap tables and its own byte offset"""
    cache, total = {}, 0
    for off, h, w, rs in zip(desc["offset"].tolist(), desc["height"].tolist(), desc["width"].tolist(), desc["row_stride"].tolist()):
        key = (h, w)
        if key not in cache:
            rows = np.unique(taps(host, h).reshape(-1))
            cols = np.unique((taps(host, w).reshape(-1)[:, None] * C + np.arange(3)[None, :]).reshape(-1))
            cache[key] = (rows, cols)
        rows, cols = cache[key]
        addr = off + rows[:, None] * rs + cols[None, :]
        total += np.unique(addr // 128).size
    return total * 128


def workloads():
    yield "uniform 4096 x 410x362", [(362, 410)] * 4096, True
    yield "uniform 4096 x 640x480", [(480, 640)] * 4096, True
    yield "uniform 1024 x 1920x1080", [(1080, 1920)] * 1024, True
    yield "ragged 4096 x 27 reference sizes", [(h, w) for (w, h) in REF_SIZES] * (4096 // 27) + [(h, w) for (w, h) in REF_SIZES[:4096 % 27]], False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    import torch
    yf = importlib.import_module("stm32h7-yolo_amd")
    images = importlib.import_module("stm32h7-yolo_amd.images")
    net = yf.Network(device=0).init()
    lib = images.load()
    host = importlib.import_module("stm32h7-yolo_amd.libs").host_library("libyf_images_host.so")
    host.yfi_tap_host.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    print(f"# libyf_images build {(lib.yf_images_build_id() or b'').decode()}, network build {net.build_id}; {torch.cuda.get_device_name(0)}")
    print(f"# {args.iters} timed launches after {args.warmup} warm-up, median of per-launch device events; inputs rotate over 2 buffers")
    for name, dims, uniform in workloads():
        if args.only and args.only not in name:
            continue
        n = len(dims)
        desc = np.zeros(n, images.IMAGE_DTYPE)
        sizes = np.array([h * w * 3 for h, w in dims], np.int64)
        offs = np.concatenate([[0], np.cumsum((sizes + 15) // 16 * 16)[:-1]])
        desc["offset"], desc["height"], desc["width"] = offs, [d[0] for d in dims], [d[1] for d in dims]
        desc["row_stride"] = [d[1] * 3 for d in dims]
        nbytes = int(offs[-1] + sizes[-1])
        bufs = [torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda") for _ in range(2)]
        d_desc = torch.from_numpy(desc.view(np.uint8).copy()).cuda()
        frames = torch.empty((n, 56, 56, 3), dtype=torch.int8, device="cuda")
        heads = torch.empty((n, 7, 7, 18), dtype=torch.int8, device="cuda")
        dets = torch.empty((n, 147, 28), dtype=torch.uint8, device="cuda")
        counts = torch.empty(n, dtype=torch.int32, device="cuda")
        status = torch.empty(n, dtype=torch.int32, device="cuda")
        h0, w0 = dims[0]
        fs = int(offs[1]) if n > 1 else 0

        def prep(i):
            b = bufs[i % 2].data_ptr()
            if uniform:
                rc = lib.yf_images_prepare_device(b, nbytes, 0, h0, w0, w0 * 3, fs, n, 56, frames.data_ptr(), s)
            else:
                rc = lib.yf_images_prepare_ragged_device(b, nbytes, 0, d_desc.data_ptr(), n, 56, frames.data_ptr(), status.data_ptr(), s)
            assert rc == n, lib.yf_images_last_error_text()

        def full(i):
            b = bufs[i % 2].data_ptr()
            if uniform:
                rc = lib.yf_images_run_decode_device(net.handle, b, nbytes, 0, h0, w0, w0 * 3, fs, n, frames.data_ptr(), heads.data_ptr(), 0,
                                                     dets.data_ptr(), counts.data_ptr(), 147, s)
            else:
                rc = lib.yf_images_run_decode_ragged_device(net.handle, b, nbytes, 0, d_desc.data_ptr(), n, frames.data_ptr(), heads.data_ptr(),
                                                            0, dets.data_ptr(), counts.data_ptr(), 147, status.data_ptr(), s)
            assert rc == n, lib.yf_images_last_error_text()

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

        lines = [touched_lines(host, desc if not uniform else np.array([(i * fs, h0, w0, w0 * 3) for i in range(n)], images.IMAGE_DTYPE))]
        t_prep, t_full = time(prep), time(full)
        gbps = lines[0] / t_prep / 1e9
        print(f"{name:36s} input {nbytes / 2**30:5.2f} GiB x2  touched {lines[0] / 1e9:5.3f} GB  "
              f"prepare {t_prep * 1e6:8.1f} us = {n / t_prep / 1e6:6.2f} M img/s = {gbps:6.0f} GB/s ({100 * gbps / (HBM_TBPS * 1e3):4.1f} % of 6.3 TB/s)  "
              f"prepare+network+decode {t_full * 1e6:8.1f} us = {n / t_full / 1e6:6.2f} M img/s")
        del bufs
        torch.cuda.empty_cache()
    net.destroy()


if __name__ == "__main__":
    main()
