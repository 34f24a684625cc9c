#!/usr/bin/env python3
"""Area-averaged frames against the linear prepare of libyf_images on the same pictures, in one run (GPU TOOL; bench.py is not involved).
The method is that of tools/fit_bench.py: device events around every launch, warm-up first, the median of the timed launches, inputs
rotating over two buffers per workload.  The paths are timed interleaved -- linear, area, (the parent commit's linear,) linear again,
area again -- so the linear prepare's own run-to-run spread stands beside every ratio.

Workloads, at 56 and at 160: 4096 pictures of 410x362 BGR, 1024 of 1920x1080 BGR, 1024 of 1920x1080 NV12, and a ragged 4096 of the 27
reference sizes (BGR).  Per workload: the prepare alone (yf_images_prepare_ragged_device / _yuv_ragged_device against
yf_images_prepare_area_ragged_device / _area_yuv_ragged_device, stretch) and images -> boxes (linear: the run_decode entries, NV12:
prepare, network, decode; area: prepare, network, decode -- three launches).

For each prepare the share of 6.3 TB/s (the figure profiles/images_bench.txt uses) is reported on ALL source bytes plus the frame bytes:
the bytes the area prepare has to read.  The linear prepare reads a small part of them (four source pixels per output pixel), so its
"share" on that count can exceed what its loads move and is printed only to put both on one scale; the ratio of times is expected to be
well above 1 and is no regression of anything.  Nothing here is gated.

With --parent-lib the parent commit's libyf_images.so is loaded beside this build's and its linear prepare is timed in the same
interleaving; then the instruction-hash comparison of every kernel the parent's library has, and the static figures of the new kernels.

    python tools/area_bench.py [--iters 20] [--warmup 5] [--only NAME] [--parent-lib PATH/libyf_images.so]
"""
import argparse
import ctypes
import hashlib
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from fit_bench import workloads          # noqa: E402
import isa_hashes                        # noqa: E402

HBM = 6.3e12


def static_figures(lib_path, parent_path):
    res = {}
    mine = isa_hashes.disassemble(lib_path, res)
    print("\n# static figures (tools/isa_hashes.py): VGPRs, SGPRs, LDS bytes, scratch bytes, SGPR + VGPR spills")
    for k in sorted(res):
        if "yfarea" in k:
            r = res[k]
            print(f"  {k.replace('_ZN6yfarea11', 'yfarea::'):50s} {r['vgpr_count']:3d} {r['sgpr_count']:3d} {r['group_segment_fixed_size']:6d} "
                  f"{r['private_segment_fixed_size']:2d} {r['sgpr_spill_count'] + r['vgpr_spill_count']:2d}")
    if parent_path:
        digest = lambda body: hashlib.sha256("\n".join(body).encode()).hexdigest()[:16]
        theirs = isa_hashes.disassemble(parent_path)
        same = [k for k in theirs if k in mine and digest(mine[k]) == digest(theirs[k])]
        moved = sorted(set(theirs) - set(same))
        print(f"\n# instruction hashes: {len(same)} of the parent library's {len(theirs)} functions are instruction for instruction the same in "
              f"this build; {len(set(mine) - set(theirs))} functions are new" + ("".join("\n#   CHANGED or missing: " + k for k in moved)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--parent-lib", default="", help="the parent commit's libyf_images.so: its linear prepare in the same run, and the hash comparison")
    args = ap.parse_args()
    import torch
    yf = importlib.import_module("stm32h7-yolo_amd")
    images = importlib.import_module("stm32h7-yolo_amd.images")
    net = yf.Network(device=0).init()
    lib = images.load()
    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        for name in ("prepare_ragged_device", "prepare_yuv_ragged_device"):
            fn = getattr(parent, "yf_images_" + name)
            fn.restype, fn.argtypes = ctypes.c_long, getattr(lib, "yf_images_" + name).argtypes
        parent.yf_images_build_id.restype = ctypes.c_char_p
    images.set_decode_tables(*net.decode_tables())
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    print(f"# libyf_images build {(lib.yf_images_build_id() or b'').decode()}"
          + (f" (parent library: build {(parent.yf_images_build_id() or b'').decode()})" if parent else "")
          + f", network build {net.build_id}; {torch.cuda.get_device_name(0)}")
    print(f"# {args.iters} timed launches after {args.warmup} warm-up, median of per-launch device events; inputs rotate over 2 buffers; "
          f"order: linear, area{', parent linear' if parent else ''}, linear again, area again.  share: (all source bytes + frame bytes) / "
          f"time / 6.3 TB/s.  Nothing is gated.")

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

    def rounds(linear, area, old=None, nbytes=None):
        t = {"lin": time(linear), "area": time(area)}
        if old is not None:
            t["old"] = time(old)
        t["lin2"], t["area2"] = time(linear), time(area)
        lin, ar = min(t["lin"], t["lin2"]), min(t["area"], t["area2"])
        text = (f"linear {t['lin'] * 1e6:9.1f} us  area {t['area'] * 1e6:9.1f} us  linear again {t['lin2'] * 1e6:9.1f} us "
                f"({100 * (t['lin2'] / t['lin'] - 1):+5.2f} %)  area again {t['area2'] * 1e6:9.1f} us  area / linear {ar / lin:6.2f}")
        if old is not None:
            text += f"  parent linear {t['old'] * 1e6:9.1f} us ({100 * (lin / t['old'] - 1):+5.2f} % this build against it)"
        if nbytes is not None:
            text += f"  share of 6.3 TB/s: area {100 * nbytes / ar / HBM:5.1f} %, linear on the same count {100 * nbytes / lin / HBM:6.1f} %"
        return text

    for name, dims, fmt in workloads():
        if args.only and args.only not in name:
            continue
        n, yuv = len(dims), fmt == "nv12"
        hs, ws = np.array([d[0] for d in dims], np.int64), np.array([d[1] for d in dims], np.int64)
        sizes = hs * ws * 3 // 2 if yuv else hs * ws * 3
        offs = np.concatenate([[0], np.cumsum((sizes + 15) // 16 * 16)[:-1]])
        nbytes, source = int(offs[-1] + sizes[-1]), int(sizes.sum())
        sides = np.zeros(n, images.IMAGE_DTYPE)                     # what the decodes read
        sides["offset"], sides["height"], sides["width"], sides["row_stride"] = offs, hs, ws, ws * 3
        if yuv:
            desc = np.zeros(n, images.YUV_IMAGE_DTYPE)
            desc["offset_y"], desc["offset_uv"], desc["height"], desc["width"], desc["stride_y"], desc["stride_uv"] = offs, offs + hs * ws, hs, ws, ws, ws
        else:
            desc = sides
        bufs = [torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda") for _ in range(2)]
        d_desc, d_sides = torch.from_numpy(desc.view(np.uint8).copy()).cuda(), torch.from_numpy(sides.view(np.uint8).copy()).cuda()
        counts = torch.empty(n, dtype=torch.int32, device="cuda")
        status = torch.empty(n, dtype=torch.int32, device="cuda")
        print(f"{name}  ({nbytes / 2**30:.2f} GiB x2; {source / 1e9:.3f} GB of source pixels)")
        for S in (56, 160):
            grid, cap = S // 8, 3 * (S // 8) ** 2
            frames = torch.empty((n, S, S, 3), dtype=torch.int8, device="cuda")
            heads = torch.empty((n, grid, grid, 18), dtype=torch.int8, device="cuda")
            dets = torch.empty((n, cap, 28), dtype=torch.uint8, device="cuda")
            px = lambda i: bufs[i % 2].data_ptr()
            code = images.format_code(fmt)
            tail = (frames.data_ptr(), status.data_ptr(), s)
            moved = source + n * S * S * 3

            def check(rc, of=lib):
                assert rc == n, of.yf_images_last_error_text()

            entry = "yf_images_prepare_yuv_ragged_device" if yuv else "yf_images_prepare_ragged_device"
            area_entry = lib.yf_images_prepare_area_yuv_ragged_device if yuv else lib.yf_images_prepare_area_ragged_device
            prep = lambda i: check(getattr(lib, entry)(px(i), nbytes, code, d_desc.data_ptr(), n, S, *tail))
            prep_old = (lambda i: check(getattr(parent, entry)(px(i), nbytes, code, d_desc.data_ptr(), n, S, *tail), parent)) if parent else None
            prep_area = lambda i: check(area_entry(px(i), nbytes, code, d_desc.data_ptr(), n, S, 0, 114, *tail))
            run_net = (lambda: net.run_device(frames.data_ptr(), heads.data_ptr(), n, stream=s)) if S == 56 else \
                      (lambda: net.run_device_hw(S, S, frames.data_ptr(), heads.data_ptr(), n, stream=s))
            out = (dets.data_ptr(), counts.data_ptr(), cap, s)
            if S == 56:
                dec = lambda i: check(lib.yf_images_decode_ragged_device(heads.data_ptr(), d_sides.data_ptr(), n, 0, *out))
            else:
                dec = lambda i: check(lib.yf_images_decode160_ragged_device(heads.data_ptr(), d_sides.data_ptr(), None, n, *out))

            def chain(i):
                if yuv:
                    prep(i), run_net(), dec(i)
                elif S == 56:
                    check(lib.yf_images_run_decode_ragged_device(net.handle, px(i), nbytes, code, d_desc.data_ptr(), n, frames.data_ptr(),
                                                                 heads.data_ptr(), 0, dets.data_ptr(), counts.data_ptr(), cap, status.data_ptr(), s))
                else:
                    check(lib.yf_images_run_decode160_ragged_device(net.handle, px(i), nbytes, code, d_desc.data_ptr(), n, frames.data_ptr(),
                                                                    heads.data_ptr(), dets.data_ptr(), counts.data_ptr(), cap, status.data_ptr(), s))

            def chain_area(i):
                prep_area(i), run_net(), dec(i)

            print(f"  {S:3d} prepare ({images.area_bands(n, S)} band(s) per frame)  {rounds(prep, prep_area, prep_old, moved)}")
            print(f"  {S:3d} images -> boxes  {rounds(chain, chain_area)}", flush=True)
            del frames, heads, dets
        del bufs
        torch.cuda.empty_cache()

    net.destroy()
    static_figures(images.lib_path(), args.parent_lib)


if __name__ == "__main__":
    main()
