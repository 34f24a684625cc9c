#!/usr/bin/env python3
"""Letterboxed frames against the plain (stretching) path of libyf_images on the same pictures, in one run (GPU TOOL; bench.py is not
involved).  The method is that of tools/images_bench.py and tools/images_yuv_bench.py: device events around every launch, warm-up first,
the median of the timed launches, inputs rotating over two buffers per workload.  The two paths are timed interleaved -- plain, fit, plain
again, fit again -- so the plain prepare's own run-to-run spread stands beside the ratio.

Workloads, at 56 and at 160: 4096 pictures of 410x362 BGR, 1024 of 1920x1080 BGR, 1024 of 1920x1080 NV12, and a ragged 4096 of the 27
reference sizes (BGR).  Per workload: the prepare alone (yf_images_prepare_ragged_device / _yuv_ragged_device against
yf_images_prepare_fit_ragged_device / _fit_yuv_ragged_device), the decode alone on the heads the network gave (the ragged decode of that
size against yf_images_decode_fit_ragged_device) and images -> boxes (the run_decode entries; NV12: prepare, yf_network_run_device[_hw],
decode -- three launches either way).

Then the static figures of the new kernels beside the plain ones (tools/isa_hashes.py), with --parent-lib the instruction-hash
comparison of every kernel the parent's library has, and the number of suppressed records `detect` reports on the 27 real pictures
under both preprocessings -- an observation, no accuracy claim: those pictures are 56x56 frames scaled up and carry no labels.

    python tools/fit_bench.py [--iters 40] [--warmup 8] [--only NAME] [--parent-lib PATH/libyf_images.so]
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from images_bench import REF_SIZES          # noqa: E402
import isa_hashes                            # noqa: E402


def workloads():
    ref = [(h, w) for (w, h) in REF_SIZES]
    yield "4096 x 410x362 bgr", [(362, 410)] * 4096, "bgr"
    yield "1024 x 1920x1080 bgr", [(1080, 1920)] * 1024, "bgr"
    yield "1024 x 1920x1080 nv12", [(1080, 1920)] * 1024, "nv12"
    yield "ragged 4096 x 27 reference sizes bgr", ref * (4096 // 27) + ref[:4096 % 27], "bgr"


def real_pictures(ptq):
    """the 27 real frames scaled up to the reference sizes, BGR (tests/images_support.real_images)"""
    real = np.fromfile(os.path.join(ROOT, "tests", "golden", "real_frames_56.bin"), np.int8).reshape(-1, 56, 56, 3)
    rgb56 = (real.astype(np.int16) + 128).astype(np.uint8)
    return [np.ascontiguousarray(ptq.resize_linear_u8(rgb56[i], w, h)[..., ::-1]) for i, (w, h) in enumerate(REF_SIZES)]


def static_figures(lib_path, parent_path):
    res = {}
    mine = isa_hashes.disassemble(lib_path, res)
    print("\n# static figures (tools/isa_hashes.py): VGPRs, SGPRs, LDS bytes, scratch bytes")
    short = lambda k: k.replace("_ZN5yffit", "yffit::").replace("_ZN12_GLOBAL__N_1", "")
    for k in sorted(res):
        if "yffit" in k or ("prepare" in k and k.endswith(("ELb1EEEvNS_8PrepArgsE", "ELb1EEEvNS_7YuvArgsE"))):
            r = res[k]
            print(f"  {short(k):70s} {r['vgpr_count']:3d} {r['sgpr_count']:3d} {r['group_segment_fixed_size']:6d} {r['private_segment_fixed_size']:2d}")
    if parent_path:
        import hashlib
        digest = lambda body: hashlib.sha256("\n".join(body).encode()).hexdigest()[:16]
        theirs = isa_hashes.disassemble(parent_path)
        same = [k for k in theirs if k in mine and digest(mine[k]) == digest(theirs[k])]
        moved = sorted(set(theirs) - set(same))
        print(f"\n# instruction hashes: {len(same)} of the parent library's {len(theirs)} functions are instruction for instruction the same in "
              f"this build; {len(set(mine) - set(theirs))} functions are new" + ("".join("\n#   CHANGED or missing: " + k for k in moved)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--only", default="")
    ap.add_argument("--parent-lib", default="", help="the parent commit's libyf_images.so, for the instruction-hash comparison")
    args = ap.parse_args()
    import torch
    yf = importlib.import_module("stm32h7-yolo_amd")
    images = importlib.import_module("stm32h7-yolo_amd.images")
    ptq = importlib.import_module("stm32h7-yolo_amd.ptq")
    net = yf.Network(device=0).init()
    lib = images.load()
    images.set_decode_tables(*net.decode_tables())
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    print(f"# libyf_images build {(lib.yf_images_build_id() or b'').decode()}, network build {net.build_id}; {torch.cuda.get_device_name(0)}")
    print(f"# {args.iters} timed launches after {args.warmup} warm-up, median of per-launch device events; inputs rotate over 2 buffers; "
          f"order: plain, fit, plain again, fit again")

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

    def four(plain, fit):
        t = [time(plain), time(fit), time(plain), time(fit)]
        return (f"plain {t[0] * 1e6:8.1f} us  fit {t[1] * 1e6:8.1f} us  plain again {t[2] * 1e6:8.1f} us ({100 * (t[2] / t[0] - 1):+5.2f} %)  "
                f"fit again {t[3] * 1e6:8.1f} us  fit / plain {min(t[1], t[3]) / min(t[0], t[2]):5.3f}")

    for name, dims, fmt in workloads():
        if args.only and args.only not in name:
            continue
        n, yuv = len(dims), fmt == "nv12"
        hs, ws = np.array([d[0] for d in dims], np.int64), np.array([d[1] for d in dims], np.int64)
        sizes = hs * ws * 3 // 2 if yuv else hs * ws * 3
        offs = np.concatenate([[0], np.cumsum((sizes + 15) // 16 * 16)[:-1]])
        nbytes = int(offs[-1] + sizes[-1])
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
        print(f"{name}  ({nbytes / 2**30:.2f} GiB x2)")
        for S in (56, 160):
            grid, cap = S // 8, 3 * (S // 8) ** 2
            frames = torch.empty((n, S, S, 3), dtype=torch.int8, device="cuda")
            heads = torch.empty((n, grid, grid, 18), dtype=torch.int8, device="cuda")
            dets = torch.empty((n, cap, 28), dtype=torch.uint8, device="cuda")
            px = lambda i: bufs[i % 2].data_ptr()
            code = images.format_code(fmt)
            tail = (frames.data_ptr(), status.data_ptr(), s)

            def check(rc):
                assert rc == n, lib.yf_images_last_error_text()

            if yuv:
                prep = lambda i: check(lib.yf_images_prepare_yuv_ragged_device(px(i), nbytes, code, d_desc.data_ptr(), n, S, *tail))
                prep_fit = lambda i: check(lib.yf_images_prepare_fit_yuv_ragged_device(px(i), nbytes, code, d_desc.data_ptr(), n, S, 114, *tail))
            else:
                prep = lambda i: check(lib.yf_images_prepare_ragged_device(px(i), nbytes, code, d_desc.data_ptr(), n, S, *tail))
                prep_fit = lambda i: check(lib.yf_images_prepare_fit_ragged_device(px(i), nbytes, code, d_desc.data_ptr(), n, S, 114, *tail))
            run_net = (lambda: net.run_device(frames.data_ptr(), heads.data_ptr(), n, stream=s)) if S == 56 else \
                      (lambda: net.run_device_hw(S, S, frames.data_ptr(), heads.data_ptr(), n, stream=s))
            out = (dets.data_ptr(), counts.data_ptr(), cap, s)
            if S == 56:
                dec = lambda i: check(lib.yf_images_decode_ragged_device(heads.data_ptr(), d_sides.data_ptr(), n, 0, *out))
            else:
                dec = lambda i: check(lib.yf_images_decode160_ragged_device(heads.data_ptr(), d_sides.data_ptr(), None, n, *out))
            dec_fit = lambda i: check(lib.yf_images_decode_fit_ragged_device(heads.data_ptr(), d_sides.data_ptr(), None, n, S, *out))

            def chain(i):
                if yuv:
                    prep(i), run_net(), dec(i)
                elif S == 56:
                    check(lib.yf_images_run_decode_ragged_device(net.handle, px(i), nbytes, code, d_desc.data_ptr(), n, frames.data_ptr(),
                                                                 heads.data_ptr(), 0, dets.data_ptr(), counts.data_ptr(), cap, status.data_ptr(), s))
                else:
                    check(lib.yf_images_run_decode160_ragged_device(net.handle, px(i), nbytes, code, d_desc.data_ptr(), n, frames.data_ptr(),
                                                                    heads.data_ptr(), dets.data_ptr(), counts.data_ptr(), cap, status.data_ptr(), s))

            def chain_fit(i):
                if yuv:
                    prep_fit(i), run_net(), dec_fit(i)
                else:
                    check(lib.yf_images_run_decode_fit_ragged_device(net.handle, px(i), nbytes, code, d_desc.data_ptr(), n, S, 114, frames.data_ptr(),
                                                                     heads.data_ptr(), dets.data_ptr(), counts.data_ptr(), cap, status.data_ptr(), s))

            print(f"  {S:3d} prepare         {four(prep, prep_fit)}")
            prep(0), run_net()                                       # heads of real frames' worth of noise for the decodes
            print(f"  {S:3d} decode          {four(dec, dec_fit)}")
            print(f"  {S:3d} images -> boxes {four(chain, chain_fit)}", flush=True)
            del frames, heads, dets
        del bufs
        torch.cuda.empty_cache()

    if not args.only:
        pictures = real_pictures(ptq)
        print("\n# suppressed records (iou 0.4) `detect` reports on the 27 real pictures: an observation, not an accuracy claim")
        for S in (56, 160):
            kept = {fit: sum(b.shape[0] for b in images.detect(net, pictures, "bgr", iou_threshold=0.4, size=S, fit=fit)) for fit in images.FITS}
            print(f"  {S:3d}: stretch {kept['stretch']}, letterbox {kept['letterbox']}")
    net.destroy()
    static_figures(images.lib_path(), args.parent_lib)


if __name__ == "__main__":
    main()
