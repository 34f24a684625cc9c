#!/usr/bin/env python3
"""Drawing on the GPU: what the two launches of yf_images_draw_records_device / _yuv_device cost (GPU TOOL; bench.py is not involved).
Device events around every call, warm-up first, the median (and the least and the most) of the timed calls, the calls of a group timed in
turn inside one loop, as tools/redact_bench.py does.  The drawing writes constants, so repeated launches on the same pictures do identical
work.  Nothing is gated: there is no earlier number for a draw.  The yardsticks beside each figure, taken in the same run: the
redaction's fill on the same records (it writes the boxes' insides too) and the network launch.

    real      4096 pictures of 410x362 with real content (the 27 real frames of tests/golden upscaled to that size, repeated), as BGR and
              as NV12 surfaces: the ragged run at 56x56 and the suppression at 0.4 on the BGR pictures leave the records; then the draw at
              half 0, 1 and 3, in one colour and with keys (a uint32 per slot, stride 4, a palette of 16).
    worst     every candidate of every frame firing, unsuppressed: 147 records per frame that overlap heavily, so with keys nearly every
              workgroup lists up to 146 later records and every pixel is looked up in that list.
    hashes    with --parent-lib (a libyf_images.so built from the parent commit): tools/isa_hashes.py on it and on this build -- the
              kernels that existed before keep their instruction streams.  Needs no GPU: --only hashes.

    python tools/draw_bench.py [--iters 30] [--warmup 5] [--only real|worst|hashes] [--parent-lib PATH] [--out profiles/draw_bench.txt]
"""
import argparse
import hashlib
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 410, 362
COLOUR = 0x00C82D5A
HALVES = (0, 1, 3)


def hashes_statement(images, parent_lib):
    from tools import isa_hashes
    digest = lambda d: {k: hashlib.sha256("\n".join(v).encode()).hexdigest()[:16] for k, v in d.items()}
    res = {}
    old, new = digest(isa_hashes.disassemble(parent_lib)), digest(isa_hashes.disassemble(images.lib_path(), res))
    changed = sorted(k for k in old if new.get(k) != old[k])
    added = sorted(k for k in new if k not in old)
    lines = [f"hashes: {len(old) - len(changed)} of the {len(old)} kernels of the parent's libyf_images.so keep their instruction streams "
             f"(tools/isa_hashes.py on both builds); {len(added)} kernels beside them: {', '.join(added)}"]
    lines += [f"hashes: CHANGED {k}" for k in changed]
    for k in added:
        r = res[k]
        lines.append(f"resources: {k}: {r['vgpr_count']} VGPRs, {r['sgpr_count']} SGPRs ({r['sgpr_spill_count']} kept in VGPR lanes), "
                     f"{r['group_segment_fixed_size']} B LDS, {r['private_segment_fixed_size']} B scratch")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "draw_bench.txt"))
    args = ap.parse_args()
    images = importlib.import_module("stm32h7-yolo_amd.images")
    text = []

    def say(line):
        print(line, flush=True)
        text.append(line)

    if args.parent_lib:
        for line in hashes_statement(images, args.parent_lib):
            say(line)
    if args.only == "hashes":
        open(args.out, "w").write("\n".join(text) + "\n")
        return
    import torch
    from images_yuv_support import bgr_to_nv12
    yf = importlib.import_module("stm32h7-yolo_amd")
    ptq = importlib.import_module("stm32h7-yolo_amd.ptq")
    net = yf.Network(device=0).init()
    lib = images.load()
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    dev = "cuda"
    n, cap = 4096, 147
    say(f"# libyf_images build {(lib.yf_images_build_id() or b'').decode()}, network build {net.build_id}; {torch.cuda.get_device_name(0)}")
    say(f"# {args.iters} timed calls after {args.warmup} warm-up; per call the median [least .. most] of device events around both launches")

    rounds = {"iters": args.iters, "warmup": args.warmup}

    def timed(*fns):
        """(median, least, most) in us of each call, the calls timed in turn inside one loop"""
        for _ in range(rounds["warmup"]):
            for fn in fns:
                fn()
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(len(fns) + 1)] for _ in range(rounds["iters"])]
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
    rng = np.random.default_rng(7)
    d_keys = torch.from_numpy(rng.integers(0, 2 ** 31, (n, cap), dtype=np.int64).astype(np.int32)).to(dev)
    d_pal = torch.tensor([c[0] << 16 | c[1] << 8 | c[2] for c in images.TRACK_PALETTE], dtype=torch.int32).to(dev)
    images.set_decode_tables(*net.decode_tables())
    network = lambda: net.run_device(d_frames.data_ptr(), d_heads.data_ptr(), n, s)

    def batch(yuv):
        return ((images.draw_records_yuv_device, images.redact_records_yuv_device, d_ypx, ynbytes, d_ydesc, "nv12") if yuv else
                (images.draw_records_device, images.redact_records_device, d_px, nbytes, d_desc, "bgr"))

    def draw(yuv, half, keyed):
        fn, _, px, nb, dd, fmt = batch(yuv)
        kw = dict(d_keys=d_keys.data_ptr(), key_stride=4, d_palette=d_pal.data_ptr(), palette_n=16) if keyed else dict(colour=COLOUR)
        return lambda: fn(px.data_ptr(), nb, fmt, dd.data_ptr(), d_dets.data_ptr(), d_counts.data_ptr(), n, cap, d_first.data_ptr(),
                          d_status.data_ptr(), half=half, stream=s, **kw)

    def fill(yuv):
        _, fn, px, nb, dd, fmt = batch(yuv)
        return lambda: fn(px.data_ptr(), nb, fmt, dd.data_ptr(), d_dets.data_ptr(), d_counts.data_ptr(), n, cap, d_first.data_ptr(),
                          d_status.data_ptr(), mode="fill", block=0, colour=COLOUR, stream=s)

    def report(name):
        torch.cuda.synchronize()
        counts = d_counts.cpu().numpy()
        total = int(np.clip(counts, 0, cap).sum())
        (t_net, lo, hi), = timed(network)
        say(f"{name:5s} {n} x {W}x{H}, {total} records (at most {int(counts.max())} per frame); network launch {t_net:8.2f} us [{lo:.2f} .. {hi:.2f}]")
        for yuv in (False, True):
            calls = [fill(yuv)] + [draw(yuv, half, keyed) for keyed in (False, True) for half in HALVES]
            labels = ["fill (the redaction's)"] + [f"draw half {half} {'keys' if keyed else 'one colour'}" for keyed in (False, True) for half in HALVES]
            times = timed(*calls)
            t_fill = times[0][0]
            for label, (t, lo, hi) in zip(labels, times):
                say(f"{name:5s} {'NV12' if yuv else 'BGR ':4s} {label:24s} {t:9.2f} us [{lo:9.2f} .. {hi:9.2f}] = {100 * t / t_net:8.2f} % of the network "
                    f"launch, {t / t_fill:5.2f} x the fill")
        assert int(d_status.cpu().numpy().sum()) == 0 and int(d_first[n].item()) == total

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
        rounds["iters"], rounds["warmup"] = max(5, args.iters // 3), min(args.warmup, 2)      # its calls take milliseconds
        say(f"# worst: {rounds['iters']} timed calls after {rounds['warmup']} warm-up")
        report("worst")
    net.destroy()
    open(args.out, "w").write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
