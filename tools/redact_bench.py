#!/usr/bin/env python3
"""Redaction on the GPU: what the two launches of yf_images_redact_records_device / _yuv_device cost (GPU TOOL; bench.py is not involved).
Device events around every call, warm-up first, the median of the timed calls, as tools/crops_bench.py does.  The mosaic is idempotent
and the fill writes constants, so repeated launches on the same pictures do identical work.

    real      4096 pictures of 410x362 with real content (the 27 real frames of tests/golden upscaled to that size, repeated), as BGR and
              as NV12 surfaces: the ragged run at 56x56 and the suppression at 0.4 on the BGR pictures leave the records (the surfaces
              have the same sides, so the same records serve them); then the mosaic at k = 8 and k = 32 and the fill, per call, beside
              the network call (yf_network_run_device over the 4096 frames) and the crop call (112x112 chips) on the same records in the
              same run.
    worst     every candidate of every frame firing, unsuppressed: 147 records per frame that overlap heavily, so nearly every workgroup
              walks a long list of earlier records.  The crop beside it cuts 16x16 chips (112x112 chips of 602 112 records do not fit).
    bandwidth the touched-lines model of tools/crops_bench.py: the distinct 128-byte lines that hold a byte of the redacted set (counted
              on every 64th picture, scaled), read and written once each by the mosaic and written once by the fill, against 6.3 TB/s.

    python tools/redact_bench.py [--iters 30] [--warmup 5] [--only real|worst]
"""
import argparse
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


def touched_lines(ptq, dets, counts, cap, offsets, pitch, bpp, block, rows=H, chroma=False):
    """bytes in the distinct 128-byte lines that hold a byte of the redacted set of planes at `offsets` (rows `pitch` apart, bpp bytes per
    pixel), on every 64th picture, scaled to the batch.  block 0: the regions themselves.  chroma: the half-resolution plane of a surface."""
    sample, total = range(0, len(offsets), 64), 0
    for i in sample:
        mask = np.zeros((rows, W * bpp if not chroma else W), bool)
        for d in dets[i, :min(max(int(counts[i]), 0), cap)]:
            r = ptq.crop_region((d["x1"], d["y1"], d["x2"], d["y2"]), W, H, 0, False)
            if r is None:
                continue
            x0, y0, x1, y1 = r[0], r[1], r[0] + r[2] - 1, r[1] + r[3] - 1
            if block:
                x0, y0, x1, y1 = x0 // block * block, y0 // block * block, x1 // block * block + block - 1, y1 // block * block + block - 1
            if chroma:
                mask[y0 >> 1:(y1 >> 1) + 1, (x0 >> 1) * 2:((x1 >> 1) + 1) * 2] = True
            else:
                mask[y0:y1 + 1, x0 * bpp:(x1 + 1) * bpp] = True
        ys, xs = np.nonzero(mask)
        total += np.unique((int(offsets[i]) + ys * pitch + xs) // 128).size * 128
    return total * len(offsets) / len(sample)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch
    from images_yuv_support import bgr_to_nv12
    yf = importlib.import_module("stm32h7-yolo_amd")
    images = importlib.import_module("stm32h7-yolo_amd.images")
    ptq = importlib.import_module("stm32h7-yolo_amd.ptq")
    binding = importlib.import_module("stm32h7-yolo_amd.binding")
    net = yf.Network(device=0).init()
    lib = images.load()
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    dev = "cuda"
    n, cap = 4096, 147
    print(f"# libyf_images build {(lib.yf_images_build_id() or b'').decode()}, network build {net.build_id}; {torch.cuda.get_device_name(0)}")
    print(f"# {args.iters} timed calls after {args.warmup} warm-up, median of per-call device events")

    def timed(*fns):
        """the medians (us) of the calls, timed in turn inside one loop"""
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
        return [float(np.median([row[k].elapsed_time(row[k + 1]) for row in ev])) * 1e3 for k in range(len(fns))]

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

    def report(name, out):
        torch.cuda.synchronize()
        counts = d_counts.cpu().numpy()
        dets = d_dets.cpu().numpy().view(binding.DET_DTYPE).reshape(n, cap)
        total = int(np.clip(counts, 0, cap).sum())
        d_chips = torch.empty((total, out, out, 3), dtype=torch.uint8, device=dev)
        d_info = torch.empty((total, 28), dtype=torch.uint8, device=dev)
        crop = lambda: images.crop_records_device(d_px.data_ptr(), nbytes, "bgr", d_desc.data_ptr(), d_dets.data_ptr(), d_counts.data_ptr(), n,
                                                  cap, out, out, d_chips.data_ptr(), total, d_first.data_ptr(), d_info.data_ptr(), stream=s)
        t_net, t_crop = timed(network, crop)
        print(f"{name:5s} {n} x {W}x{H}, {total} records (at most {int(counts.max())} per frame); network call {t_net:8.2f} us, "
              f"prefix + crop to {out}x{out} on the same records {t_crop:8.2f} us")
        del d_chips, d_info
        for yuv in (False, True):
            for label, mode, block in (("mosaic k = 8", "mosaic", 8), ("mosaic k = 32", "mosaic", 32), ("fill", "fill", 0)):
                t, = timed(redact(yuv, mode, block))
                if yuv:
                    lines = (touched_lines(ptq, dets, counts, cap, ydesc["offset_y"], W, 1, block)
                             + touched_lines(ptq, dets, counts, cap, ydesc["offset_uv"], W, 1, block, rows=H // 2, chroma=True))
                else:
                    lines = touched_lines(ptq, dets, counts, cap, desc["offset"], W * 3, 3, block)
                moved = lines * (1 if mode == "fill" else 2)
                print(f"{name:5s} {'NV12' if yuv else 'BGR ':4s} {label:13s} prefix + redact {t:8.2f} us = {100 * t / t_net:6.2f} % of the network "
                      f"call, {t / t_crop:5.2f} x the crop call; touched lines {lines / 1e6:7.2f} MB, "
                      f"{'written' if mode == 'fill' else 'read and written'}: {moved / (t * 1e-6) / 1e9:6.0f} GB/s "
                      f"({100 * moved / (t * 1e-6) / 1e12 / HBM_TBPS:4.1f} % of {HBM_TBPS} TB/s)")
        assert int(d_status.cpu().numpy().sum()) == 0 and int(d_first[n].item()) == total

    if not args.only or args.only == "real":
        images.run_decode_ragged_device(net, d_px.data_ptr(), nbytes, "bgr", d_desc.data_ptr(), n, d_frames.data_ptr(), d_heads.data_ptr(),
                                        d_dets.data_ptr(), d_counts.data_ptr(), cap, d_status.data_ptr(), stream=s)
        images.nms_device(d_dets.data_ptr(), d_counts.data_ptr(), n, cap, 0.4, stream=s)
        report("real", 112)
    if not args.only or args.only == "worst":
        h = np.random.default_rng(3).integers(-128, 128, (n, 7, 7, 18), dtype=np.int16)
        h[..., 4::6] = 120
        d_heads.copy_(torch.from_numpy(h.astype(np.int8)))
        net.decode_device(d_heads.data_ptr(), n, d_dets.data_ptr(), d_counts.data_ptr(), cap, w_scale=W / 56., h_scale=H / 56., stream=s)
        report("worst", 16)
    net.destroy()


if __name__ == "__main__":
    main()
