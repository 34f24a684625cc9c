#!/usr/bin/env python3
"""Face chips on the GPU: what the two launches of yf_images_crop_records_device cost (GPU TOOL; bench.py is not involved).  Device events
around every call, warm-up first, the median of the timed calls, as tools/images_bench.py and tools/tiles_bench.py do.

    real      4096 pictures of 410x362 BGR with real content (the 27 real frames of tests/golden upscaled to that size, repeated): the ragged
              run at 56x56 and the suppression at 0.4 leave the records; then prefix + crop at 112x112 per call, and the same time as a
              share of the network call (yf_network_run_device over the 4096 frames) in the same run.
    prepare   the yardstick of the kernel: 1024 pictures of 410x362 BGR (random bytes, two buffers in turn, each above 256 MiB), one record
              per frame whose region is the whole picture, chips of 160x160 -- the source reads and the output bytes of
              yf_images_prepare_ragged_device(out_hw = 160) on the same pictures.  The two are timed interleaved, call by call.
    bandwidth the achieved share of 6.3 TB/s on the touched-lines model of tools/images_bench.py (the distinct 128-byte lines the sampled
              bytes fall in) for `prepare`, and for an up-scaling case: eight 40x40 regions per picture of the 4096 -> 112x112, where the
              chip bytes written are several times the lines read.

    python tools/crops_bench.py [--iters 30] [--warmup 5] [--only real|prepare|upscale]
"""
import argparse
import ctypes
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 410, 362
HBM_TBPS = 6.3


def region_lines(taps, host, offs, rs, x0, y0, w, h, out_w, out_h):
    """distinct 128-byte lines the chips of the regions (x0, y0, w, h) of packed 3-byte pictures at byte offsets `offs` sample"""
    rows = np.unique(taps(host, h, out_h).reshape(-1)) + y0
    cols = np.unique(((taps(host, w, out_w).reshape(-1) + x0)[:, None] * 3 + np.arange(3)[None, :]).reshape(-1))
    rel = (rows[:, None] * rs + cols[None, :]).reshape(-1)
    return sum(np.unique((int(o) + rel) // 128).size for o in offs) * 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch
    from tools.images_bench import taps
    yf = importlib.import_module("stm32h7-yolo_amd")
    images = importlib.import_module("stm32h7-yolo_amd.images")
    ptq = importlib.import_module("stm32h7-yolo_amd.ptq")
    binding = importlib.import_module("stm32h7-yolo_amd.binding")
    net = yf.Network(device=0).init()
    lib = images.load()
    host = importlib.import_module("stm32h7-yolo_amd.libs").host_library("libyf_images_host.so")
    host.yfi_tap_host.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    dev = "cuda"
    print(f"# libyf_images build {(lib.yf_images_build_id() or b'').decode()}, network build {net.build_id}; {torch.cuda.get_device_name(0)}")
    print(f"# {args.iters} timed calls after {args.warmup} warm-up, median of per-call device events")

    def timed(*fns):
        """the medians (us) of the calls, timed in turn inside one loop"""
        for i in range(args.warmup):
            for fn in fns:
                fn(i)
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(len(fns) + 1)] for _ in range(args.iters)]
        for i, row in enumerate(ev):
            row[0].record(stream)
            for k, fn in enumerate(fns):
                fn(i)
                row[k + 1].record(stream)
        torch.cuda.synchronize()
        return [float(np.median([row[k].elapsed_time(row[k + 1]) for row in ev])) * 1e3 for k in range(len(fns))]

    def descriptors(n):
        desc = np.zeros(n, images.IMAGE_DTYPE)
        size = (H * W * 3 + 15) // 16 * 16
        desc["offset"], desc["height"], desc["width"], desc["row_stride"] = np.arange(n, dtype=np.int64) * size, H, W, W * 3
        return desc, int(desc["offset"][-1]) + H * W * 3

    def crop_call(d_px, nbytes, d_desc, d_dets, d_counts, n, cap, out, d_chips, room, d_first, d_info):
        return lambda i: images.crop_records_device(d_px[i % len(d_px)].data_ptr(), nbytes, "bgr", d_desc.data_ptr(), d_dets.data_ptr(),
                                                    d_counts.data_ptr(), n, cap, out, out, d_chips.data_ptr(), room, d_first.data_ptr(),
                                                    d_info.data_ptr(), stream=s)

    if not args.only or args.only == "real":
        n, cap, out = 4096, 147, 112
        real = np.fromfile(os.path.join(ROOT, "tests", "golden", "real_frames_56.bin"), np.int8).reshape(-1, 56, 56, 3)
        rgb56 = (real.astype(np.int16) + 128).astype(np.uint8)
        photos = [np.ascontiguousarray(ptq.resize_linear_u8(f, W, H)[..., ::-1]) for f in rgb56]
        desc, nbytes = descriptors(n)
        buf = np.zeros(nbytes, np.uint8)
        for i in range(n):
            o = int(desc["offset"][i])
            buf[o:o + H * W * 3] = photos[i % len(photos)].reshape(-1)
        d_px, d_desc = torch.from_numpy(buf).to(dev), torch.from_numpy(desc.view(np.uint8)).to(dev)
        d_frames = torch.empty((n, 56, 56, 3), dtype=torch.int8, device=dev)
        d_heads = torch.empty((n, 7, 7, 18), dtype=torch.int8, device=dev)
        d_dets = torch.empty((n, cap, 28), dtype=torch.uint8, device=dev)
        d_counts = torch.empty(n, dtype=torch.int32, device=dev)
        d_status = torch.empty(n, dtype=torch.int32, device=dev)
        images.set_decode_tables(*net.decode_tables())
        images.run_decode_ragged_device(net, d_px.data_ptr(), nbytes, "bgr", d_desc.data_ptr(), n, d_frames.data_ptr(), d_heads.data_ptr(),
                                        d_dets.data_ptr(), d_counts.data_ptr(), cap, d_status.data_ptr(), stream=s)
        images.nms_device(d_dets.data_ptr(), d_counts.data_ptr(), n, cap, 0.4, stream=s)
        torch.cuda.synchronize()
        total = int(np.clip(d_counts.cpu().numpy(), 0, cap).sum())
        d_chips = torch.empty((total, out, out, 3), dtype=torch.uint8, device=dev)
        d_info = torch.empty((total, 28), dtype=torch.uint8, device=dev)
        d_first = torch.empty(n + 1, dtype=torch.int32, device=dev)
        crop = crop_call([d_px], nbytes, d_desc, d_dets, d_counts, n, cap, out, d_chips, total, d_first, d_info)
        network = lambda i: net.run_device(d_frames.data_ptr(), d_heads.data_ptr(), n, s)
        t_crop, t_net = timed(crop, network)
        info = d_info.cpu().numpy().view(images.CHIP_DTYPE).reshape(-1)
        print(f"real    {n} x {W}x{H} BGR, {total} boxes after suppression ({int((info['status'] == 0).sum())} with a region, mean region "
              f"{float(info['width'].mean()):.0f}x{float(info['height'].mean()):.0f}) -> {out}x{out}")
        print(f"real    prefix + crop {t_crop:8.2f} us = {100 * t_crop / t_net:5.2f} % of the network call ({t_net:8.2f} us, same run)")
        del d_px, d_chips, d_frames
        torch.cuda.empty_cache()

    if not args.only or args.only == "prepare":
        n, cap, out = 1024, 1, 160
        desc, nbytes = descriptors(n)
        bufs = [torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device=dev) for _ in range(2)]
        d_desc = torch.from_numpy(desc.view(np.uint8)).to(dev)
        dets = np.zeros((n, cap), binding.DET_DTYPE)
        dets["x2"], dets["y2"] = W - 1, H - 1
        d_dets = torch.from_numpy(dets.view(np.uint8).reshape(n, cap, 28)).to(dev)
        d_counts = torch.ones(n, dtype=torch.int32, device=dev)
        d_chips = torch.empty((n, out, out, 3), dtype=torch.uint8, device=dev)
        d_info = torch.empty((n, 28), dtype=torch.uint8, device=dev)
        d_first = torch.empty(n + 1, dtype=torch.int32, device=dev)
        d_frames = torch.empty((n, out, out, 3), dtype=torch.int8, device=dev)
        d_status = torch.empty(n, dtype=torch.int32, device=dev)
        crop = crop_call(bufs, nbytes, d_desc, d_dets, d_counts, n, cap, out, d_chips, n, d_first, d_info)
        prep = lambda i: images.prepare_ragged_device(bufs[i % 2].data_ptr(), nbytes, "bgr", d_desc.data_ptr(), n, out, d_frames.data_ptr(),
                                                      d_status.data_ptr(), stream=s)
        t_crop, t_prep = timed(crop, prep)
        same = bool(((d_chips.to(torch.int16) - 128).to(torch.int8) == d_frames).all().item())      # chips in RGB order, as frames are
        lines = region_lines(taps, host, desc["offset"], W * 3, 0, 0, W, H, out, out)
        print(f"prepare {n} x {W}x{H} BGR, the whole picture -> {out}x{out}: prefix + crop {t_crop:8.2f} us, yf_images_prepare_ragged_device "
              f"{t_prep:8.2f} us, crop / prepare = {t_crop / t_prep:5.3f} (interleaved; chips + 128 equal the frames: {same})")
        for name, t in (("crop", t_crop), ("prepare", t_prep)):
            gbps = lines / (t * 1e-6) / 1e9
            print(f"prepare touched {lines / 1e9:5.3f} GB, written {n * out * out * 3 / 1e9:5.3f} GB: {name:8s} {gbps:6.0f} GB/s read "
                  f"({100 * gbps / (HBM_TBPS * 1e3):4.1f} % of {HBM_TBPS} TB/s)")
        del bufs, d_chips, d_frames
        torch.cuda.empty_cache()

    if not args.only or args.only == "upscale":
        n, cap, out, side = 4096, 8, 112, 40
        desc, nbytes = descriptors(n)
        bufs = [torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device=dev) for _ in range(2)]
        d_desc = torch.from_numpy(desc.view(np.uint8)).to(dev)
        rng = np.random.default_rng(40)
        dets = np.zeros((n, cap), binding.DET_DTYPE)
        dets["x1"], dets["y1"] = rng.integers(0, W - side, (n, cap)), rng.integers(0, H - side, (n, cap))
        dets["x2"], dets["y2"] = dets["x1"] + side - 1, dets["y1"] + side - 1
        d_dets = torch.from_numpy(dets.view(np.uint8).reshape(n, cap, 28)).to(dev)
        d_counts = torch.full((n,), cap, dtype=torch.int32, device=dev)
        total = n * cap
        d_chips = torch.empty((total, out, out, 3), dtype=torch.uint8, device=dev)
        d_info = torch.empty((total, 28), dtype=torch.uint8, device=dev)
        d_first = torch.empty(n + 1, dtype=torch.int32, device=dev)
        t_crop, = timed(crop_call(bufs, nbytes, d_desc, d_dets, d_counts, n, cap, out, d_chips, total, d_first, d_info))
        sample = range(0, n, 64)                                                  # the model on every 64th picture, scaled
        lines = sum(region_lines(taps, host, [desc["offset"][i]], W * 3, int(dets["x1"][i, k]), int(dets["y1"][i, k]), side, side, out, out)
                    for i in sample for k in range(cap)) * (n / len(sample))
        written = total * out * out * 3
        print(f"upscale {n} x {W}x{H} BGR, {cap} regions of {side}x{side} each -> {out}x{out} ({total} chips): prefix + crop {t_crop:8.2f} us = "
              f"{total / t_crop:6.2f} M chips/s")
        print(f"upscale touched {lines / 1e9:5.3f} GB = {lines / (t_crop * 1e-6) / 1e9:6.0f} GB/s read "
              f"({100 * lines / (t_crop * 1e-6) / 1e12 / HBM_TBPS:4.1f} % of {HBM_TBPS} TB/s); written {written / 1e9:5.3f} GB = "
              f"{written / (t_crop * 1e-6) / 1e9:6.0f} GB/s ({100 * written / (t_crop * 1e-6) / 1e12 / HBM_TBPS:4.1f} %); "
              f"{total * out * out / (t_crop * 1e-6) / 1e9:6.1f} G output pixels/s")
    net.destroy()


if __name__ == "__main__":
    main()
