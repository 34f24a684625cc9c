#!/usr/bin/env python3
"""yf_images_run_decode_f16_device / _ragged_device on a network that never saw yf_network_fp16_init: an error that carries the network's
own text, nothing launched, every output untouched -- and the int8 path of the same network still works afterwards.  Test helper:
tests/test_images_float_gpu.py runs it in a fresh process, so that the test session's shared network keeps its fp16 state."""
import importlib, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
yf = importlib.import_module("stm32h7-yolo_amd")
torch.cuda.is_available()
net = yf.Network(device=0).init()
images = importlib.import_module("stm32h7-yolo_amd.images")
n, H, W, cap = 3, 40, 50, 147
imgs = [np.random.default_rng(k).integers(0, 256, (H, W, 3), dtype=np.uint8) for k in range(n)]
buf, desc = images.pack_images(imgs, "bgr", align=H * W * 3)
d_px = torch.from_numpy(buf).cuda()
d_desc = torch.from_numpy(desc.view(np.uint8).copy()).cuda()
outs = dict(frames=torch.full((n, 56, 56, 3), 0x4D4D, dtype=torch.int16, device="cuda"),
            logits=torch.full((n, 7, 7, 18), 7.0, dtype=torch.float32, device="cuda"),
            dets=torch.full((n, cap, 28), 0xA5, dtype=torch.uint8, device="cuda"),
            counts=torch.full((n,), -7, dtype=torch.int32, device="cuda"),
            status=torch.full((n,), -7, dtype=torch.int32, device="cuda"))
before = {k: v.clone() for k, v in outs.items()}
texts = []
for ragged in (False, True):
    try:
        if ragged:
            images.run_decode_f16_ragged_device(net, d_px.data_ptr(), buf.nbytes, "bgr", d_desc.data_ptr(), n, outs["frames"].data_ptr(),
                                                outs["logits"].data_ptr(), outs["dets"].data_ptr(), outs["counts"].data_ptr(), cap,
                                                outs["status"].data_ptr())
        else:
            images.run_decode_f16_device(net, d_px.data_ptr(), buf.nbytes, "bgr", H, W, W * 3, H * W * 3, n, outs["frames"].data_ptr(),
                                         outs["logits"].data_ptr(), outs["dets"].data_ptr(), outs["counts"].data_ptr(), cap)
    except images.ImagesError as e:
        texts.append(str(e))
torch.cuda.synchronize()
untouched = all(torch.equal(outs[k], before[k]) for k in outs)
print(f"errors: {texts}", flush=True)
said_so = len(texts) == 2 and all("yf_network_fp16_init first" in t for t in texts)
# the network is otherwise sound: the int8 image path runs, and after fp16_init the fp16 one does too
boxes8 = images.detect(net, imgs, "bgr")
net.fp16_init()
boxes16 = images.detect(net, imgs, "bgr", dtype="fp16")
ok = untouched and said_so and len(boxes8) == n and len(boxes16) == n
print("float-without-init ok" if ok else f"float-without-init FAILED (untouched {untouched}, said so {said_so})")
net.destroy()
sys.exit(0 if ok else 1)
