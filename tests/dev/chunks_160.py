#!/usr/bin/env python3
"""The 160x160 path over several chunks of its HBM arena, against the CPU oracle.  YF_160_CHUNK is read when the engine is created, so each case sets it and
   creates a network of its own (this process has no other).  Cases: 41 frames in chunks of 16 (16 + 16 + 9: the XCD job order twice, the plain order once;
   frame and head pointers advance by chunks, every chunk reuses the arena), 8 frames in one chunk of 8, 232 frames in chunks of 112 (112 + 112 + 8: chunks
   whose workgroups take second jobs in band_k1 / band_k23, then one without) -- each under the reference rounding and the fp32 requantisation, after a launch
   of the frames' complements (tests/model_variants.py, run_160_after_complement).  One line per case; exit status 1 at the first mismatch.
   Test helper: tests/test_band160_reuse_gpu.py runs it in a fresh process; runs on the GPU box."""
import importlib, os, sys
import numpy as np, torch
TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.dirname(TESTS), TESTS]
import model_variants as mv
from oracle.oracle import Oracle
yf = importlib.import_module("stm32h7-yolo_amd")
CASES = ((16, 41), (8, 8), (112, 232))                       # (YF_160_CHUNK, frames)
ROUNDINGS = (0, mv.FP32)
x = mv.reuse_frames_160(max(n for _, n in CASES))
orc = Oracle()
ref = {r: orc.run(x, threads=16, variant=mv.ROUNDINGS[r][1]) for r in ROUNDINGS}
assert all(len({h.tobytes() for h in ref[r]}) == x.shape[0] for r in ROUNDINGS)
d_x = torch.from_numpy(x).cuda()
for chunk, n in CASES:
    os.environ["YF_160_CHUNK"] = str(chunk)
    sizes = "+".join(str(min(chunk, n - done)) for done in range(0, n, chunk))
    net = yf.Network(device=0).init()
    try:
        for r in ROUNDINGS:
            net.set_requant_rounding(r)
            assert ("fp32 requantisation" in net.kernel_name) == (r == mv.FP32)
            got = mv.run_160_after_complement(torch, net, d_x, n)
            d = mv.first_difference(got.reshape(n, -1), ref[r][:n].reshape(n, -1), (20, 20, 18))
            what = f"chunks YF_160_CHUNK={chunk} n={n} ({sizes}) rounding {mv.rounding_name(r)}:"
            if d is not None:
                print(what, f"MISMATCH first at (frame, y, x, channel) = {d[:4]}: got {d[4]}, oracle {d[5]}; frame {d[0]} is frame {d[0] % chunk} of chunk {d[0] // chunk}", flush=True)
                sys.exit(1)
            print(what, "ok", flush=True)
    finally:
        net.destroy()
sys.exit(0)
