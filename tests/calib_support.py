"""What the calibration tests share (test_calib_host.py, test_calib_gpu.py): the two float weight sets as .yfw bytes, the calibration frames,
and the host build's ranges, logits and quantised models, each computed once per process."""
import functools
import importlib
import os

import numpy as np

from conftest import ROOT, GOLDEN

calib = importlib.import_module("stm32h7-yolo_amd.calib")
ptq = importlib.import_module("stm32h7-yolo_amd.ptq")
model_file = importlib.import_module("stm32h7-yolo_amd.model_file")

SHIPPED_YFM = os.path.join(ROOT, "oracle", "model", "yoloface_int8.yfm")
WEIGHT_SETS = ("npz", "yfw")            # the float weights the shipped int8 model was quantised from; the shipped .yfw (the ONNX export)


@functools.lru_cache(maxsize=None)
def npz_convs():
    z = np.load(os.path.join(GOLDEN, "ptq_float_convs.npz"))
    return [(z[f"w{k}"], z[f"b{k}"], bool(z[f"dw{k}"])) for k in range(24)]


@functools.lru_cache(maxsize=None)
def yfw_bytes(name):
    if name == "npz":
        return model_file.write_yfw(npz_convs())
    return open(os.path.join(ROOT, "stm32h7-yolo_amd", "model", "yoloface_fp32.yfw"), "rb").read()


@functools.lru_cache(maxsize=None)
def calib_frames():
    x = np.fromfile(os.path.join(GOLDEN, "calib_frames_56_cv.bin"), np.int8).reshape(-1, 56, 56, 3)
    assert x.shape[0] == 27
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def host_result(name):
    """(ranges, logits) of the host build on the 27 calibration frames"""
    r, lg = calib.host_run(yfw_bytes(name), calib_frames())
    lg.setflags(write=False)
    return r, lg


@functools.lru_cache(maxsize=None)
def host_model(name):
    """the .yfm bytes quantize_model makes of the weight set and the host build's ranges"""
    return ptq.quantize_model(yfw_bytes(name), host_result(name)[0])


class HostCalibration:
    """A test aid: calib.Calibration's interface on the CPU, through calib.host_run -- observe(frames) with int8 numpy frames, ranges(), logits
    (numpy), reset().  The accumulation and the "no frame yet" refusal here are this class's own bookkeeping; the library's (yf_calib_ranges)
    are exercised where the library runs, in test_calib_gpu.py."""

    def __init__(self, yfw_bytes, threads=1):
        self.yfw, self.threads = bytes(yfw_bytes), threads
        calib.host_run(self.yfw, np.zeros((1, 56, 56, 3), np.int8), want_logits=False)      # a refused model is refused here
        self.reset()

    def observe(self, frames, logits=True):
        r, self.logits = calib.host_run(self.yfw, frames, self.threads, logits)
        for t, (lo, hi) in r.items():
            a, b = self._ranges.get(t, (lo, hi))
            self._ranges[t] = (min(a, lo), max(b, hi))
        self.frames_observed += len(np.asarray(frames).reshape(-1, 56, 56, 3))
        return self.frames_observed

    def ranges(self):
        if not self._ranges:
            raise calib.CalibError("ranges: no frame has been observed yet: there are no ranges")
        return dict(self._ranges)

    def reset(self):
        self._ranges, self.logits, self.frames_observed = {}, None, 0


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def ranges_array(r):
    """{tensor: (min, max)} -> (sorted tensor ids, float32 [n, 2])"""
    ids = sorted(r)
    return ids, np.array([r[t] for t in ids], np.float32)
