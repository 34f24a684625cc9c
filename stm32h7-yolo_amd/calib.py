"""ctypes binding of libyf_calib.so (include/yf_calib.h): calibration of a FLOAT model of the network on the GPU, and with it the whole way from
retrained float weights to a model the int8 engine runs:

    float weights -> .yfw (model_file.write_yfw) -> Calibration.observe(frames) -> ranges() -> ptq.quantize_model -> .yfm
                  -> Network.init_model / Interpreter(model_content=...)

The evaluation is float32 with the arithmetic csrc/yf_calib_arith.h defines ("Calibration arithmetic"); `host_run` is the same
arithmetic on the CPU (libyf_calib_host.so), bit for bit.  Unlike libyf_images.so the library needs no network: it links the HIP runtime only.
"""
import ctypes
import os

import numpy as np

from . import binding, libs

N_RANGES = 47
FRAME_BYTES = 56 * 56 * 3
LOGITS = 7 * 7 * 18


class CalibError(RuntimeError):
    pass


def lib_path():
    """libyf_calib.so in the package's lib/: it shares nothing with libyf_network.so, so a YF_LIB_PATH override of that one does not move it."""
    return os.path.join(libs.LIB_DIR, "libyf_calib.so")


def host_lib_path():
    return os.path.join(libs.LIB_DIR, "libyf_calib_host.so")


def expected_build_id():
    """The id csrc/Makefile bakes into libyf_calib.so (yf_calib_build_id): sha256 over CALIB_SRCS, CALIBFLAGS and the CFLAGS of the parser."""
    return libs.source_id(libs.make_var("CALIB_SRCS").split(), libs.make_var("CALIBFLAGS") + "|" + libs.make_var("CFLAGS") + "\n")


def library_is_current():
    """True when the in-tree libyf_calib.so can be loaded without running make: it is newer than its sources and the Makefile.  Its baked-in
    id is still checked after loading."""
    return libs.newer_than(lib_path(), libs.make_var("CALIB_SRCS").split() + ["Makefile"])


_lib = None
_host = None


def load():
    """dlopen libyf_calib.so after the HIP runtime PyTorch uses (binding._one_hip_runtime: one runtime per process), rebuilding it when its
    sources are newer; an existing file is used without a build only if it is current and carries the expected id."""
    global _lib
    if _lib is not None:
        return _lib
    lib = libs.open_library(lib_path(), library_is_current, [("yf_calib_build_id", expected_build_id)], preload=binding._one_hip_runtime)
    lib.yf_calib_build_id.restype = ctypes.c_char_p
    lib.yf_calib_build_id.argtypes = []
    vp = ctypes.c_void_p
    lib.yf_calib_create.restype, lib.yf_calib_create.argtypes = vp, [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int]
    lib.yf_calib_observe_device.restype, lib.yf_calib_observe_device.argtypes = ctypes.c_long, [vp, vp, ctypes.c_long, vp, vp]
    lib.yf_calib_ranges.restype, lib.yf_calib_ranges.argtypes = ctypes.c_int, [vp, vp, vp]
    lib.yf_calib_reset.restype, lib.yf_calib_reset.argtypes = ctypes.c_int, [vp]
    lib.yf_calib_frames_observed.restype, lib.yf_calib_frames_observed.argtypes = ctypes.c_long, [vp]
    lib.yf_calib_destroy.restype, lib.yf_calib_destroy.argtypes = None, [vp]
    lib.yf_calib_last_error_text.restype, lib.yf_calib_last_error_text.argtypes = ctypes.c_char_p, []
    _lib = lib
    return lib


def load_host():
    """libyf_calib_host.so (no HIP, no GPU) through libs.host_library, which brings it up to date first."""
    global _host
    if _host is None:
        lib = libs.host_library("libyf_calib_host.so")
        vp = ctypes.c_void_p
        lib.yf_calib_host_run.restype = ctypes.c_long
        lib.yf_calib_host_run.argtypes = [ctypes.c_char_p, ctypes.c_size_t, vp, ctypes.c_long, vp, vp, vp, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]
        _host = lib
    return _host


def _ranges_dict(minmax, ids):
    return {int(t): (float(minmax[i, 0]), float(minmax[i, 1])) for i, t in enumerate(ids)}


def host_run(yfw_bytes, frames, threads=1, want_logits=True):
    """The evaluation on the CPU: int8 frames [n, 56, 56, 3] -> ({tensor id: (min, max)} of these frames, float32 logits [n, 7, 7, 18] or
    None).  A refused .yfw raises CalibError with the parser's text."""
    lib = load_host()
    x = np.ascontiguousarray(frames, np.int8).reshape(-1, 56, 56, 3)
    n = x.shape[0]
    minmax, ids = np.zeros((N_RANGES, 2), np.float32), np.zeros(N_RANGES, np.int32)
    logits = np.zeros((n, 7, 7, 18), np.float32) if want_logits else None
    err = ctypes.create_string_buffer(400)
    rc = lib.yf_calib_host_run(bytes(yfw_bytes), len(yfw_bytes), x.ctypes.data, n, minmax.ctypes.data, ids.ctypes.data,
                               logits.ctypes.data if want_logits else None, int(threads), err, 400)
    if rc != n:
        raise CalibError(f"yf_calib_host_run: {err.value.decode()} (returned {rc}, expected {n})")
    return _ranges_dict(minmax, ids), logits


class Calibration:
    """A calibration of the float model `yfw_bytes` on GPU `device` (None: torch's current device).

    observe(frames)  frames: an int8 device tensor [n, 56, 56, 3] (or a numpy array, which is uploaded).  Asynchronous on torch's current
                     stream (or `stream`, a raw hipStream_t); folds the frames' extremes into the ranges so far.
    ranges()         synchronises: {tflite tensor id: (min, max)} over everything observed since creation or reset() -- the input, every
                     convolution, LeakyReLU and ADD output and the two pool outputs: what ptq.quantize_model takes.
    logits           the float32 logits [n, 7, 7, 18] of the last observe (a device tensor; None before the first, or with logits=False)."""

    def __init__(self, yfw_bytes, device=None):
        import torch
        self._lib = load()
        torch.cuda.init()
        if device is None:
            self.device = torch.cuda.current_device()
        else:
            self.device = torch.device("cuda", device).index if isinstance(device, int) else torch.device(device).index
        self.handle = self._lib.yf_calib_create(bytes(yfw_bytes), len(yfw_bytes), self.device)
        if not self.handle:
            raise CalibError(f"yf_calib_create: {self._text()}")
        self.logits = None
        self._keep = None

    def _text(self):
        return (self._lib.yf_calib_last_error_text() or b"").decode()

    def observe(self, frames, logits=True, stream=None):
        import torch
        if not isinstance(frames, torch.Tensor):
            frames = torch.from_numpy(np.ascontiguousarray(frames, np.int8))
        dev = torch.device("cuda", self.device)
        if frames.dtype != torch.int8 or frames.numel() % FRAME_BYTES or frames.numel() == 0:
            raise ValueError(f"frames: expected int8 [n, 56, 56, 3] with n >= 1, got {frames.dtype} {tuple(frames.shape)}")
        frames = frames.to(dev).contiguous()
        n = frames.numel() // FRAME_BYTES
        out = torch.empty((n, 7, 7, 18), dtype=torch.float32, device=dev) if logits else None
        s = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        rc = self._lib.yf_calib_observe_device(self.handle, frames.data_ptr(), n, out.data_ptr() if logits else None, s)
        if rc != n:
            raise CalibError(f"yf_calib_observe_device: {self._text()} (returned {rc}, expected {n})")
        self._keep, self.logits = frames, out       # the launch is asynchronous: the frames stay alive until the next call
        return n

    @property
    def frames_observed(self):
        return self._lib.yf_calib_frames_observed(self.handle)

    def ranges(self):
        minmax, ids = np.zeros((N_RANGES, 2), np.float32), np.zeros(N_RANGES, np.int32)
        rc = self._lib.yf_calib_ranges(self.handle, minmax.ctypes.data, ids.ctypes.data)
        if rc != N_RANGES:
            raise CalibError(f"yf_calib_ranges: {self._text()} (returned {rc})")
        return _ranges_dict(minmax, ids)

    def reset(self):
        if self._lib.yf_calib_reset(self.handle) != 0:
            raise CalibError(f"yf_calib_reset: {self._text()}")
        self.logits = None

    def destroy(self):
        if self.handle:
            self._lib.yf_calib_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def quantize_on_device(yfw_bytes, frames, device=None):
    """Float weights (.yfw bytes) and calibration frames -> the bytes of a .yfm image for Network.init_model: the frames are evaluated on the
    GPU, the ranges go through ptq.quantize_model.  `frames`: an int8 DEVICE tensor [n, 56, 56, 3] of the network's frames (pixel - 128,
    RGB).  Decoded images of any size become such frames through images.prepare_device / prepare_ragged_device first; this function does
    not wrap that step."""
    from . import ptq
    cal = Calibration(yfw_bytes, device)
    try:
        cal.observe(frames, logits=False)
        return ptq.quantize_model(yfw_bytes, cal.ranges())
    finally:
        cal.destroy()
