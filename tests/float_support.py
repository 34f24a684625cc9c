"""What the tests of the fp16 image path share (test_images_float_*): the host build's float functions, the restatement of the reference's
float decode (yoloface/tensorflow/h5_predition.py:51-72) in numpy, the exponential it is stated with, and the logits the decodes are
compared on.

`decode_restated` follows the script's array program step by step: reshape(7, 7, 3, 6).transpose(2, 0, 1, 3), np.meshgrid's grid,
(sigmoid(xy) + grid) * 8, exp(wh) * anchors, sigmoid of the rest, the rows above 0.7, xywh -> xyxy, the two scales, int32.  Its `E` is a
parameter: `exp_rounded` (the library's stated choice: float64 exp, rounded once) or `np.exp` on float32 (what the script literally runs)."""
import ctypes
import os

import numpy as np

from conftest import ROOT
from images_support import host_lib

DET = np.dtype([("frame", "<i4"), ("anchor", "u1"), ("row", "u1"), ("col", "u1"), ("q_conf", "i1"),
                ("conf", "<f4"), ("x1", "<i4"), ("y1", "<i4"), ("x2", "<i4"), ("y2", "<i4")])
LN_7_3 = float(np.log(7.0 / 3.0))                 # sigmoid(t) > 0.7  <=>  t > ln(7/3)
ANCHORS = ((9, 14), (12, 17), (22, 21))


def float_host():
    """libyf_images_host.so with the prototypes of its float functions (csrc/yf_images_float.h through csrc/yf_images_host.c)"""
    lib = host_lib()
    vp = ctypes.c_void_p
    lib.yfi_f16_of_u8_host.restype = None
    lib.yfi_f16_of_u8_host.argtypes = [vp]
    for fn in (lib.yfi_exp_f32_host, lib.yfi_sigmoid_f32_host):
        fn.restype = None
        fn.argtypes = [vp, ctypes.c_long, vp]
    lib.yfi_decode_f32_host.restype = ctypes.c_int
    lib.yfi_decode_f32_host.argtypes = [vp, ctypes.c_int32, ctypes.c_float, ctypes.c_float, vp, ctypes.c_int]
    return lib


def host_halves(lib):
    h = np.zeros(256, np.uint16)
    lib.yfi_f16_of_u8_host(h.ctypes.data)
    return h


def host_exp(lib, x, fn="yfi_exp_f32_host"):
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty_like(x)
    getattr(lib, fn)(x.ctypes.data, x.size, out.ctypes.data)
    return out


def host_decode(lib, logits, frame, w_scale, h_scale, cap):
    """(true count, the min(count, cap) records written) of one frame; slots beyond stay 0xA5 and are checked here"""
    t = np.ascontiguousarray(logits, np.float32)
    recs = np.frombuffer(bytes([0xA5]) * (28 * cap), DET).copy()
    count = lib.yfi_decode_f32_host(t.ctypes.data, frame, w_scale, h_scale, recs.ctypes.data, cap)
    k = min(count, cap)
    assert (recs[k:].view(np.uint8) == 0xA5).all()
    return count, recs[:k]


def exp_rounded(x):
    """E: the float32 nearest to the float64 value of e^x"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.exp(np.asarray(x, np.float32).astype(np.float64)).astype(np.float32)


def exp_numpy_f32(x):
    with np.errstate(over="ignore", under="ignore"):
        return np.exp(np.asarray(x, np.float32))


def to_int32(v):
    """float32 -> int32 as the script's astype(np.int32) does on an x86-64 PC: truncation, out of range and NaN -> INT32_MIN"""
    v = np.asarray(v, np.float32)
    ok = np.isfinite(v) & (v > np.float32(-2147483904.0)) & (v < np.float32(2147483648.0))
    return np.where(ok, np.trunc(np.where(ok, v, 0)).astype(np.int64), -2 ** 31).astype(np.int32)


def scales_of(width, height):
    """W/56. and H/56. as they act on a float32 array"""
    return float(np.float32(width / 56.)), float(np.float32(height / 56.))


def decode_restated(logits, frame, w_scale, h_scale, E=exp_rounded):
    """All records of one frame [7, 7, 18], in the script's order, as a DET array; also the float32 confidences of all 147 candidates"""
    one = np.float32(1)

    def sigmoid(x):
        with np.errstate(over="ignore", invalid="ignore"):
            return one / (one + E(-x))

    output = np.array(logits, np.float32).reshape((7, 7, 3, 6)).transpose([2, 0, 1, 3]).copy()
    anchors = np.zeros([3, 1, 1, 2], dtype=np.float32)
    for a, wh in enumerate(ANCHORS):
        anchors[a, 0, 0, :] = wh
    yv, xv = np.meshgrid(np.arange(7), np.arange(7))
    grid = np.stack((yv, xv), 2).reshape((1, 7, 7, 2)).astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        output[..., 0:2] = (sigmoid(output[..., 0:2]) + grid) * 8
        output[..., 2:4] = E(output[..., 2:4]) * anchors
        output[..., 4:] = sigmoid(output[..., 4:])
        flat = output.reshape((-1, 6))
        keep = np.nonzero(flat[..., 4] > np.float32(0.7))[0]
        x = flat[keep]
        box = np.zeros((x.shape[0], 4), dtype=np.float32)
        box[..., 0] = x[..., 0] - x[..., 2] / 2
        box[..., 1] = x[..., 1] - x[..., 3] / 2
        box[..., 2] = x[..., 0] + x[..., 2] / 2
        box[..., 3] = x[..., 1] + x[..., 3] / 2
        box[:, [0, 2]] *= np.float32(w_scale)
        box[:, [1, 3]] *= np.float32(h_scale)
    edges = to_int32(box)
    recs = np.zeros(keep.shape[0], DET)
    recs["frame"] = frame
    recs["anchor"], recs["row"], recs["col"] = keep // 49, keep % 49 // 7, keep % 7
    recs["conf"] = x[:, 4]
    recs["x1"], recs["y1"], recs["x2"], recs["y2"] = edges[:, 0], edges[:, 1], edges[:, 2], edges[:, 3]
    return recs, flat[:, 4].copy()


def same_bytes(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- logits ----
def fp32_convs():
    from oracle.np_fp32 import load_yfw
    return load_yfw(os.path.join(ROOT, "stm32h7-yolo_amd", "model", "yoloface_fp32.yfw"))


def real_frames_u8():
    real = np.fromfile(os.path.join(ROOT, "tests", "golden", "real_frames_56.bin"), np.int8).reshape(-1, 56, 56, 3)
    return (real.astype(np.int16) + 128).astype(np.uint8)


def fp32_logits(frames_u8):
    """the float32 network on uint8 RGB frames [n, 56, 56, 3] / 255: logits float32 [n, 7, 7, 18]"""
    from oracle.np_fp32 import run_fp32
    convs = fp32_convs()
    return np.stack([run_fp32(convs, f.astype(np.float32) / 255) for f in frames_u8]).astype(np.float32)


def threshold_neighbours():
    """ln(7/3) as a float32 and its 8 neighbours on each side"""
    c = np.float32(LN_7_3).view(np.uint32).astype(np.int64)
    return (c + np.arange(-8, 9)).astype(np.uint32).view(np.float32)


def seeded_logits(n=512, seed=77):
    return (np.random.default_rng(seed).standard_normal((n, 7, 7, 18)) * 3).astype(np.float32)


def special_logits(seed=78):
    """frames built of specials: NaN, +-inf, +-89, +-104 and the neighbours of the threshold, mixed with ordinary values"""
    rng = np.random.default_rng(seed)
    pool = np.concatenate([np.float32([np.nan, np.inf, -np.inf, 89, -89, 104, -104, 0.0, -0.0, 88.5, -87.5, -103.5]), threshold_neighbours(),
                           (rng.standard_normal(24) * 3).astype(np.float32)])
    frames = rng.choice(pool, (48, 7, 7, 18)).astype(np.float32)
    nb = threshold_neighbours()
    # confidence logits walking through the threshold's neighbours, every other logit special
    walk = rng.choice(pool, (16, 7, 7, 18)).astype(np.float32)
    walk[..., 4::6] = nb[np.arange(16 * 49 * 3) % nb.size].reshape(16, 7, 7, 3)
    # every candidate firing (cap below the count), boxes ordinary or special
    full = rng.choice(pool, (8, 7, 7, 18)).astype(np.float32)
    full[..., 4::6] = np.float32(5.0)
    full[:4, ..., 0:4] = (rng.standard_normal((4, 7, 7, 4)) * 2).astype(np.float32)
    return np.concatenate([frames, walk, full])


# ---- the device side ----
def expect_frame_f16(ptq, halves, img, fmt):
    """the restatement: RGB order, cv2.resize to 56x56, the half of pixel / 255. -- as fp16 bits"""
    from images_support import BGR
    rgb = img[..., :3][..., ::-1] if BGR[fmt] else img[..., :3]
    return halves[ptq.resize_linear_u8(np.ascontiguousarray(rgb), 56, 56)]


FRAME_FILL = 0x4D4D                                # what frames hold before a call (fp16 bits)


class F16Batch:
    """a packed ragged batch on the device with the workspaces of the fp16 path; one extra frame, record row and count behind the batch
    show that nothing is written there.  Frames are filled with FRAME_FILL, logits with 7.0, status with -7, records 0xA5, counts -7."""

    def __init__(self, torch, images, imgs, fmt, cap=147, desc=None, buf=None):
        if desc is None:
            buf, desc = images.pack_images(imgs, fmt)
        self.n, self.buf, self.desc, self.fmt, self.cap = desc.shape[0], buf, desc, fmt, cap
        n = self.n + 1
        self.d_px = torch.from_numpy(buf).cuda()
        self.d_desc = torch.from_numpy(desc.view(np.uint8).copy()).cuda()
        self.d_frames = torch.full((n, 56, 56, 3), FRAME_FILL, dtype=torch.int16, device="cuda")
        self.d_logits = torch.full((n, 7, 7, 18), 7.0, dtype=torch.float32, device="cuda")
        self.d_dets = torch.full((n, cap, 28), 0xA5, dtype=torch.uint8, device="cuda")
        self.d_counts = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        self.d_status = torch.full((n,), -7, dtype=torch.int32, device="cuda")

    def prepare(self, images):
        images.prepare_f16_ragged_device(self.d_px.data_ptr(), self.buf.nbytes, self.fmt, self.d_desc.data_ptr(), self.n,
                                         self.d_frames.data_ptr(), self.d_status.data_ptr())

    def run_decode(self, images, network):
        images.run_decode_f16_ragged_device(network, self.d_px.data_ptr(), self.buf.nbytes, self.fmt, self.d_desc.data_ptr(), self.n,
                                            self.d_frames.data_ptr(), self.d_logits.data_ptr(), self.d_dets.data_ptr(),
                                            self.d_counts.data_ptr(), self.cap, self.d_status.data_ptr())

    def frames(self):
        return self.d_frames.cpu().numpy().view(np.uint16)

    def untouched_behind(self):
        n = self.n
        return bool((self.d_frames[n] == FRAME_FILL).all().item() and (self.d_logits[n] == 7.0).all().item() and
                    (self.d_dets[n] == 0xA5).all().item() and self.d_counts[n].item() == -7 and self.d_status[n].item() == -7)


def device_records(d_dets, d_counts, cap):
    """device records and counts -> DET [n, cap], int32 [n], raw bytes [n, cap, 28]"""
    raw = d_dets.cpu().numpy()
    return raw.view(DET).reshape(-1, cap), d_counts.cpu().numpy(), raw.reshape(-1, cap, 28)


def check_records_against_host(lib, logits, scales, dets, counts, raw, cap, frames=None):
    """every frame's records and count equal the host build's on the same logits, byte for byte; slots beyond keep their sentinel"""
    total = 0
    for f in (range(logits.shape[0]) if frames is None else frames):
        ws, hs = scales[f] if isinstance(scales, list) else scales
        count, want = host_decode(lib, logits[f], f, ws, hs, cap)
        assert counts[f] == count, (f, counts[f], count)
        k = min(count, cap)
        assert dets[f, :k].tobytes() == want.tobytes(), f
        assert (raw[f, k:] == 0xA5).all(), f
        total += k
    return total
