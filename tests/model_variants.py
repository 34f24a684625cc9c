"""Weight blobs other than the shipped one, for the tests (plain module, TEST INFRASTRUCTURE ONLY).

ai_network_init builds the device tables from the CALLER's 11304-byte weight/bias blob; the oracle reads a .yfm model file.  A variant is a byte
patch of both: the blob at the ST offsets (csrc/gen/yf_model_gen.h, yf_convs[]: w_off, b_off) and the .yfm at data_base + doff of the same tensors
(oracle/np_restatement.py, load_yfm), file sizes unchanged, so that network.init(weights=blob) and Oracle(yfm_path) state the same network.  Scales
and zero points stay the shipped ones (they are compiled into the library).  Everything is seeded and deterministic, and nothing outside the
repository is read."""
import os
import re
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GEN = os.path.join(ROOT, "stm32h7-yolo_amd", "csrc", "gen")
SHIPPED_YFM = os.path.join(ROOT, "oracle", "model", "yoloface_int8.yfm")
BLOB_BYTES = 11304
ACC_LIMIT = 1 << 29                 # the host admits a channel while |bias'| + 255 * sum|w| < 2^29 (yf_tables.h, yf_pass)
FP32_LIMIT = 2097152.0              # ... and, for YF_ROUND_FP32, while acc_max * fs < 2^21 (yf_host_prep.c, build_chan_fp32)
YF_PREP_ERR_SHIFT_RANGE = 3
DENSE_OPS = [1, 5, 6, 12, 13, 17, 19, 23, 29, 30, 34, 36, 40, 42, 47, 51, 53]      # execution order == index of yf_table_index.dense[]
DW_OPS = [3, 10, 15, 27, 32, 38, 49]                                               # ... of yf_table_index.dw[]
CONV_OPS = sorted(DENSE_OPS + DW_OPS)
# library rounding (include/yf_network.h YF_ROUND_*) -> (name, oracle variant, oracle mbqm mode of the dense convs, of the depthwise convs)
FP32 = 0x10
GENERIC = 0x100
ROUNDINGS = {0: ("ref", 0, 0, 0), 1: ("ties_up", 1, 1, 0), 2: ("ties_up_all", 2, 1, 1), 3: ("single", 4, 2, 0), FP32: ("fp32", 3, None, None)}
# the dump build's records in order (tests/test_gpu_parity.py STAGES): (name, tflite op)
STAGES = [("T1", 2), ("T2", 4), ("T3", 5), ("T4", 7), ("Q21", 21), ("T6", 11), ("T7", 12), ("T8", 14), ("T9", 16),
          ("T11", 18), ("T14", 22), ("T15", 24), ("Q45", 45), ("T17", 28), ("T18", 29), ("T19", 31), ("T20", 33),
          ("T22", 35), ("T23", 37), ("T24", 39), ("T26", 41), ("T30", 46), ("T31", 48), ("T32", 50), ("T33", 52),
          ("P8", 8), ("C17", 17), ("P25", 25), ("C34", 34), ("C40", 40), ("L43", 43)]
# the 19 byte LUTs (yf_tables.h YF_L_*): id -> the tflite op whose INPUT tensor indexes it
LUT_INPUT_OP = {0: 2, 1: 4, 2: 7, 3: 21, 4: 11, 5: 14, 6: 16, 7: 20, 8: 24, 9: 45, 10: 28, 11: 31, 12: 33, 13: 37, 14: 39, 15: 43, 16: 48, 17: 50, 18: 52}


def rounding_name(r):
    return ROUNDINGS[r & 0xFF][0] + ("+generic" if r & GENERIC else "")


# ---- the shipped model: blob bytes, conv table, .yfm ---------------------------------------------------------------------------------
def shipped_blob():
    src = open(os.path.join(GEN, "yf_weights_blob_gen.c")).read()
    body = src[src.index("{") + 1: src.rindex("}")]
    blob = bytes(int(v) for v in re.findall(r"\d+", body))
    assert len(blob) == BLOB_BYTES
    return blob


def conv_table():
    """yf_convs[] of csrc/gen/yf_model_gen.h: tflite op -> dict(depthwise, kh, kw, cin, cout, t_in, t_out, w_off, b_off)."""
    src = open(os.path.join(GEN, "yf_model_gen.h")).read()
    rows = re.findall(r"^\s*\{(\d+(?:,\s*\d+){12}),\s*yf_conv\d+_wscale_bits\},", src, re.M)
    out = {}
    for r in rows:
        v = [int(x) for x in r.split(",")]
        out[v[0]] = dict(op=v[0], depthwise=v[1], kh=v[2], kw=v[3], cin=v[7], cout=v[8], t_in=v[9], t_out=v[10], w_off=v[11], b_off=v[12])
    assert sorted(out) == CONV_OPS
    return out


class Model:
    """The convolutions' weights and biases in the tflite tensor layout (dense OHWI, depthwise 1HWC), as [cout, k] / [9, c] int8 and int32[cout]."""

    def __init__(self):
        from oracle.np_restatement import load_yfm
        self.convs = conv_table()
        self.yfm_bytes = open(SHIPPED_YFM, "rb").read()
        self.yfm = load_yfm(SHIPPED_YFM)
        nt, no = struct.unpack_from("<2I", self.yfm_bytes, 4)
        self.data_base = 24 + 44 * nt + 52 * no
        self.blob = shipped_blob()
        T, ops = self.yfm["tensors"], self.yfm["ops"]
        self.w, self.b, self.quant = {}, {}, {}
        for op, d in self.convs.items():
            o = ops[op]
            assert o["op"] == (4 if d["depthwise"] else 3)
            wt, bt = T[o["ins"][1]], T[o["ins"][2]]
            shape = (9, d["cout"]) if d["depthwise"] else (d["cout"], d["kh"] * d["kw"] * d["cin"])
            self.w[op] = wt["data"].reshape(shape).copy()
            self.b[op] = bt["data"].astype(np.int32).copy()
            assert self.blob[d["w_off"]:d["w_off"] + wt["dbytes"]] == wt["data"].tobytes()           # blob and .yfm state the same shipped tensors
            assert self.blob[d["b_off"]:d["b_off"] + 4 * d["cout"]] == self.b[op].astype("<i4").tobytes()
            self.quant[op] = dict(zp_in=int(T[d["t_in"]]["zp"]), zp_out=int(T[d["t_out"]]["zp"]), s_in=np.float32(T[d["t_in"]]["scale"][0]),
                                  s_out=np.float32(T[d["t_out"]]["scale"][0]), s_w=wt["scale"].astype(np.float32), w_doff=wt["doff"], b_doff=bt["doff"])

    def per_channel(self, op, w=None):
        """[cout, taps] view of a conv's weights: the taps that feed output channel ch."""
        w = self.w[op] if w is None else w
        return w.T if self.convs[op]["depthwise"] else w

    def sums(self, op, w):
        pc = self.per_channel(op, w).astype(np.int64)
        return pc.sum(axis=1), np.abs(pc).sum(axis=1)

    def fs(self, op, ch):
        """fs of the float32 requantisation: fl32(fl32(s_in * s_w) / s_out), two float32 operations (build_chan_fp32)."""
        q = self.quant[op]
        return np.float32(np.float32(q["s_in"] * q["s_w"][ch]) / q["s_out"])

    def fp32_acc_bound(self, op, ch):
        """the largest acc_max YF_ROUND_FP32 admits for the channel: (double)acc_max * (double)fs < 2^21, and below 2^29"""
        fs = float(self.fs(op, ch))
        a = int(FP32_LIMIT / fs)
        while float(a) * fs >= FP32_LIMIT:
            a -= 1
        while float(a + 1) * fs < FP32_LIMIT:
            a += 1
        return min(a, ACC_LIMIT - 1)

    def write(self, w, b, yfm_path):
        """(blob bytes, yfm_path written) of the network with conv weights w[op] / biases b[op] (ops not named keep the shipped tensors)."""
        blob, yfm = bytearray(self.blob), bytearray(self.yfm_bytes)
        for op, d in self.convs.items():
            wb = np.ascontiguousarray(w.get(op, self.w[op]), np.int8).tobytes()
            bb = np.ascontiguousarray(b.get(op, self.b[op])).astype("<i4").tobytes()
            q = self.quant[op]
            assert len(wb) == self.w[op].size and len(bb) == 4 * d["cout"]
            blob[d["w_off"]:d["w_off"] + len(wb)] = wb
            blob[d["b_off"]:d["b_off"] + len(bb)] = bb
            yfm[self.data_base + q["w_doff"]:self.data_base + q["w_doff"] + len(wb)] = wb
            yfm[self.data_base + q["b_doff"]:self.data_base + q["b_doff"] + len(bb)] = bb
        assert len(blob) == BLOB_BYTES and len(yfm) == len(self.yfm_bytes)
        with open(yfm_path, "wb") as f:
            f.write(bytes(yfm))
        return bytes(blob), str(yfm_path)


_model = None


def model():
    global _model
    if _model is None:
        _model = Model()
    return _model


# ---- variant families ---------------------------------------------------------------------------------------------------------------
def _sat8(x):
    return np.clip(np.rint(x), -127, 127).astype(np.int8)


def _identity(m):
    return {}, {}


def _jitter(m, seed):
    """every weight moved by -2..+2 (never 0) with saturation to int8, every bias by a relative step of up to 1/16 (never 0)"""
    rng = np.random.default_rng(1000 + seed)
    w, b = {}, {}
    for op in CONV_OPS:
        step = rng.integers(1, 3, m.w[op].shape) * rng.choice([-1, 1], m.w[op].shape)
        w0 = m.w[op].astype(np.int64)
        step = np.where((w0 + step > 127) | (w0 + step < -128), -step, step)                       # saturation would leave the byte: step the other way
        w[op] = (w0 + step).astype(np.int8)
        b0 = m.b[op].astype(np.int64)
        rel = np.rint(np.abs(b0) * rng.uniform(1 / 64, 1 / 16, b0.shape)).astype(np.int64) + 1
        b[op] = (b0 + rel * rng.choice([-1, 1], b0.shape)).astype(np.int32)
    return w, b


def _amplify(m, op, gain):
    return {op: _sat8(m.w[op].astype(np.float64) * gain)}, {op: np.rint(m.b[op].astype(np.float64) * gain).astype(np.int32)}


def _bias_edge(m, op, ch, sign, acc_max):
    """channel ch's bias such that |bias'| + 255 * sum|w| == acc_max, bias' = bias - zp_in * sum(w) of the given sign"""
    sum_w, abs_w = m.sums(op, m.w[op])
    bias2 = sign * (acc_max - 255 * int(abs_w[ch]))
    assert sign * bias2 > 0
    b = m.b[op].copy()
    b[ch] = bias2 + m.quant[op]["zp_in"] * int(sum_w[ch])
    return {}, {op: b}


def _uniform(m, op, value):
    return {op: np.full(m.w[op].shape, value, np.int8)}, {}


def _permute(m, op, seed):
    """output channels of one conv (weights and biases) permuted; a derangement-ish shuffle, the per-channel scales stay put"""
    perm = np.random.default_rng(2000 + 64 * seed + op).permutation(m.convs[op]["cout"])
    w = m.w[op][:, perm] if m.convs[op]["depthwise"] else m.w[op][perm]
    return {op: np.ascontiguousarray(w)}, {op: m.b[op][perm]}


# amplify: the gain per conv, chosen on the CPU (tests/test_model_variants_host.py states the conditions and checks them): the targeted conv's output
# reaches both clamps on the test frames, is not constant per channel and takes at least as many distinct values as the shipped model's.
# The first of 2, 3, 4, 6, 8 that meets them; conv2d_53 (the head) takes fewer distinct values than the shipped head at gains 2..16 and meets them at 1.5.
AMPLIFY_GAIN = {1: 2, 3: 3, 5: 2, 6: 2, 10: 2, 12: 2, 13: 2, 15: 2, 17: 2, 19: 2, 23: 2, 27: 2, 29: 2, 30: 2, 32: 2, 34: 2, 36: 2, 38: 2, 40: 3, 42: 2,
                47: 2, 49: 3, 51: 2, 53: 1.5}

BIAS_EDGE_CHANNELS = {5: 2, 15: 17, 1: 3, 53: 17, 27: 16, 47: 39}      # dense, depthwise, conv2d_1 (own packing), the head (cout 18: last pass half filled), ...


class Variant:
    def __init__(self, name, family, fn, args, op=None, refused=False):
        self.name, self.family, self.fn, self.args, self.op, self.refused = name, family, fn, args, op, refused

    def build(self, dirpath):
        """(blob, yfm_path): the .yfm is written into dirpath (pytest's tmp_path)"""
        m = model()
        w, b = self.fn(m, *self.args)
        return m.write(w, b, os.path.join(str(dirpath), self.name + ".yfm"))

    def tensors(self):
        m = model()
        w, b = self.fn(m, *self.args)
        return {op: w.get(op, m.w[op]) for op in CONV_OPS}, {op: b.get(op, m.b[op]) for op in CONV_OPS}

    def acc_max(self):
        """op -> per-channel bound of the accumulator, |bias'| + 255 * sum|w| with bias' = bias - zp_in * sum(w)"""
        m = model()
        w, b = self.tensors()
        out = {}
        for op in CONV_OPS:
            sum_w, abs_w = m.sums(op, w[op])
            out[op] = np.abs(b[op].astype(np.int64) - m.quant[op]["zp_in"] * sum_w) + 255 * abs_w
        return out

    def admitted(self, rounding):
        """what the host states it admits (yf_tables.h, yf_pass): every channel's accumulator bound below 2^29 and, for YF_ROUND_FP32, acc_max * fs
        below 2^21.  Stated here from the bounds, not asked of the library: the host tests assert that yf_prepare_tables_rounding agrees."""
        m = model()
        for op, a in self.acc_max().items():
            if int(a.max()) >= ACC_LIMIT:
                return False
            if rounding == FP32 and any(float(int(a[ch])) * float(m.fs(op, ch)) >= FP32_LIMIT for ch in range(a.shape[0])):
                return False
        return True

    def __repr__(self):
        return self.name


def identity():
    return Variant("identity", "identity", _identity, ())


def jitter(seed):
    return Variant(f"jitter-{seed}", "jitter", _jitter, (seed,))


def amplify(op, gain=None):
    gain = AMPLIFY_GAIN[op] if gain is None else gain
    return Variant(f"amplify-conv2d_{op}-x{gain:g}", "amplify", _amplify, (op, gain), op)


def bias_edge(op, ch, sign, refused=False, acc_max=None):
    """the last admitted accumulator bound (2^29 - 1) or, refused=True, its twin at the first refused one (2^29); acc_max: another bound"""
    a = (ACC_LIMIT if refused else ACC_LIMIT - 1) if acc_max is None else acc_max
    tag = "" if acc_max is None else f"-acc{acc_max}"
    return Variant(f"bias_edge-conv2d_{op}-ch{ch}-{'pos' if sign > 0 else 'neg'}{tag}{'-refused' if refused else ''}", "bias_edge", _bias_edge,
                   (op, ch, sign, a), op, refused)


def uniform(op, value):
    return Variant(f"uniform-conv2d_{op}-{value:+d}".replace("+0", "0"), "uniform", _uniform, (op, value), op)


def permute(op, seed=0):
    return Variant(f"permute-conv2d_{op}-{seed}", "permute", _permute, (op, seed), op)


def bias_edges(refused=False):
    return [bias_edge(op, ch, s, refused) for op, ch in BIAS_EDGE_CHANNELS.items() for s in (1, -1)]


def fp32_edge(op=5, ch=2, sign=1, refused=False):
    """a blob every integer rounding admits and YF_ROUND_FP32 refuses (refused=True), and its twin on the admitted side of the channel's own bound"""
    a = model().fp32_acc_bound(op, ch)
    assert a + 1 < ACC_LIMIT
    v = bias_edge(op, ch, sign, acc_max=a + 1 if refused else a)
    v.name = f"fp32_edge-conv2d_{op}-ch{ch}-{'pos' if sign > 0 else 'neg'}{'-refused' if refused else ''}"
    v.family, v.refused = "fp32_edge", False           # the integer roundings admit both twins
    return v


def all_admitted():
    """every variant the integer roundings admit, in a fixed order"""
    return ([jitter(1), jitter(2)] + [amplify(op) for op in CONV_OPS] + bias_edges() + [uniform(op, v) for op in CONV_OPS for v in (0, 127, -128)] +
            [permute(op) for op in CONV_OPS])


# ---- frames -------------------------------------------------------------------------------------------------------------------------
def structured_extreme_frames(m=None):
    """Frames built to drive accumulators and requantisation to their edges rather than to look like images: the eight corner colours, stripes and
    checkerboards of +127 / -128 at periods 1, 2, 4 and 7 (stride-2 layers see them in and out of phase), single hot and cold pixels at the borders and
    corners (the halo / padding paths), frames matched to the SIGN of the shipped conv2d_1's weights for each of its eight output channels (the largest
    accumulators that layer can produce, both signs), and per-pixel random extremes.  m: the shipped model as load_yfm gives it."""
    if m is None:
        m = model().yfm
    frames = []
    for r in (-128, 127):
        for g in (-128, 127):
            for b in (-128, 127):
                frames.append(np.broadcast_to(np.array([r, g, b], np.int8), (56, 56, 3)).copy())
    yy, xx = np.mgrid[0:56, 0:56]
    for period in (1, 2, 4, 7):
        for pat in ((xx // period) % 2, (yy // period) % 2, ((xx // period) + (yy // period)) % 2):
            f = np.where(pat[..., None] == 1, 127, -128).astype(np.int8)
            frames += [np.broadcast_to(f, (56, 56, 3)).copy(), (-1 - np.broadcast_to(f, (56, 56, 3))).astype(np.int8)]
    for (y, x) in ((0, 0), (0, 55), (55, 0), (55, 55), (0, 27), (27, 0), (55, 28), (28, 55), (27, 27)):
        for base, hot in ((-128, 127), (127, -128), (0, 127)):
            f = np.full((56, 56, 3), base, np.int8)
            f[y, x] = hot
            frames.append(f)
    conv1 = next(o for o in m["ops"] if o["op"] == 3)                            # CONV_2D #1: conv2d_1, 3x3 stride 2 behind the explicit top/left PAD
    w = np.asarray(m["tensors"][conv1["ins"][1]]["data"]).reshape(8, 3, 3, 3)   # OHWI int8
    ky = np.where((np.arange(56) + 1) % 2 == 1, 1, 0)                             # input row y is padded row y + 1: odd -> the window's middle tap, even -> its first
    for o in range(8):
        for sign in (1, -1):
            t = w[o][ky][:, ky].astype(np.int32) * sign                           # [56, 56, 3]: the weight each input value meets in (one of) its windows
            frames.append(np.where(t >= 0, 127, -128).astype(np.int8))
    rng = np.random.default_rng(99)
    frames += list(np.where(rng.integers(0, 2, (12, 56, 56, 3)) == 1, 127, -128).astype(np.int8))
    return np.stack(frames)


def variant_frames():
    """The frame set of the variant tests: the structured extreme frames, 14 seeded random frames (two of them low contrast) and the six golden inputs:
    one ragged (odd) batch, small enough for the one-frame-per-workgroup path."""
    rng = np.random.default_rng(4242)
    r = rng.integers(-128, 128, (14, 56, 56, 3), dtype=np.int8)
    r[12:] //= 16
    golden = np.fromfile(os.path.join(ROOT, "tests", "golden", "golden_inputs.bin"), np.int8).reshape(-1, 56, 56, 3)
    x = np.concatenate([structured_extreme_frames(), r, golden])
    assert x.shape[0] % 2 == 1 and x.shape[0] <= 512
    return x


def band_edge_frames_160():
    """The frames of test_160x160_band_edges (tests/test_gpu_parity.py): structure ON the cuts between the row bands of the 160x160 kernels."""
    frames = []
    for cut in (32, 64, 96, 128):
        for dy in (-2, -1, 0, 1):
            f = np.full((160, 160, 3), -128, np.int8)
            f[cut + dy, :, :] = 127                                           # one hot row next to / on a band cut
            frames.append(f)
        f = np.full((160, 160, 3), 127, np.int8)
        f[cut - 3:cut + 3, 40:43, :] = -128                                   # a short cold bar across the cut
        f[cut - 1, 0, :] = -128; f[cut, 159, :] = -128                        # ... and cold pixels on the cut at both borders
        frames.append(f)
    for y, x in ((0, 0), (0, 159), (159, 0), (159, 159), (0, 80), (159, 79), (80, 0), (79, 159)):
        f = np.zeros((160, 160, 3), np.int8)
        f[y, x] = (127, -128, 127)
        frames.append(f)
    yy = np.arange(160)[:, None, None]
    for period in (8, 16, 32):
        frames.append(np.broadcast_to(np.where((yy // period) % 2 == 1, 127, -128), (160, 160, 3)).astype(np.int8).copy())
        frames.append(np.broadcast_to(np.where(((yy + period // 2) // period) % 2 == 1, 127, -128), (160, 160, 3)).astype(np.int8).copy())
    rng = np.random.default_rng(160)
    for band in range(5):
        f = np.full((160, 160, 3), 3, np.int8)
        f[32 * band:32 * band + 32] = rng.integers(-128, 128, (32, 160, 3), dtype=np.int8)      # noise inside one band only
        frames.append(f)
    return np.stack(frames)


def reuse_frames_160(n=1024, seed=160):
    """The frames of the workgroup-reuse tests at 160x160 (tests/test_band160_reuse_host.py, tests/test_band160_reuse_gpu.py): n frames whose heads are
    pairwise distinct under every rounding, so that a frame in the wrong slot, a band taken from another frame or a row left over from the previous job of
    a workgroup shows.  Frame k has kind k % 4 -- 0: band_edge_frames_160()[(k // 4) % 39] with an 8x8 patch of noise at a random place; 1: a constant frame
    at a random level with noise in one of the five 32-row bands; 2: noise; 3: low-contrast noise (// 16).  All draws from one generator, in frame order."""
    rng = np.random.default_rng(seed)
    edges = band_edge_frames_160()
    out = np.empty((n, 160, 160, 3), np.int8)
    for k in range(n):
        kind = k % 4
        if kind == 0:
            out[k] = edges[(k // 4) % edges.shape[0]]
            y0, x0 = (int(v) for v in rng.integers(0, 152, 2))
            out[k, y0:y0 + 8, x0:x0 + 8] = rng.integers(-128, 128, (8, 8, 3), dtype=np.int8)
        elif kind == 1:
            out[k] = rng.integers(-128, 128)
            band = int(rng.integers(0, 5))
            out[k, 32 * band:32 * band + 32] = rng.integers(-128, 128, (32, 160, 3), dtype=np.int8)
        elif kind == 2:
            out[k] = rng.integers(-128, 128, (160, 160, 3), dtype=np.int8)
        else:
            out[k] = (rng.integers(-128, 128, (160, 160, 3)) // 16).astype(np.int8)
    return out


# ---- the 160x160 band kernels' schedule, restated ---------------------------------------------------------------------------------------
# csrc/yf_band160.hip.h: each band kernel is a persistent grid; workgroup b takes jobs b, b + grid, b + 2 grid, ... below n * (jobs per frame) and split_job
# maps a job number to (frame, band) in the XCD-grouped order when grid % 8 == 0 and n % 8 == 0, in the plain order otherwise.  csrc/yf_engine.hip
# (launch160_banded): grid = min(jobs, CUs x resident workgroups per CU); the static_asserts beside K1_LDS / K23_LDS / K4_LDS bound the residents by 2.
BAND_KERNELS = ("band_k1", "band_k23", "band_k4")
BAND_JOBS_PER_FRAME = (5, 5, 1)
BAND_MAX_WGS_PER_CU = 2


def band_grids(n, bands, cus):
    """the grids launch160_banded can choose for n frames on a device of `cus` CUs: one or two resident workgroups per CU"""
    return sorted({min(n * bands, cus * occ) for occ in range(1, BAND_MAX_WGS_PER_CU + 1)})


def band_xcd_order(n, grid):
    return grid % 8 == 0 and n % 8 == 0


def band_split_job(v, xcd, bands):
    """split_job: job number -> (frame, band)"""
    if xcd:
        l = v >> 3
        q = l // bands
        return (v & 7) + 8 * q, l - q * bands
    return v // bands, v - (v // bands) * bands


def band_walk(n, bands, grid, xcd=None):
    """[workgroup][round] -> (frame, band): the jobs of every workgroup in the order it takes them (xcd None: the order the kernel takes)"""
    xcd = band_xcd_order(n, grid) if xcd is None else xcd
    return [[band_split_job(v, xcd, bands) for v in range(b, n * bands, grid)] for b in range(grid)]


def band_locate(n, bands, grid, frame, band):
    """(workgroup, round) that computes band `band` of frame `frame`: the inverse of band_split_job in the order the kernel takes"""
    if band_xcd_order(n, grid):
        v = (((frame >> 3) * bands + band) << 3) | (frame & 7)
    else:
        v = frame * bands + band
    assert band_split_job(v, band_xcd_order(n, grid), bands) == (frame, band)
    return v % grid, v // grid


def run_160_after_complement(torch, network, d_x, n, canary=77, stream=None):
    """Heads [n, 20, 20, 18] of the first n frames of the device tensor d_x through the 160x160 path.  The same count of the frames' bitwise complements
    is launched first, on the same stream into a scratch output: the per-stream HBM arena outlives a launch, so a band row that a kernel fails to write
    is then read back as ANOTHER frame's values, not as the right ones an earlier launch of the same frames left.  The output has a canary frame behind
    the batch, asserted untouched."""
    d_scratch = torch.empty((n, 20, 20, 18), dtype=torch.int8, device="cuda")
    d_out = torch.full((n + 1, 20, 20, 18), canary, dtype=torch.int8, device="cuda")
    d_not = torch.bitwise_not(d_x[:n])
    torch.cuda.synchronize()
    network.run_device_hw(160, 160, d_not.data_ptr(), d_scratch.data_ptr(), n, stream)
    network.run_device_hw(160, 160, d_x.data_ptr(), d_out.data_ptr(), n, stream)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert (got[n] == canary).all(), f"n = {n}: wrote past the last frame"
    return got[:n]


# ---- the oracle's per-op dump ---------------------------------------------------------------------------------------------------------
def dump_layout(h=56):
    """(sizes, offsets, shapes) of the oracle's per-op dump at 56x56: op i's output is dump[:, offs[i]:offs[i] + sizes[i]], shaped shapes[i] = (h, w, c)."""
    m = model().yfm
    shapes = [tuple(m["tensors"][o["out"]]["shape"][1:]) for o in m["ops"]]
    sizes = [int(np.prod(s)) for s in shapes]
    return sizes, np.concatenate([[0], np.cumsum(sizes)]), shapes


def producer_op(tensor):
    return next(i for i, o in enumerate(model().yfm["ops"]) if o["out"] == tensor)


def lut_input_producers():
    """LUT id -> the tflite op that PRODUCES the tensor indexing it (its values + 128 are the indices the LUT is read at)"""
    ops = model().yfm["ops"]
    return {lid: producer_op(ops[op]["ins"][0]) for lid, op in LUT_INPUT_OP.items()}


def first_difference(got, ref, shape):
    """(frame, y, x, channel, got, ref) of the first differing byte of two [n, h*w*c] arrays, or None"""
    bad = np.argwhere(got.reshape((-1,) + tuple(shape)) != ref.reshape((-1,) + tuple(shape)))
    if not bad.shape[0]:
        return None
    f, y, x, c = (int(v) for v in bad[0])
    return f, y, x, c, int(got.reshape((-1,) + tuple(shape))[f, y, x, c]), int(ref.reshape((-1,) + tuple(shape))[f, y, x, c])
