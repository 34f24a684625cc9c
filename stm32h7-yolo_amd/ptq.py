"""Post-training quantisation arithmetic -- host-side mirror of the reference's `yoloface/tflite/tflite_quantize.py:29-96`.

The reference produces `yoloface_int8.tflite` with the TFLite converter (`tf.lite.TFLiteConverter`, DEFAULT optimisation,
int8 builtins, representative dataset = `small_dataset/*.jpg` resized to 56x56 and divided by 255).  TensorFlow is not
available here; this module restates the converter's published quantisation rules so the constants the engine consumes
(`yf_host_prep.c`) can be regenerated from a float model and a calibration set:

  * weights      per output channel, symmetric, narrow range:  s_c = max|w_c| / 127,  q = clip(round(w / s_c), -127, 127)
  * bias         int32,  q = round(b / (s_in * s_c))            (scale s_in * s_c, zero point 0)
  * activations  asymmetric int8 over the calibrated [min, max], range extended to contain 0:
                 s = (max - min) / 255,  zp = clip(round(-128 - min / s), -128, 127)
  * MAX_POOL_2D keeps the parameters of its input; CONCATENATION inputs are requantised to the output's parameters
    (the QUANTIZE ops of the int8 graph)

`tests/test_ptq.py` checks the first two rules EXACTLY against the reference's two model files (every int8 weight and every
int32 bias of `yoloface_int8.tflite` is reproduced from the float weights of `yoloface.tflite`), and the third by calibrating
on the reference's representative dataset prepared as its script prepares it (`resize_linear_u8` restates OpenCV's
INTER_LINEAR resize, which is what makes the difference: PIL's antialiased resize left the first layers 10-27 % off): every
activation zero point and 42 of 46 scales are reproduced (float32 rounding noise), four scales within 0.8 %.
This is an offline tool; it is not on the inference path.

`clip_ranges` chooses a clipped range per tensor from a histogram of its values over the calibration frames (calib.Calibration.histogram
or calib.host_histogram: csrc/yf_calib_hist.h), by percentile or by least modelled quantisation error; min/max stays the default everywhere.

`quantize_model` applies the rules to a whole float model: .yfw bytes and calibrated ranges in, a .yfm image out that yf_network_init_model
admits.  The ranges come from the calibration library (calib.py: the float32 evaluation on the GPU, or its host build).
"""
import functools

import numpy as np

from . import model_file

INPUT_SCALE_BITS, INPUT_ZERO_POINT = 0x3B808081, -128           # what every frame producer assumes: pixel - 128 in units of 1/255


def quantize_conv_weights(w, channel_axis):
    """float weights -> (int8 weights, float32 per-channel scales).  channel_axis: 0 for CONV_2D (OHWI), 3 for
    DEPTHWISE_CONV_2D (1HWC)."""
    w = np.asarray(w, np.float32)
    axes = tuple(k for k in range(w.ndim) if k != channel_axis)
    scale = (np.abs(w).max(axis=axes) / np.float32(127.0)).astype(np.float32)
    shape = [1] * w.ndim
    shape[channel_axis] = -1
    safe = np.where(scale == 0, np.float32(1), scale).reshape(shape)
    q = np.clip(np.round(w / safe), -127, 127).astype(np.int8)
    return q, scale


def quantize_bias(b, s_in, s_w):
    """float bias -> int32 with scale s_in * s_w[c] (evaluated in double, as the converter does)."""
    scale = np.float64(np.float32(s_in)) * np.asarray(s_w, np.float32).astype(np.float64)
    return np.round(np.asarray(b, np.float32).astype(np.float64) / scale).astype(np.int64).astype(np.int32)


def activation_qparams(rmin, rmax):
    """calibrated range -> (float32 scale, int zero point) for an int8 activation tensor."""
    rmin, rmax = min(float(rmin), 0.0), max(float(rmax), 0.0)
    if rmax == rmin:
        return np.float32(1.0), 0
    scale = (rmax - rmin) / 255.0
    zp = int(np.clip(np.round(-128.0 - rmin / scale), -128, 127))
    return np.float32(scale), zp


def quantize_model(yfw_bytes, ranges):
    """Float weights (.yfw bytes, model_file.read_yfw) and calibrated ranges {tensor id: (min, max)} -> the bytes of a .yfm image.
    The graph is the library's (model_file.load_graph: csrc/gen/yf_graph_gen.h); only the numbers are new:
      * filters by quantize_conv_weights, biases by quantize_bias on the scale finally assigned to the convolution's input;
      * every CONV_2D, DEPTHWISE_CONV_2D, LEAKY_RELU and ADD output by activation_qparams of its own range;
      * the input pinned to (0x3b808081, -128), the bits the frame producers assume;
      * a CONCATENATION output by the union of its inputs' ranges (a QUANTIZE or MAX_POOL_2D output's range is the range observed for the
        pool's output), and EVERY input of a CONCATENATION -- a QUANTIZE output or a tensor wired in directly -- carries the output's parameters;
      * PAD and MAX_POOL_2D outputs carry their input's parameters.
    `ranges` must hold the input, every convolution, LeakyReLU and ADD output and the two pool outputs (calib.Calibration.ranges()).
    A filter channel that is all zero would get scale 0, which no parser admits: ValueError names the convolution and the channel.
    A range with an end that is not finite, or with min above max, is refused before anything is computed: ValueError names the tensor and
    the two ends.  Calibration hands over such a range when the float network overflowed on the frames (an infinite end), and (+inf, -inf),
    the value a slot starts from, for a tensor that was NaN at every element."""
    O = model_file.OPCODE
    ranges = {int(k): (float(v[0]), float(v[1])) for k, v in ranges.items()}
    for t in sorted(ranges):
        lo, hi = ranges[t]
        if not (np.isfinite(lo) and np.isfinite(hi) and lo <= hi):
            raise ValueError(f"ranges: tensor {t}: the range is ({lo}, {hi}), expected two finite numbers with min <= max: the float network "
                             f"overflowed, or computed nothing but NaN, on the calibration frames")
    convs = model_file.read_yfw(yfw_bytes)
    g = model_file.load_graph()
    T, ops = g["tensors"], g["ops"]
    producer = {o["out"]: o for o in ops}

    def range_of(t):
        """the range of the values tensor t holds: observed, or that of the tensor a QUANTIZE copies"""
        while t not in ranges:
            o = producer.get(t)
            if o is None or o["op"] != O["QUANTIZE"]:
                raise ValueError(f"ranges: tensor {t} is missing")
            t = o["ins"][0]
        return ranges[t]

    q = {g["input"]: (np.array([INPUT_SCALE_BITS], "<u4").view("<f4")[0], INPUT_ZERO_POINT)}
    for o in ops:
        if o["op"] in (O["CONV_2D"], O["DEPTHWISE_CONV_2D"], O["LEAKY_RELU"], O["ADD"]):
            q[o["out"]] = activation_qparams(*range_of(o["out"]))
        elif o["op"] == O["CONCATENATION"]:
            r = [range_of(t) for t in o["ins"][:2]]
            q[o["out"]] = activation_qparams(min(r[0][0], r[1][0]), max(r[0][1], r[1][1]))
    for o in ops:
        if o["op"] == O["CONCATENATION"]:
            for t in o["ins"][:2]:
                q[t] = q[o["out"]]
    for o in ops:                                   # (in op order: a PAD or pool behind a tensor whose parameters were just replaced follows it)
        if o["op"] in (O["PAD"], O["MAX_POOL_2D"]):
            q[o["out"]] = q[o["ins"][0]]
    for t, (scale, zp) in q.items():
        T[t]["scale"], T[t]["zp"] = np.array([scale], "<f4"), int(zp)
    for c, (d, (w, b, dw)) in enumerate(zip(model_file.graph_convs(g), convs)):
        o = ops[d["op"]]
        wq, s_w = quantize_conv_weights(w, 3 if dw else 0)
        if (s_w == 0).any():
            raise ValueError(f"conv {c} (op {d['op']}): filter channel {int(np.argmax(s_w == 0))} is all zero: its scale would be 0")
        s_in = T[o["ins"][0]]["scale"][0]
        wt, bt = T[o["ins"][1]], T[o["ins"][2]]
        wt["scale"], wt["data"] = s_w.astype("<f4"), wq.reshape(-1)
        bt["scale"] = (np.float64(np.float32(s_in)) * s_w.astype(np.float64)).astype("<f4")
        bt["data"] = quantize_bias(b, s_in, s_w).astype("<i4")
    missing = [i for i, t in enumerate(T) if len(t["scale"]) != t["n_scales"] or (t["data"] is None) == t["is_const"]]
    if missing:
        raise ValueError(f"tensors {missing} were left without numbers")
    return model_file.write_yfm(g)


def dequantized_yfw(yfw_bytes, yfm_bytes, convs=None):
    """.yfw bytes in which the convolutions listed in `convs` (indices in graph order; None: all) carry the numbers the int8 model
    `yfm_bytes` gives them, dequantised: w = float32(q) * s_c (one float32 multiply), b = float32(double(q) * double(s_bias)).  The others
    keep the float values of `yfw_bytes`; with no convolution listed the input bytes come back unchanged."""
    g = model_file.graph_convs()
    which = range(len(g)) if convs is None else sorted({int(c) for c in convs})
    bad = [c for c in which if not 0 <= c < len(g)]
    if bad:
        raise ValueError(f"convs: {bad}, expected indices 0 to {len(g) - 1}")
    if not len(which):
        return bytes(yfw_bytes)
    out = list(model_file.read_yfw(yfw_bytes))
    m = model_file.load_yfm(yfm_bytes)
    T, ops = m["tensors"], m["ops"]
    for c in which:
        d = g[c]
        wt, bt = T[ops[d["op"]]["ins"][1]], T[ops[d["op"]]["ins"][2]]
        shape = [1, 1, 1, 1]
        shape[3 if d["depthwise"] else 0] = -1
        w = wt["data"].reshape(d["shape"]).astype(np.float32) * wt["scale"].astype(np.float32).reshape(shape)
        b = (bt["data"].astype(np.float64) * bt["scale"].astype(np.float32).astype(np.float64)).astype(np.float32)
        out[c] = (w.astype(np.float32), b, d["depthwise"])
    return model_file.write_yfw(out)


def with_biases(yfw_bytes, biases):
    """.yfw bytes with the same weights and the given biases: `biases` has one item per convolution in graph order -- float32 [cout], or None
    for a convolution that keeps its bias -- or is a dict {convolution: bias}.  A bias of another length or with a value that is not finite
    raises ValueError naming the convolution."""
    convs = list(model_file.read_yfw(yfw_bytes))
    if isinstance(biases, dict):
        bad = [c for c in biases if not 0 <= int(c) < len(convs)]
        if bad:
            raise ValueError(f"biases: convolutions {sorted(bad)}, expected indices 0 to {len(convs) - 1}")
        biases = [biases.get(c) for c in range(len(convs))]
    if len(biases) != len(convs):
        raise ValueError(f"biases: {len(biases)} items, expected one per convolution ({len(convs)})")
    for c, b in enumerate(biases):
        if b is None:
            continue
        b = np.asarray(b, np.float32).reshape(-1)
        if b.size != convs[c][1].size or not np.isfinite(b).all():
            raise ValueError(f"biases: conv {c}: {b.size} values{'' if np.isfinite(b).all() else ', not all finite'}, expected {convs[c][1].size} "
                             f"finite float32")
        convs[c] = (convs[c][0], b, convs[c][2])
    return model_file.write_yfw(convs)


CLIP_METHODS = ("minmax", "percentile", "mse")


def choose_ranges(candidates, errors):
    """{tensor: [range, ...]} and {tensor: [error of each candidate]} -> {tensor: the candidate with the least error}; ties go to the earlier
    candidate (a candidate replaces the choice only when its error is strictly below it, so a NaN never wins).  What
    calib.quantize_on_device(..., ranges="head") chooses with, the candidates being the "minmax", "percentile" and "mse" ranges in that order
    and the errors the head's squared error when that tensor alone is quantised."""
    out = {}
    for t, cands in candidates.items():
        e = list(errors[t])
        if len(e) != len(cands) or not len(cands):
            raise ValueError(f"tensor {t}: {len(cands)} candidates and {len(e)} errors")
        best = 0
        for i in range(1, len(e)):
            if e[i] < e[best]:
                best = i
        out[t] = (float(cands[best][0]), float(cands[best][1]))
    return out


def _edges(lo, hi, bins):
    """edge[k] = min + k * (max - min) / bins in float64: bin k of the histogram spans edge[k] .. edge[k + 1]"""
    return lo + np.arange(bins + 1, dtype=np.float64) * (hi - lo) / bins


def _clipped(lo, hi, edges, a, b):
    """the range with `a` leading and `b` trailing bins cut: a bound that is not cut is the given one, unchanged"""
    bins = len(edges) - 1
    return (lo if a == 0 else float(edges[a]), hi if b == 0 else float(edges[bins - b]))


def clip_error(counts, lo, hi, rmin, rmax):
    """The modelled error of quantising a tensor whose histogram over [lo, hi] is `counts` with activation_qparams(rmin, rmax):
    sum_k n_k * (dequant(quant(c_k)) - c_k)^2 over the bin centres c_k, quantised with round-half-even and clipped to -128..127.  float64."""
    n = np.asarray(counts).astype(np.float64)
    e = _edges(float(lo), float(hi), n.size)
    return _centre_error(n, (e[:-1] + e[1:]) / 2, rmin, rmax)


def _centre_error(n, c, rmin, rmax):
    scale, zp = activation_qparams(rmin, rmax)
    scale = float(scale)
    q = np.clip(np.rint(c / scale) + zp, -128, 127)
    return float((n * ((q - zp) * scale - c) ** 2).sum())


def clip_ranges(counts, ranges, method, percentile=0.9999, keep=(0,)):
    """Clipped calibration ranges from histograms: counts [47, bins] (row i belongs to the i-th tensor id of `ranges` in ascending order,
    the slot order of yf_calib_ranges), ranges {tensor: (min, max)} the axes of the histograms were built from -> {tensor: (min, max)}.
      "minmax"      `ranges`, unchanged.
      "percentile"  tail = floor((1 - percentile) / 2 * total); `a` is the largest number of leading bins whose summed count is <= tail, `b`
                    the same from the trailing end; the range is edge[a] .. edge[bins - b].  A bound with a == 0 (b == 0) is the given
                    one, unchanged, so percentile=1.0 over the frames the ranges came from changes nothing.  If a + b >= bins the range is
                    the one fullest bin.
      "mse"         the candidate (a, b), a and b multiples of max(1, bins // 64) up to bins / 2, with the least clip_error; ties go to the
                    smaller a + b, then to the smaller a.  (0, 0) is a candidate: the error is never above min/max's.
    The tensors of `keep` are never clipped (the default: the input, whose parameters quantize_model pins anyway), nor is a tensor whose
    histogram is empty.  Host, numpy, float64: an offline step."""
    if method not in CLIP_METHODS:
        raise ValueError(f"method: {method!r}, expected one of {CLIP_METHODS}")
    ranges = {int(t): (float(v[0]), float(v[1])) for t, v in ranges.items()}
    if method == "minmax":
        return ranges
    counts = np.asarray(counts)
    ids = sorted(ranges)
    if counts.ndim != 2 or counts.shape[0] != len(ids) or counts.shape[1] < 1:
        raise ValueError(f"counts: shape {counts.shape}, expected [{len(ids)}, bins], one row per tensor of `ranges`")
    if not 0.0 <= percentile <= 1.0:
        raise ValueError(f"percentile: {percentile}, expected 0 to 1")
    bins, keep, out = counts.shape[1], {int(t) for t in keep}, {}
    if method == "mse":
        # (with an even `bins` the grid reaches a = b = bins / 2, a range of no width: activation_qparams widens every range to hold 0 and gives
        # (1.0, 0) for {0, 0}, so such a candidate has a finite error like any other and never wins against one that keeps values)
        step = max(1, bins // 64)
        grid = [k for k in range(0, bins + 1, step) if 2 * k <= bins]
        cands = sorted(((a, b) for a in grid for b in grid), key=lambda ab: (ab[0] + ab[1], ab[0]))
    for t, row in zip(ids, counts):
        lo, hi = ranges[t]
        total = int(row.astype(np.uint64).sum())
        if t in keep or total == 0:
            out[t] = (lo, hi)
            continue
        edges = _edges(lo, hi, bins)
        if method == "percentile":
            tail = int(np.floor((1.0 - percentile) / 2.0 * total))
            a = int(np.searchsorted(np.cumsum(row.astype(np.float64)), tail, side="right"))
            b = int(np.searchsorted(np.cumsum(row[::-1].astype(np.float64)), tail, side="right"))
            if a + b >= bins:
                k = int(np.argmax(row))
                out[t] = (float(edges[k]), float(edges[k + 1]))
            else:
                out[t] = _clipped(lo, hi, edges, a, b)
        else:
            n, c = row.astype(np.float64), (edges[:-1] + edges[1:]) / 2
            errors = [_centre_error(n, c, *_clipped(lo, hi, edges, a, b)) for a, b in cands]
            out[t] = _clipped(lo, hi, edges, *cands[int(np.argmin(errors))])
    return out


class Calibrator:
    """Running min/max per named tensor over a representative dataset (TFLite calibration keeps the extremes over all
    samples)."""

    def __init__(self):
        self.ranges = {}

    def observe(self, name, value):
        v = np.asarray(value)
        lo, hi = float(v.min()), float(v.max())
        if name in self.ranges:
            a, b = self.ranges[name]
            lo, hi = min(lo, a), max(hi, b)
        self.ranges[name] = (lo, hi)

    def qparams(self, name):
        return activation_qparams(*self.ranges[name])


@functools.lru_cache(maxsize=4096)
def _resize_axis(n_out, n_in):
    """the source index and the two 11-bit weights of every output index of one axis of `resize_linear_u8` (read-only arrays)"""
    scale = np.float64(n_in) / n_out
    idx, c0, c1 = np.zeros(n_out, np.int64), np.zeros(n_out, np.int64), np.zeros(n_out, np.int64)
    for d in range(n_out):
        f = np.float32((d + 0.5) * scale - 0.5)                        # OpenCV computes this in float
        s = int(np.floor(f))
        f = np.float32(f - s)
        if s < 0:
            s, f = 0, np.float32(0)
        if s >= n_in - 1:
            s, f = n_in - 1, np.float32(0)
        # saturate_cast<short>(float) = cvRound: round half to even
        c0[d] = int(np.rint(np.float32((np.float32(1) - f) * np.float32(2048))))
        c1[d] = int(np.rint(np.float32(f * np.float32(2048))))
        idx[d] = s
    for a in (idx, c0, c1):
        a.setflags(write=False)
    return idx, c0, c1


def resize_linear_u8(img, out_w, out_h):
    """OpenCV's `cv2.resize(img, (out_w, out_h))` (INTER_LINEAR, the default) for uint8 images [H, W, C], restated from the
    published algorithm (imgproc/resize.cpp: pixel centres aligned -- src = (dst + 0.5) * scale - 0.5 --, NO antialiasing,
    fixed-point weights of 11 bits per axis):
        horizontal pass  row[x] = S[sx] * a0 + S[sx + 1] * a1              a0 + a1 = 2048 (int16 weights, round half even)
        vertical pass    dst = ( ((b0 * (row0 >> 4)) >> 16) + ((b1 * (row1 >> 4)) >> 16) + 2 ) >> 2
    The reference's calibration images go through exactly this call (tflite_quantize.py:45-52)."""
    src = np.asarray(img, np.uint8)
    h, w = src.shape[:2]
    src = src.reshape(h, w, -1).astype(np.int64)

    xi, xa0, xa1 = _resize_axis(int(out_w), int(w))
    yi, yb0, yb1 = _resize_axis(int(out_h), int(h))
    xi1 = np.minimum(xi + 1, w - 1)
    rows = src[:, xi, :] * xa0[None, :, None] + src[:, xi1, :] * xa1[None, :, None]          # [H, out_w, C], int32 range
    yi1 = np.minimum(yi + 1, h - 1)
    r0, r1 = rows[yi], rows[yi1]
    out = (((yb0[:, None, None] * (r0 >> 4)) >> 16) + ((yb1[:, None, None] * (r1 >> 4)) >> 16) + 2) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


def letterbox_fit(h, w, size):
    """Where a picture of `h` x `w` lies in a letterboxed frame of side `size`, as csrc/yf_images_fit.h states it, in Python integers:
    -> (x0, y0, width, height).  The longer side becomes `size`, the other one the exact ratio rounded HALF UP (at least 1):
    (2 * h * size + w) // (2 * w) for w >= h; the rectangle is centred with the odd pixel of padding right and bottom (floor), as
    ultralytics' LetterBox centres it.  The rounding is the library's choice: Python's `round` differs from it at exact halves only,
    where it rounds to even."""
    h, w, size = int(h), int(w), int(size)
    fw = fh = size
    if w > h:
        fh = max(1, (2 * h * size + w) // (2 * w))
    elif h > w:
        fw = max(1, (2 * w * size + h) // (2 * h))
    return (size - fw) // 2, (size - fh) // 2, fw, fh


def letterbox_u8(img_hwc, size, pad=114, interp="linear"):
    """The letterboxed frame of a uint8 picture [H, W, C]: `resize_linear_u8` (interp="area": `resize_area_u8`) to the rectangle of
    `letterbox_fit`, the rest of the [size, size, C] frame filled with `pad` (0..255; the trainers' grey is 114) in every channel ->
    uint8 [size, size, C]."""
    src = np.asarray(img_hwc, np.uint8)
    if src.ndim != 3:
        raise ValueError(f"expected uint8 [H, W, C], got {src.shape}")
    if not 0 <= int(pad) <= 255:
        raise ValueError(f"pad {pad!r}: 0 to 255")
    if interp not in ("linear", "area"):
        raise ValueError(f"interp {interp!r}: 'linear' or 'area'")
    x0, y0, fw, fh = letterbox_fit(src.shape[0], src.shape[1], size)
    out = np.full((int(size), int(size), src.shape[2]), int(pad), np.uint8)
    out[y0:y0 + fh, x0:x0 + fw] = resize_linear_u8(src, fw, fh) if interp == "linear" else resize_area_u8(src, fh, fw)
    return out


@functools.lru_cache(maxsize=256)
def _area_axis(n_out, n_in):
    """int64 [n_out, n_in]: a(d, s), the overlap of output d's [d n_in, (d + 1) n_in) with source s's [s n_out, (s + 1) n_out) on the
    grid of n_in * n_out sub-positions (read-only)"""
    d = np.arange(n_out, dtype=np.int64)[:, None]
    s = np.arange(n_in, dtype=np.int64)[None, :]
    a = np.maximum(0, np.minimum((d + 1) * n_in, (s + 1) * n_out) - np.maximum(d * n_in, s * n_out))
    a.setflags(write=False)
    return a


def resize_area_u8(img, out_h, out_w):
    """The exact area average of a uint8 picture [H, W, C] at [out_h, out_w, C], as csrc/yf_images_area.h states it, in integers: every
    source pixel counted with the share of it an output pixel covers.  Per axis a(d, s) = the overlap of [d n_in, (d + 1) n_in) and
    [s n_out, (s + 1) n_out) (an integer; the a(d, .) sum to n_in); per output pixel and channel
        S = sum ay(y, sy) ax(x, sx) p[sy][sx],   v = (2 S + H W) // (2 H W)          rounded half up
    for any ratio -- reduction, enlargement, identity.  For integer ratios this is the rounded block mean, the result of the integer path
    of cv2.resize(..., interpolation=cv2.INTER_AREA); elsewhere OpenCV accumulates float weights and this is the value they approximate.
    Not pinned against a real cv2.  (Note the order (out_h, out_w); `resize_linear_u8` keeps cv2's (out_w, out_h).)"""
    src = np.asarray(img, np.uint8)
    h, w = src.shape[:2]
    src = src.reshape(h, w, -1).astype(np.int64)
    ay, ax = _area_axis(int(out_h), int(h)), _area_axis(int(out_w), int(w))
    rows = np.einsum("xs,hsc->hxc", ax, src)                     # [H, out_w, C]: at most 255 * W
    total = np.einsum("yh,hxc->yxc", ay, rows)                   # at most 255 * H * W, about 6.8e10
    d = np.int64(h) * np.int64(w)
    return ((2 * total + d) // (2 * d)).astype(np.uint8)


def yuv420sp_to_rgb_u8(y, uv, v_first=False):
    """OpenCV's `cv2.cvtColor(yuv, cv2.COLOR_YUV2RGB_NV12)` (v_first: `_NV21`) for a 4:2:0 semi-planar surface, restated from the published
    algorithm (imgproc/src/color_yuv.simd.hpp, YUV420sp -> RGB: BT.601 limited range in 20-bit fixed point) and, like `resize_linear_u8`,
    not pinned against a real cv2.  `y` uint8 [H, W], `uv` uint8 [H / 2, W] of byte pairs (U, V; v_first: V, U), H and W even -> uint8
    [H, W, 3] in RGB order (`[..., ::-1]` is COLOR_YUV2BGR_*).  Pixel (r, c) takes the pair of UV row r >> 1 at columns 2 * (c >> 1), + 1;
    chroma is not interpolated.  int32 suffices (the largest magnitude is about 5.6e8); `>>` of a negative is arithmetic.
        yy = max(0, Y - 16) * 1220542;  uu = U - 128;  vv = V - 128
        R = clamp8((yy + (1 << 19) + 1673527 * vv) >> 20)
        G = clamp8((yy + (1 << 19) - 852492 * vv - 409993 * uu) >> 20)
        B = clamp8((yy + (1 << 19) + 2116026 * uu) >> 20)"""
    y, uv = np.asarray(y), np.asarray(uv)
    if y.dtype != np.uint8 or uv.dtype != np.uint8 or y.ndim != 2 or uv.ndim != 2:
        raise ValueError(f"expected uint8 planes [H, W] and [H / 2, W], got {y.dtype} {y.shape} and {uv.dtype} {uv.shape}")
    h, w = y.shape
    if h % 2 or w % 2 or uv.shape != (h // 2, w):
        raise ValueError(f"Y plane {y.shape}, UV plane {uv.shape}: even sides and a UV plane of [H / 2, W]")
    first = np.repeat(np.repeat(uv[:, 0::2], 2, axis=0), 2, axis=1).astype(np.int32)
    second = np.repeat(np.repeat(uv[:, 1::2], 2, axis=0), 2, axis=1).astype(np.int32)
    uu, vv = ((second, first) if v_first else (first, second))
    uu, vv = uu - 128, vv - 128
    yy = np.maximum(0, y.astype(np.int32) - 16) * np.int32(1220542) + np.int32(1 << 19)
    r = (yy + 1673527 * vv) >> 20
    g = (yy - 852492 * vv - 409993 * uu) >> 20
    b = (yy + 2116026 * uu) >> 20
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def crop_region(box, width, height, margin_permille=0, square=False):
    """The region of a detection's box in a picture of `height` x `width` pixels, as csrc/yf_images_crop.h states it, in Python integers:
    `box` = (x1, y1, x2, y2), inclusive edges.  bw = x2 - x1 + 1, bh likewise, either < 1: no region.  Margin: mx = bw * margin_permille
    // 1000, my likewise; x1 -= mx, x2 += mx, y1 -= my, y2 += my.  `square`: side = max(width, height) of that, x1 -= (side - width) // 2,
    x2 = x1 + side - 1, y likewise.  Clamp to the picture; x1 > x2 or y1 > y2: no region.  The region is not squared again after the
    clamp.  -> (x0, y0, width, height), or None."""
    x1, y1, x2, y2 = (int(v) for v in box)
    bw, bh = x2 - x1 + 1, y2 - y1 + 1
    if bw < 1 or bh < 1:
        return None
    mx, my = bw * int(margin_permille) // 1000, bh * int(margin_permille) // 1000
    x1, x2, y1, y2 = x1 - mx, x2 + mx, y1 - my, y2 + my
    if square:
        w, h = x2 - x1 + 1, y2 - y1 + 1
        side = max(w, h)
        x1 -= (side - w) // 2
        x2 = x1 + side - 1
        y1 -= (side - h) // 2
        y2 = y1 + side - 1
    x1, y1, x2, y2 = max(x1, 0), max(y1, 0), min(x2, int(width) - 1), min(y2, int(height) - 1)
    if x1 > x2 or y1 > y2:
        return None
    return x1, y1, x2 - x1 + 1, y2 - y1 + 1


def crop_resize_u8(img, box, out_w, out_h, margin_permille=0, square=False):
    """The face chip of `box` in `img` (uint8 [H, W, C]): `cv2.resize(img[y0 : y0 + h, x0 : x0 + w], (out_w, out_h))` of the region
    `crop_region` gives, through `resize_linear_u8` -- what yf_images_crop_records_device computes.  A box without a region gives zeros."""
    img = np.asarray(img, np.uint8)
    region = crop_region(box, img.shape[1], img.shape[0], margin_permille, square)
    if region is None:
        return np.zeros((out_h, out_w) + img.shape[2:], np.uint8)
    x0, y0, w, h = region
    return resize_linear_u8(img[y0:y0 + h, x0:x0 + w], out_w, out_h).reshape((out_h, out_w) + img.shape[2:])


def _mosaic_plane(src, out, blocks, kx, ky):
    """every block of `blocks` (a set of (bx, by)) of the plane `out` [rows, cols, channels] gets, per channel, the rounded integer mean
    (sum + cnt // 2) // cnt of the same block of `src`; a block holds kx columns and ky rows, clipped at the plane's right and bottom edge"""
    for bx, by in blocks:
        blk = src[by * ky:by * ky + ky, bx * kx:bx * kx + kx].astype(np.int64)
        cnt = blk.shape[0] * blk.shape[1]
        out[by * ky:by * ky + ky, bx * kx:bx * kx + kx] = (blk.sum(axis=(0, 1)) + cnt // 2) // cnt


def _touched_blocks(regions, block):
    """the union of the blocks of a grid anchored at pixel (0, 0) that the regions (x0, y0, width, height) touch; None: a record without a region"""
    return {(bx, by) for x0, y0, w, h in (r for r in regions if r is not None)
            for bx in range(x0 // block, (x0 + w - 1) // block + 1) for by in range(y0 // block, (y0 + h - 1) // block + 1)}


def _redact_mode(mode, block):
    if mode in ("mosaic", 0) and not isinstance(mode, bool):
        if block not in (4, 8, 16, 32, 64):
            raise ValueError(f"block {block!r}: 4, 8, 16, 32 or 64")
        return True
    if mode in ("fill", 1) and not isinstance(mode, bool):
        if block not in (0, None):
            raise ValueError(f"block {block!r}: the fill has no block (0)")
        return False
    raise ValueError(f"mode {mode!r}: 'mosaic' or 'fill'")


def redact_u8(picture_hwc, regions, mode, block, colour):
    """The redacted copy of a packed picture (uint8 [H, W, 3 or 4]), as csrc/yf_images_redact.h states it.  `regions`: (x0, y0, width,
    height) per record, as `crop_region` gives them (None entries are skipped).
    mode "mosaic", block k in {4, 8, 16, 32, 64}: the block grid is anchored at pixel (0, 0) and clipped at the right and bottom edge; the
    union of the blocks the regions touch is redacted, each block to its rounded integer mean per colour channel, (sum + cnt // 2) // cnt
    over the pixels of the picture as it came in.  mode "fill", block 0: every pixel of every region gets `colour`, three bytes for the
    picture's channels 0, 1, 2 in the picture's own order.  A fourth channel is never touched."""
    src = np.asarray(picture_hwc, np.uint8)
    out = src.copy()
    if _redact_mode(mode, block):
        _mosaic_plane(src[..., :3], out[..., :3], _touched_blocks(regions, block), block, block)
    else:
        for x0, y0, w, h in (r for r in regions if r is not None):
            out[y0:y0 + h, x0:x0 + w, :3] = np.asarray(colour, np.uint8).reshape(3)
    return out


def redact_yuv420sp(y, uv, regions, mode, block, colour, v_first=False):
    """`redact_u8` for an NV12 / NV21 surface (y uint8 [H, W], uv uint8 [H / 2, W]) -> (y, uv) redacted copies.  Mosaic: the luma blocks on
    the Y plane, and for each block of the set the chroma block of the same (bx, by) -- block // 2 pairs by block // 2 rows, clipped to
    W / 2 and H / 2 -- whose first bytes are averaged together and whose second bytes together (v_first does not matter).  Fill: `colour`
    = (Y, U, V); the regions' Y bytes, and the chroma pairs cx in [x0 >> 1, (x0 + width - 1) >> 1], cy in [y0 >> 1, (y0 + height - 1)
    >> 1] get (U, V), or (V, U) with v_first."""
    y_src, uv_src = np.asarray(y, np.uint8), np.asarray(uv, np.uint8)
    y_out, uv_out = y_src.copy(), uv_src.copy()
    h2, w = uv_src.shape
    pairs_src, pairs_out = uv_src.reshape(h2, w // 2, 2), uv_out.reshape(h2, w // 2, 2)
    if _redact_mode(mode, block):
        blocks = _touched_blocks(regions, block)
        _mosaic_plane(y_src[..., None], y_out[..., None], blocks, block, block)
        _mosaic_plane(pairs_src, pairs_out, blocks, block // 2, block // 2)
    else:
        yy, u, v = (int(c) for c in colour)
        for x0, y0, rw, rh in (r for r in regions if r is not None):
            y_out[y0:y0 + rh, x0:x0 + rw] = yy
            pairs_out[y0 >> 1:((y0 + rh - 1) >> 1) + 1, x0 >> 1:((x0 + rw - 1) >> 1) + 1] = (v, u) if v_first else (u, v)
    return y_out, uv_out


# ---- the blur (csrc/yf_images_blur.h), in plain numpy ----
BLUR_MAX_GRID = 16
BLUR_MIN_CELL = 4


def blur_cells(side, grid, min_cell=BLUR_MIN_CELL):
    """the cells along a side of `side` pixels: max(1, min(grid, side // min_cell))"""
    return max(1, min(int(grid), int(side) // min_cell))


def blur_grid_u8(plane_hwc, grid, min_cell=BLUR_MIN_CELL):
    """The grid of means of a region (uint8 [height, width, channels]) -> uint8 [gy, gx, channels]: cell cx holds the columns
    [cx * width // gx, (cx + 1) * width // gx), rows likewise; per cell and channel (sum + cnt // 2) // cnt in exact integers."""
    src = np.asarray(plane_hwc, np.uint8)
    h, w = src.shape[:2]
    gx, gy = blur_cells(w, grid, min_cell), blur_cells(h, grid, min_cell)
    # the prefix sums of the region, int64: a cell's sum is four reads
    acc = np.zeros((h + 1, w + 1, src.shape[2]), np.int64)
    acc[1:, 1:] = src.astype(np.int64).cumsum(axis=0).cumsum(axis=1)
    xs = np.array([c * w // gx for c in range(gx + 1)])
    ys = np.array([c * h // gy for c in range(gy + 1)])
    sums = acc[ys[1:, None], xs[None, 1:]] - acc[ys[:-1, None], xs[None, 1:]] - acc[ys[1:, None], xs[None, :-1]] + acc[ys[:-1, None], xs[None, :-1]]
    cnt = ((ys[1:] - ys[:-1])[:, None] * (xs[1:] - xs[:-1])[None, :])[..., None]
    return ((sums + cnt // 2) // cnt).astype(np.uint8)


def _blur_grid(grid):
    if isinstance(grid, bool) or int(grid) != grid or not 1 <= int(grid) <= BLUR_MAX_GRID:
        raise ValueError(f"grid {grid!r}: 1 to {BLUR_MAX_GRID}")
    return int(grid)


def _blur_plane(src, out, rects, grid, min_cell, colours):
    """every rectangle (x0, y0, width, height) of `rects` (None: no region) of the plane `out` [rows, cols, channels] becomes the grid of
    means of the same rectangle of `src` resized back to it -- or, with colours[k] not None, that colour; a pixel in several rectangles
    gets the value of the first that holds it: they are painted from the last to the first."""
    for k in range(len(rects) - 1, -1, -1):
        if rects[k] is None:
            continue
        x0, y0, w, h = rects[k]
        if colours[k] is not None:
            out[y0:y0 + h, x0:x0 + w] = colours[k]
        else:
            out[y0:y0 + h, x0:x0 + w] = resize_linear_u8(blur_grid_u8(src[y0:y0 + h, x0:x0 + w], grid, min_cell), w, h)


def blur_u8(picture_hwc, regions, grid, colour=None, filled=()):
    """The blurred copy of a packed picture (uint8 [H, W, 3 or 4]), as csrc/yf_images_blur.h states it.  `regions`: (x0, y0, width,
    height) per record, as `crop_region` gives them (None entries are skipped).  Every region becomes `resize_linear_u8` of its own grid
    of means (`blur_grid_u8`: at most grid x grid cells, none narrower than 4 pixels), the means taken from the picture as it came in;
    a pixel in several regions gets the value of the first region that holds it.  `filled`: the indices of the records that get `colour`
    instead (three bytes for the picture's channels 0, 1, 2 in the picture's own order) -- the records without a slot in the workspace.
    A fourth channel is never touched."""
    grid = _blur_grid(grid)
    src = np.asarray(picture_hwc, np.uint8)
    out = src.copy()
    filled = set(filled)
    colours = [np.asarray(colour, np.uint8).reshape(3) if k in filled else None for k in range(len(regions))]
    _blur_plane(src[..., :3], out[..., :3], list(regions), grid, BLUR_MIN_CELL, colours)
    return out


def blur_yuv420sp(y, uv, regions, grid, colour=None, filled=(), v_first=False):
    """`blur_u8` for an NV12 / NV21 surface (y uint8 [H, W], uv uint8 [H / 2, W]) -> (y, uv) blurred copies.  The Y plane is a one-channel
    picture over the region; the chroma plane a two-channel picture of pairs over the chroma region cx in [x0 >> 1, (x0 + width - 1) >>
    1], cy likewise, with a grid of its own whose cells are at least 2 pairs wide; a pair in several chroma regions gets the value of the
    first.  First bytes are averaged together and second bytes together (v_first matters to the fill only).  `colour` = (Y, U, V)."""
    grid = _blur_grid(grid)
    y_src, uv_src = np.asarray(y, np.uint8), np.asarray(uv, np.uint8)
    y_out, uv_out = y_src.copy(), uv_src.copy()
    h2, w = uv_src.shape
    pairs_src, pairs_out = uv_src.reshape(h2, w // 2, 2), uv_out.reshape(h2, w // 2, 2)
    regions, filled = list(regions), set(filled)
    chroma = [None if r is None else (r[0] >> 1, r[1] >> 1, ((r[0] + r[2] - 1) >> 1) - (r[0] >> 1) + 1, ((r[1] + r[3] - 1) >> 1) - (r[1] >> 1) + 1)
              for r in regions]
    if filled:
        yy, u, v = (int(c) for c in colour)
    luma = [np.uint8(yy) if k in filled else None for k in range(len(regions))]
    pair = [np.array((v, u) if v_first else (u, v), np.uint8) if k in filled else None for k in range(len(regions))]
    _blur_plane(y_src[..., None], y_out[..., None], regions, grid, BLUR_MIN_CELL, luma)
    _blur_plane(pairs_src, pairs_out, chroma, grid, 2, pair)
    return y_out, uv_out


# ---- the drawing (csrc/yf_images_draw.h), in plain numpy ----
def outline_mask(box, half, width, height):
    """the drawn set of one record in a picture of height x width, bool [height, width]"""
    x1, y1, x2, y2 = (int(v) for v in box)
    xa, xb, ya, yb = min(x1, x2), max(x1, x2), min(y1, y2), max(y1, y2)
    h = int(half)
    xs, ys = np.arange(width, dtype=np.int64)[None, :], np.arange(height, dtype=np.int64)[:, None]
    # the distances outside the box, cut at h + 1 (more than h is all the rule asks), and inside it
    ex = np.minimum(np.maximum(np.maximum(xa - xs, xs - xb), 0), h + 1)
    ey = np.minimum(np.maximum(np.maximum(ya - ys, ys - yb), 0), h + 1)
    ix, iy = np.minimum(xs - xa, xb - xs), np.minimum(ys - ya, yb - ys)
    near = (ex <= h) & (ey <= h)
    round_corner = (ex == 0) | (ey == 0) | (ex * ex + ey * ey <= h * h)
    not_interior = (ex > 0) | (ey > 0) | (np.minimum(ix, iy) <= h)
    return near & round_corner & not_interior


def _draw_colours(colours, count):
    c = np.asarray(colours, np.int64)
    if c.ndim == 1:
        c = np.broadcast_to(c, (count, 3))
    if c.shape != (count, 3) or c.min(initial=0) < 0 or c.max(initial=0) > 255:
        raise ValueError(f"colours: three bytes, or three bytes per box ({count} boxes)")
    return c.astype(np.uint8)


def _draw_half(half):
    if isinstance(half, bool) or half not in (0, 1, 2, 3):
        raise ValueError(f"half {half!r}: 0, 1, 2 or 3")
    return int(half)


def draw_rectangles_u8(picture_hwc, boxes, half, colours):
    """The copy of a packed picture (uint8 [H, W, 3 or 4]) with the outline of every box (x1, y1, x2, y2) drawn, as
    csrc/yf_images_draw.h states it, box after box in the order given -- a pixel that several boxes draw ends with the colour of the last,
    which is the overlap rule.  The edges are used as they are (no clamp; x1 > x2 is the same box as x2 > x1).  `half` = h in 0..3: a
    pixel at distances (ex, ey) outside the box and (ix, iy) inside it is drawn iff ex <= h and ey <= h, and ex == 0 or ey == 0 or
    ex * ex + ey * ey <= h * h, and ex > 0 or ey > 0 or min(ix, iy) <= h.  h = 0 is cv2.rectangle(..., 1); h = 1 is what OpenCV's
    drawing.cpp is read to draw for thickness 2 (three pixels per edge, a disc of radius 1 at each corner) -- read from memory of the
    source and, like `resize_linear_u8`, not pinned against a real cv2.  `colours`: three bytes for the picture's channels 0, 1, 2 in the
    picture's own order, or one such triple per box.  A fourth channel is never touched."""
    out = np.asarray(picture_hwc, np.uint8).copy()
    h = _draw_half(half)
    cols = _draw_colours(colours, len(boxes))
    for box, colour in zip(boxes, cols):
        out[..., :3][outline_mask(box, h, out.shape[1], out.shape[0])] = colour
    return out


def draw_rectangles_yuv420sp(y, uv, boxes, half, colours, v_first=False):
    """`draw_rectangles_u8` for an NV12 / NV21 surface (y uint8 [H, W], uv uint8 [H / 2, W]) -> (y, uv) copies.  `colours`: (Y, U, V), or
    one triple per box.  Box after box: the Y byte of every drawn pixel, and every chroma pair of which at least one of the four luma
    pixels is drawn gets (U, V), or (V, U) with v_first."""
    y_out, uv_out = np.asarray(y, np.uint8).copy(), np.asarray(uv, np.uint8).copy()
    hh, w = y_out.shape
    pairs = uv_out.reshape(hh // 2, w // 2, 2)
    h = _draw_half(half)
    cols = _draw_colours(colours, len(boxes))
    for box, (yy, u, v) in zip(boxes, cols):
        mask = outline_mask(box, h, w, hh)
        y_out[mask] = yy
        pairs[mask.reshape(hh // 2, 2, w // 2, 2).any(axis=(1, 3))] = (v, u) if v_first else (u, v)
    return y_out, uv_out


# ---- the tracker (csrc/yf_images_track.h), in plain Python ----
TRACK_SLOTS, TRACK_MAX_DETS = 64, 64
TRACK_CLIPPED, TRACK_DROPPED = 1, 2
_INT32_MAX = 2 ** 31 - 1
_ZERO_DET = (0, 0, 0, 0, 0, 0.0, 0, 0, 0, 0)


def track_empty_state():
    """The empty state of one stream: what 2824 zero bytes are.  {"issued", "reserved", "slots": 64 x [id, hits, misses, age, det]}, det a
    record as below."""
    return {"issued": 0, "reserved": 0, "slots": [[0, 0, 0, 0, _ZERO_DET] for _ in range(TRACK_SLOTS)]}


def _track_inc(v):
    return v if v == _INT32_MAX else v + 1


def _track_area(d):
    return (float(d[8]) - float(d[6]) + 1.0) * (float(d[9]) - float(d[7]) + 1.0)


def track_iou(a, b):
    """(inter, iou) of two records' boxes: the suppression's arithmetic (csrc/yf_images_nms.h, the + 1 pixel convention of
    yoloface_test.py:165-190), one float64 operation per step; iou is None when inter is not above 0"""
    xx1, yy1 = float(max(a[6], b[6])), float(max(a[7], b[7]))
    xx2, yy2 = float(min(a[8], b[8])), float(min(a[9], b[9]))
    wv, hv = xx2 - xx1 + 1.0, yy2 - yy1 + 1.0
    w, h = wv if wv > 0.0 else 0.0, hv if hv > 0.0 else 0.0
    inter = w * h
    if not inter > 0.0:
        return inter, None
    uni = (_track_area(a) + _track_area(b)) - inter
    return inter, inter / uni


def _track_match(boxes, dets, match_iou):
    """the global greedy match of one step: `boxes` {slot: record} of the occupied slots (only the four edges are read), `dets` the
    detections that count -> (slot_det, det_slot, ties).  The eligible pairs taken once in sorted order (-iou, detection, slot), those
    with a matched member skipped: the same pairs as round after round of the largest IoU left."""
    pairs = []
    for k, box in sorted(boxes.items()):
        for j, d in enumerate(dets):
            iou = track_iou(box, d)[1]
            if iou is not None and iou >= match_iou:
                pairs.append((-iou, j, k))
    pairs.sort()
    slot_det, det_slot = {}, {}
    ties = 0
    for at, (neg, j, k) in enumerate(pairs):
        if j in det_slot or k in slot_det:
            continue
        # a tie: another pair of the same IoU was still to be had when this one was taken, and shares a member with it
        nxt = at + 1
        while nxt < len(pairs) and pairs[nxt][0] == neg:
            j2, k2 = pairs[nxt][1:]
            if j2 not in det_slot and k2 not in slot_det and (j2 == j or k2 == k):
                ties += 1
                break
            nxt += 1
        det_slot[j], slot_det[k] = k, j
    return slot_det, det_slot, ties


def track_step(state, dets, params, count=None, cap=None, frame=0, stats=None):
    """One step of the tracker -- one stream, one frame -- as csrc/yf_images_track.h states it, in Python integers and floats (float64).
    `state`: as `track_empty_state` gives it (not changed; the new state is returned).  `dets`: the frame's records, tuples (frame, anchor,
    row, col, q_conf, conf, x1, y1, x2, y2) -- only the four edges are read, a record travels as it is.  `params`: (match_iou, min_hits,
    max_misses).  `count`, `cap`: the frame's count and the capacity of its row (default: len(dets) both); the first
    m = min(max(count, 0), cap, 64) records count.  `stats`: a dict whose counters "matches", "births", "removals", "held", "ties",
    "dropped" are added to.
    -> (state, emitted, status): emitted = [(record with its frame field set to `frame`, (id, hits, misses, age)), ...] in ascending id,
    all of them (the device writes the first out_cap); status bit 0: count above min(cap, 64), bit 1: a detection found no free slot.

    The match is the global greedy one: repeatedly the eligible pair (inter > 0.0 and iou >= match_iou) of the largest IoU among the slots
    and detections still unmatched, ties to the lower detection, then the lower slot.  Taking the pairs in that order once, sorted, and
    skipping those with a matched member picks the same pairs: the order of two pairs does not depend on which others are left."""
    match_iou, min_hits, max_misses = float(params[0]), int(params[1]), int(params[2])
    count = len(dets) if count is None else int(count)
    cap = len(dets) if cap is None else int(cap)
    lim = min(cap, TRACK_MAX_DETS)
    m = min(max(count, 0), lim)
    status = TRACK_CLIPPED if count > lim else 0
    dets = [tuple(d) for d in dets[:m]]
    slots = [list(s) for s in state["slots"]]
    issued = int(state["issued"])
    occupied = [s[0] != 0 for s in slots]
    slot_det, det_slot, ties = _track_match({k: s[4] for k, s in enumerate(slots) if occupied[k]}, dets, match_iou)
    removals = held = 0
    for k, s in enumerate(slots):
        if not occupied[k]:
            continue
        s[3] = _track_inc(s[3])
        if k in slot_det:
            s[4], s[1], s[2] = dets[slot_det[k]], _track_inc(s[1]), 0
        else:
            s[2] = _track_inc(s[2])
            if s[2] > max_misses:
                slots[k] = [0, 0, 0, 0, _ZERO_DET]
                removals += 1
    births = dropped = 0
    for j, d in enumerate(dets):
        if j in det_slot:
            continue
        free = [k for k, s in enumerate(slots) if s[0] == 0]
        if not free:
            status |= TRACK_DROPPED
            dropped += 1
            continue
        issued = (issued + 1) & 0xFFFFFFFF
        if issued == 0:
            issued = 1
        slots[free[0]] = [issued, 1, 0, 1, d]
        births += 1
    emitted = []
    for k in sorted((k for k, s in enumerate(slots) if s[0] != 0 and s[1] >= min_hits), key=lambda k: (slots[k][0], k)):
        i, hits, misses, age, d = slots[k]
        emitted.append(((int(frame),) + tuple(d[1:]), (i, hits, misses, age)))
        held += misses > 0
    if stats is not None:
        for name, v in (("matches", len(slot_det)), ("births", births), ("removals", removals), ("held", held), ("ties", ties),
                        ("dropped", dropped)):
            stats[name] = stats.get(name, 0) + v
    return {"issued": issued, "reserved": state["reserved"], "slots": slots}, emitted, status


# ---- the tracker with a motion model (csrc/yf_images_motion.h), in plain Python integers ----
MOTION_ONE, MOTION_LIMIT = 256, 2 ** 40
MOTION_DEFAULT = (192, 128, 256, 0)          # (alpha, beta, damp, smooth): the library's suggestion -- a choice, not a measurement
_INT32_MIN = -2 ** 31


def track_motion_empty_state():
    """The empty state of one stream: what 7176 zero bytes are.  {"issued", "reserved", "slots": 64 x [id, hits, misses, age, det, pad,
    pos, vel]}, det a record as in `track_step`, pos and vel lists of four integers (x1, y1, x2, y2; 1/256 pixel, 1/256 pixel per step)."""
    return {"issued": 0, "reserved": 0, "slots": [[0, 0, 0, 0, _ZERO_DET, 0, [0] * 4, [0] * 4] for _ in range(TRACK_SLOTS)]}


def motion_sat(v):
    """yfi_motion_sat: the clamp of a position or velocity to [-2^40, 2^40]"""
    return max(-MOTION_LIMIT, min(MOTION_LIMIT, int(v)))


def motion_mul(g, v):
    """yfi_motion_mul: the gain g (1/256) applied to v, toward zero"""
    return (g * v) >> 8 if v >= 0 else -((g * -v) >> 8)


def motion_box(p):
    """yfi_motion_box: the pixel of a position, floor((p + 128) / 256) clamped to int32"""
    return max(_INT32_MIN, min(_INT32_MAX, (int(p) + 128) // 256))


# ---- the optimal assignment (csrc/yf_images_assign.h), in plain Python integers ----
ASSIGN_TOP = 2 ** 30 + 1                     # the largest weight; cost = ASSIGN_TOP - weight
ASSIGNS = ("greedy", "optimal")


def track_assign_weights(boxes, dets, match_iou):
    """the table of weights of one step: w[i][j] of detection i and slot j < 64 -- 1 + int(iou * 2^30) (the product exact, the conversion
    truncating) for an eligible pair (inter > 0.0 and iou >= match_iou), 0 otherwise and for every slot not in `boxes`"""
    w = [[0] * TRACK_SLOTS for _ in dets]
    for k, box in boxes.items():
        for i, d in enumerate(dets):
            iou = track_iou(box, d)[1]
            if iou is not None and iou >= match_iou:
                w[i][k] = 1 + int(iou * 1073741824.0)
    return w


def track_assign_solve(w, stats=None):
    """yfi_assign_solve: the maximum-weight assignment of the rows of w (detections, at most 64) to its 64 columns (slots) by the
    shortest-augmenting-path procedure csrc/yf_images_assign.h prescribes -- rows in ascending order, cost ASSIGN_TOP - w, potentials
    from 0, a strict comparison in the relaxation, the LOWEST column attaining the minimum -- -> (slot_det, det_slot, total_weight); a
    row assigned to a column of weight 0 is unmatched.  The procedure is the definition: it settles which of several optima is taken.
    `stats`: a dict whose counter "rounds" (the repetitions of the search, at most m (m + 1) / 2) is added to and whose "potential" is
    raised to the largest |u|, |v| met, "path" to the columns of the longest augmenting path."""
    m, inf = len(w), 1 << 62
    rounds = bound = longest = 0
    u, v, p = [0] * m, [0] * TRACK_SLOTS, [-1] * TRACK_SLOTS
    for i in range(m):
        minv, used, way = [inf] * TRACK_SLOTS, [False] * TRACK_SLOTS, [-1] * TRACK_SLOTS
        visited = [r == i for r in range(m)]
        i0, j0 = i, -1
        while True:
            for j in range(TRACK_SLOTS):
                if not used[j]:
                    cur = (ASSIGN_TOP - w[i0][j]) - u[i0] - v[j]
                    if cur < minv[j]:
                        minv[j], way[j] = cur, j0
            delta, j1 = inf, -1
            for j in range(TRACK_SLOTS):
                if not used[j] and minv[j] < delta:
                    delta, j1 = minv[j], j
            for r in range(m):
                if visited[r]:
                    u[r] += delta
            for j in range(TRACK_SLOTS):
                if used[j]:
                    v[j] -= delta
                else:
                    minv[j] -= delta
            rounds += 1
            bound = max(bound, max(u, default=0), -min(v))
            j0 = j1
            if p[j0] < 0:
                break
            used[j0], i0 = True, p[j0]
            visited[i0] = True
        length = 0
        while j0 >= 0:
            j1 = way[j0]
            p[j0] = p[j1] if j1 >= 0 else i
            j0 = j1
            length += 1
        longest = max(longest, length)
    if stats is not None:
        stats["rounds"] = stats.get("rounds", 0) + rounds
        stats["potential"] = max(stats.get("potential", 0), bound)
        stats["path"] = max(stats.get("path", 0), longest)
    slot_det = {j: p[j] for j in range(TRACK_SLOTS) if p[j] >= 0 and w[p[j]][j] > 0}
    det_slot = {i: j for j, i in slot_det.items()}
    return slot_det, det_slot, sum(w[i][j] for j, i in slot_det.items())


def track_assign_match(boxes, dets, match_iou):
    """the optimal match of one step, with `_track_match`'s arguments: the maximum total weight over the eligible pairs -- maximum total
    IoU at 2^-30 resolution, not cardinality first -- -> (slot_det, det_slot, total_weight) in plain Python integers"""
    return track_assign_solve(track_assign_weights(boxes, dets, match_iou))


def track_motion_step(state, dets, params, count=None, cap=None, frame=0, stats=None, assign="greedy"):
    """One step of the tracker with a motion model -- one stream, one frame -- as csrc/yf_images_motion.h states it: `track_step` with a
    constant-velocity g-h filter on every edge, in Python integers (the IoU of the match stays float64).  `state`: as
    `track_motion_empty_state` gives it (not changed; the new state is returned).  `dets`, `count`, `cap`, `frame`, `stats`: as in
    `track_step`.  `params`: (match_iou, min_hits, max_misses, alpha, beta, damp, smooth), the gains in [0, 256] (1/256), smooth 0 or 1;
    `MOTION_DEFAULT` holds the library's suggestion for the last four, a choice and not a measurement.
    -> (state, emitted, status) as `track_step` gives them: a held-over track (misses > 0), and with smooth every track, is emitted with
    its edges replaced by the filter's position in pixels.
    `assign`: "greedy", the match of `track_step`; "optimal", `track_assign_match` in its place (csrc/yf_images_assign.h; the counter
    "ties" is then not added to)."""
    if assign not in ASSIGNS:
        raise ValueError(f"assign {assign!r}: 'greedy' or 'optimal'")
    match_iou, min_hits, max_misses = float(params[0]), int(params[1]), int(params[2])
    alpha, beta, damp, smooth = (int(v) for v in params[3:7])
    count = len(dets) if count is None else int(count)
    cap = len(dets) if cap is None else int(cap)
    lim = min(cap, TRACK_MAX_DETS)
    m = min(max(count, 0), lim)
    status = TRACK_CLIPPED if count > lim else 0
    dets = [tuple(d) for d in dets[:m]]
    slots = [[s[0], s[1], s[2], s[3], s[4], s[5], list(s[6]), list(s[7])] for s in state["slots"]]
    issued = int(state["issued"])
    occupied = [s[0] != 0 for s in slots]
    # predict: P' = pos + vel, both through the clamp first; the box of the match is P' in pixels
    pred = {k: [motion_sat(p) + motion_sat(v) for p, v in zip(s[6], s[7])] for k, s in enumerate(slots) if occupied[k]}
    boxes = {k: (0,) * 6 + tuple(motion_box(p) for p in pp) for k, pp in pred.items()}
    if assign == "optimal":
        slot_det, det_slot, ties = track_assign_match(boxes, dets, match_iou)[:2] + (0,)
    else:
        slot_det, det_slot, ties = _track_match(boxes, dets, match_iou)
    removals = held = 0
    for k, s in enumerate(slots):
        if not occupied[k]:
            continue
        s[3] = _track_inc(s[3])
        vel = [motion_sat(v) for v in s[7]]
        if k in slot_det:
            d = dets[slot_det[k]]
            s[4], s[1], s[2] = d, _track_inc(s[1]), 0
            res = [256 * int(z) - pp for z, pp in zip(d[6:10], pred[k])]
            s[6] = [motion_sat(pp + motion_mul(alpha, r)) for pp, r in zip(pred[k], res)]
            s[7] = [motion_sat(v + motion_mul(beta, r)) for v, r in zip(vel, res)]
        else:
            s[2] = _track_inc(s[2])
            if s[2] > max_misses:
                slots[k] = [0, 0, 0, 0, _ZERO_DET, 0, [0] * 4, [0] * 4]
                removals += 1
            else:
                s[6] = [motion_sat(pp) for pp in pred[k]]
                s[7] = [motion_mul(damp, v) for v in vel]
    births = dropped = 0
    for j, d in enumerate(dets):
        if j in det_slot:
            continue
        free = [k for k, s in enumerate(slots) if s[0] == 0]
        if not free:
            status |= TRACK_DROPPED
            dropped += 1
            continue
        issued = (issued + 1) & 0xFFFFFFFF
        if issued == 0:
            issued = 1
        slots[free[0]] = [issued, 1, 0, 1, d, 0, [256 * int(z) for z in d[6:10]], [0] * 4]
        births += 1
    emitted = []
    for k in sorted((k for k, s in enumerate(slots) if s[0] != 0 and s[1] >= min_hits), key=lambda k: (slots[k][0], k)):
        i, hits, misses, age, d, _, pos, _ = slots[k]
        edges = tuple(motion_box(p) for p in pos) if misses > 0 or smooth else tuple(d[6:10])
        emitted.append(((int(frame),) + tuple(d[1:6]) + edges, (i, hits, misses, age)))
        held += misses > 0
    if stats is not None:
        for name, v in (("matches", len(slot_det)), ("births", births), ("removals", removals), ("held", held), ("ties", ties),
                        ("dropped", dropped)):
            stats[name] = stats.get(name, 0) + v
    return {"issued": issued, "reserved": state["reserved"], "slots": slots}, emitted, status


# ---- the score of tracks against labelled identities (csrc/yf_images_score.h), in plain Python integers ----
SCORE_MAX_IDS, SCORE_MAX_ROWS = 256, 64
SCORE_GT_CLIPPED, SCORE_HYP_CLIPPED, SCORE_GT_VOID, SCORE_HYP_VOID = 1, 2, 4, 8
SCORE_COUNTERS = ("frames", "gt", "hyp", "matches", "misses", "false_positives", "switches", "overlap")
_U64 = 2 ** 64 - 1


def track_score_empty_state():
    """The empty state of one stream: what 3136 zero bytes are.  {"counters": the eight of SCORE_COUNTERS, "last": 256 hypothesis ids,
    "present": 256, "tracked": 256}, the three tables indexed by a ground-truth id - 1."""
    return {"counters": [0] * 8, "last": [0] * SCORE_MAX_IDS, "present": [0] * SCORE_MAX_IDS, "tracked": [0] * SCORE_MAX_IDS}


def track_score_step(state, truths, hyps, score_iou, gt_count=None, gt_cap=None, out_count=None, out_cap=None, stats=None):
    """One step of the CLEAR-MOT score -- one stream, one frame -- as csrc/yf_images_score.h states it, in Python integers (the IoU stays
    float64).  `state`: as `track_score_empty_state` gives it (not changed; the new state is returned).  `truths`: the frame's labelled
    objects (id, x1, y1, x2, y2), valid ids 1 .. 256.  `hyps`: the tracks a tracker reported for the frame, (id, x1, y1, x2, y2) -- of
    `track_step`'s emitted pairs (record, info): (info[0], *record[6:10]).  `gt_count`, `gt_cap`, `out_count`, `out_cap`: the counts and
    the capacities of the two rows (default: the lengths); the first min(max(count, 0), cap, 64) of each count.  `stats`: a dict whose
    counters "kept", "new", "switches", "void_rows", "void_columns" are added to.
    -> (state, match, status): match[i] for every row that counts, the column of its hypothesis or -1; status bit 0 / 1: a count above
    min(cap, 64) of the truth / the hypotheses, bit 2: a void row (id 0, above 256, or an earlier row's), bit 3: a record of id 0.

    An object keeps the hypothesis id it was last matched to while that pair stays eligible (inter > 0.0 and iou >= score_iou); the
    other rows and columns go to `track_assign_solve`; a new match to another id than the last one is one switch."""
    score_iou = float(score_iou)
    gt_count = len(truths) if gt_count is None else int(gt_count)
    gt_cap = len(truths) if gt_cap is None else int(gt_cap)
    out_count = len(hyps) if out_count is None else int(out_count)
    out_cap = len(hyps) if out_cap is None else int(out_cap)
    glim, hlim = min(gt_cap, SCORE_MAX_ROWS), min(out_cap, TRACK_SLOTS)
    g, h = min(max(gt_count, 0), glim), min(max(out_count, 0), hlim)
    status = (SCORE_GT_CLIPPED if gt_count > glim else 0) | (SCORE_HYP_CLIPPED if out_count > hlim else 0)
    truths = [tuple(int(v) for v in t) for t in truths[:g]]
    hyps = [tuple(int(v) for v in t) for t in hyps[:h]]
    row_ok = [1 <= t[0] <= SCORE_MAX_IDS and all(e[0] != t[0] for e in truths[:i]) for i, t in enumerate(truths)]
    col_ok = [t[0] != 0 for t in hyps]
    if not all(row_ok):
        status |= SCORE_GT_VOID
    if not all(col_ok):
        status |= SCORE_HYP_VOID
    as_record = lambda t: (0,) * 6 + tuple(t[1:5])
    w = track_assign_weights({j: as_record(t) for j, t in enumerate(hyps) if col_ok[j]}, [as_record(t) for t in truths], score_iou)
    for i in range(g):
        if not row_ok[i]:
            w[i] = [0] * TRACK_SLOTS
    last, present, tracked = list(state["last"]), list(state["present"]), list(state["tracked"])
    # continuity: a valid correspondence is kept
    row_col, row_w, kept_cols = [-1] * g, [0] * g, set()
    for i in range(g):
        if not row_ok[i]:
            continue
        k = last[truths[i][0] - 1]
        if k == 0:
            continue
        j = next((j for j, t in enumerate(hyps) if t[0] == k), None)
        if j is None or j in kept_cols or w[i][j] <= 0:
            continue
        kept_cols.add(j)
        row_col[i], row_w[i] = j, w[i][j]
    kept = len(kept_cols)
    # the rest: the kept rows and columns leave the table, the procedure of csrc/yf_images_assign.h takes all g rows
    for i in range(g):
        for j in range(TRACK_SLOTS):
            if row_col[i] >= 0 or j in kept_cols:
                w[i][j] = 0
    switches = new = 0
    det_slot = track_assign_solve(w)[1] if any(v > 0 for row in w for v in row) else {}
    for i, j in sorted(det_slot.items()):
        k = last[truths[i][0] - 1]
        switches += k != 0 and k != hyps[j][0]
        row_col[i], row_w[i] = j, w[i][j]
        new += 1
    rows, cols, matches = sum(row_ok), sum(col_ok), kept + new
    for i in range(g):
        if not row_ok[i]:
            continue
        o = truths[i][0] - 1
        present[o] = _track_inc(present[o])
        if row_col[i] >= 0:
            tracked[o] = _track_inc(tracked[o])
            last[o] = hyps[row_col[i]][0]
    adds = (1, rows, cols, matches, rows - matches, cols - matches, switches, sum(row_w))
    counters = [(c + a) & _U64 for c, a in zip(state["counters"], adds)]
    if stats is not None:
        for name, v in (("kept", kept), ("new", new), ("switches", switches), ("void_rows", g - rows), ("void_columns", h - cols)):
            stats[name] = stats.get(name, 0) + v
    return {"counters": counters, "last": last, "present": present, "tracked": tracked}, row_col, status


def track_score_summary(states):
    """yf_images_score_summary over the states of the streams: the sums of the eight counters (modulo 2^64), "objects" (entries with
    present > 0, counted per stream), "mostly_tracked" (5 tracked >= 4 present), "mostly_lost" (5 tracked <= present), and
    mota = 1.0 - float(misses + false_positives + switches) / float(gt) (0.0 without ground truth), motp = (float(overlap) /
    float(matches)) / 2^30 (0.0 without a match), each a chain of single float64 operations: the mean IoU of the matched pairs at 2^-30
    resolution, every weight with the + 1 of the assignment's weights."""
    out = {name: 0 for name in SCORE_COUNTERS}
    out.update(objects=0, mostly_tracked=0, mostly_lost=0)
    for st in states:
        for name, c in zip(SCORE_COUNTERS, st["counters"]):
            out[name] = (out[name] + c) & _U64
        for p, t in zip(st["present"], st["tracked"]):
            if p > 0:
                out["objects"] += 1
                out["mostly_tracked"] += 5 * t >= 4 * p
                out["mostly_lost"] += 5 * t <= p
    errors = (out["misses"] + out["false_positives"] + out["switches"]) & _U64
    out["mota"] = 1.0 - float(errors) / float(out["gt"]) if out["gt"] else 0.0
    out["motp"] = (float(out["overlap"]) / float(out["matches"])) / 1073741824.0 if out["matches"] else 0.0
    return out


# ---- appearance descriptors and re-identification (csrc/yf_images_describe.h, csrc/yf_images_reid.h), in plain Python integers ----
DESC_GRID, DESC_BYTES = 8, 64
REID_ENTRIES = 64
REID_CLIPPED, REID_VOID = 1, 2
REID_KNOWN, REID_REIDENTIFIED, REID_BORN = 1, 2, 3
_LUMA = {"bgr": (29, 150, 77), "bgra": (29, 150, 77), "rgb": (77, 150, 29), "rgba": (77, 150, 29)}


def _describe_cells(region, cell_value):
    """the 64 bytes of a region (x0, y0, width, height), or None for none or one narrower or lower than 8: cell c of a side holds
    [c * side // 8, (c + 1) * side // 8); cell_value(x range, y range, cnt) is the cell's byte"""
    if region is None or region[2] < DESC_GRID or region[3] < DESC_GRID:
        return None
    x0, y0, w, h = region
    out = []
    for cy in range(DESC_GRID):
        ya, yb = cy * h // DESC_GRID, (cy + 1) * h // DESC_GRID
        for cx in range(DESC_GRID):
            xa, xb = cx * w // DESC_GRID, (cx + 1) * w // DESC_GRID
            out.append(cell_value(range(x0 + xa, x0 + xb), range(y0 + ya, y0 + yb), (xb - xa) * (yb - ya)))
    return out


def describe_u8(picture_hwc, box, fmt, margin_permille=0, square=False):
    """The appearance descriptor of `box` = (x1, y1, x2, y2) in a packed picture (uint8 [H, W, 3 or 4], fmt "bgr", "rgb", "bgra" or
    "rgba"), as csrc/yf_images_describe.h states it: the 64 bytes v[cy * 8 + cx], or None for an invalid descriptor (no region, or a
    region narrower or lower than 8 pixels).  The region is `crop_region`'s, cut into 8 x 8 cells; a cell's byte is its mean luma,
    (S + 128 cnt) // (256 cnt) with S the sum over its pixels of 77 R + 150 G + 29 B; a fourth channel is never read.  A tiny template,
    not a learned embedding."""
    wts = _LUMA[fmt.lower()]
    img = [[tuple(int(c) for c in px[:3]) for px in row] for row in np.asarray(picture_hwc, np.uint8).tolist()]
    region = crop_region(box, len(img[0]), len(img), margin_permille, square)

    def luma(xs, ys, cnt):
        s = sum(wts[0] * img[y][x][0] + wts[1] * img[y][x][1] + wts[2] * img[y][x][2] for y in ys for x in xs)
        return (s + 128 * cnt) // (256 * cnt)
    return _describe_cells(region, luma)


def describe_yuv420sp(y, box, margin_permille=0, square=False):
    """`describe_u8` for an NV12 / NV21 surface: only the Y plane (uint8 [H, W]) is read; a cell's byte is (sum of Y + cnt // 2) //
    cnt."""
    plane = np.asarray(y, np.uint8).tolist()
    region = crop_region(box, len(plane[0]), len(plane), margin_permille, square)
    return _describe_cells(region, lambda xs, ys, cnt: (sum(plane[yy][x] for yy in ys for x in xs) + cnt // 2) // cnt)


def reid_distance(a, b):
    """The distance of two descriptors of 64 bytes: sum_i |(64 a_i - A) - (64 b_i - B)| with A, B the byte sums -- the mean-removed sum
    of absolute differences, at most 64 * 64 * 255."""
    a, b = [int(v) for v in a], [int(v) for v in b]
    assert len(a) == DESC_BYTES and len(b) == DESC_BYTES
    sa, sb = sum(a), sum(b)
    return sum(abs((64 * x - sa) - (64 * y - sb)) for x, y in zip(a, b))


def reid_empty_state():
    """The empty state of one stream: what 5128 zero bytes are.  {"clock", "reserved", "entries": 64 of {"id", "alias", "seen", "flags",
    "v": 64 bytes}}."""
    return {"clock": 0, "reserved": 0, "entries": [{"id": 0, "alias": 0, "seen": 0, "flags": 0, "v": [0] * DESC_BYTES} for _ in range(REID_ENTRIES)]}


def _reid_meet(entry, new, blend):
    if entry["flags"] & 1:
        entry["v"] = [(o * (256 - blend) + n * blend + 128) >> 8 for o, n in zip(entry["v"], new)]
    else:
        entry["v"] = list(new)
        entry["flags"] |= 1


def reid_step(state, records, descs, params, count=None, out_cap=None):
    """One step of the re-identification -- one stream, one frame -- as csrc/yf_images_reid.h states it.  `state`: as `reid_empty_state`
    gives it (not changed; the new state is returned).  `records`: the tracker's info rows (id, hits, misses, age) of the frame in the
    order they lie.  `descs`: per record its 64 descriptor bytes, or None for an invalid one.  `params` = (max_distance, max_age, blend).
    `count`, `out_cap`: the frame's count and the rows' capacity (default: the length); the first m = min(max(count, 0), out_cap, 64)
    records count.
    -> (state, ids, what, status): per record that counts its new id and 0 void / 1 known / 2 re-identified / 3 born; status bit 0: a
    count above min(out_cap, 64), bit 1: a record of tracker id 0."""
    max_distance, max_age, blend = (int(v) for v in params)
    count = len(records) if count is None else int(count)
    out_cap = len(records) if out_cap is None else int(out_cap)
    lim = min(out_cap, REID_ENTRIES)
    m = min(max(count, 0), lim)
    status = REID_CLIPPED if count > lim else 0
    recs = [tuple(int(v) for v in r) for r in records[:m]]
    descs = [None if d is None else [int(v) for v in d] for d in descs[:m]]
    if any(r[0] == 0 for r in recs):
        status |= REID_VOID
    entries = [dict(e, v=list(e["v"])) for e in state["entries"]]
    now = (state["clock"] + 1) & 0xFFFFFFFF
    ids, what, bound = [0] * m, [0] * m, [False] * REID_ENTRIES
    # bind
    for r, (tid, _, misses, _) in enumerate(recs):
        if tid == 0:
            continue
        e = next((k for k, en in enumerate(entries) if en["id"] != 0 and en["alias"] == tid), None)
        if e is None:
            continue
        bound[e], what[r], ids[r] = True, REID_KNOWN, entries[e]["id"]
        entries[e]["seen"] = now
        if misses == 0 and descs[r] is not None:
            _reid_meet(entries[e], descs[r], blend)
    # expire
    for k, en in enumerate(entries):
        if en["id"] != 0 and not bound[k] and ((now - en["seen"]) & 0xFFFFFFFF) > max_age:
            entries[k] = {"id": 0, "alias": 0, "seen": 0, "flags": 0, "v": [0] * DESC_BYTES}
    # re-identify
    rcand = [r for r in range(m) if what[r] == 0 and recs[r][0] != 0 and recs[r][2] == 0 and descs[r] is not None]
    ecand = [k for k, en in enumerate(entries) if not bound[k] and en["id"] != 0 and en["flags"] & 1] if rcand else []
    pairs = sorted((reid_distance(descs[r], entries[k]["v"]), r, k) for r in rcand for k in ecand)
    for d, r, k in pairs:                                           # only a taken entry's descriptor changes: the distances hold
        if d > max_distance:
            break
        if what[r] != 0 or bound[k]:
            continue
        entries[k]["alias"], entries[k]["seen"] = recs[r][0], now
        _reid_meet(entries[k], descs[r], blend)
        bound[k], what[r], ids[r] = True, REID_REIDENTIFIED, entries[k]["id"]
    # births
    for r in range(m):
        if what[r] != 0 or recs[r][0] == 0:
            continue
        e = next((k for k, en in enumerate(entries) if en["id"] == 0), None)
        if e is None:
            ages = [((now - en["seen"]) & 0xFFFFFFFF, -k) for k, en in enumerate(entries) if not bound[k]]
            e = -max(ages)[1]
        entries[e] = {"id": recs[r][0], "alias": recs[r][0], "seen": now, "flags": 0 if descs[r] is None else 1,
                      "v": [0] * DESC_BYTES if descs[r] is None else list(descs[r])}
        bound[e], what[r], ids[r] = True, REID_BORN, recs[r][0]
    return {"clock": now, "reserved": state.get("reserved", 0), "entries": entries}, ids, what, status
