"""What the channel-sum tests share (test_calib_chan_host.py, test_calib_chan_gpu.py): a plain-Python restatement of the order csrc/yf_calib_chan.h
defines, written from the definition's text -- per frame and channel the pixels p = oy * ow + ox in chunks of 64 consecutive p; in a chunk
lane l holds float64(y) of pixel 64 * chunk + l, or +0.0 when there is no such pixel; s[l] = s[l] + s[l + h] for l < h, h = 32 .. 1; the
frame's value is chunk 0, then + chunk 1, ... ascending; over frames frame 0, then + frame 1, ... ascending --, the raw convolution outputs
of calib_packs.evaluate to feed it, the planted-bias packs, and bit-wise comparisons of doubles.  Everything is computed once per process."""
import functools

import numpy as np

import calib_packs as cp
import calib_support as cs
from calib_support import calib, model_file

CHUNK = 64


def chunk_values(lanes):
    """float64 [64, channels] -> [channels]: the halving"""
    s = np.array(lanes, np.float64)
    assert s.shape[0] == CHUNK
    h = CHUNK // 2
    while h:
        s[:h] = s[:h] + s[h:2 * h]
        h //= 2
    return s[0].copy()


def frame_values(raw):
    """one frame's raw output of one convolution, float32 [pixels, cout] in pixel order -> float64 [cout]"""
    raw = np.asarray(raw)
    assert raw.dtype == np.float32 and raw.ndim == 2
    pixels, total = raw.shape[0], None
    with np.errstate(all="ignore"):
        for at in range(0, pixels, CHUNK):
            lanes = np.zeros((CHUNK, raw.shape[1]), np.float64)
            seg = raw[at:at + CHUNK].astype(np.float64)
            lanes[:seg.shape[0]] = seg
            v = chunk_values(lanes)
            total = v if total is None else total + v
    return total


def restate(raws):
    """raws: per convolution in file order float32 [n, pixels, cout] -> (per-frame sums float64 [n, 544], totals float64 [544])"""
    n = raws[0].shape[0]
    rows = np.stack([np.concatenate([frame_values(r[f]) for r in raws]) for f in range(n)])
    total = rows[0].copy()
    with np.errstate(all="ignore"):
        for f in range(1, n):
            total = total + rows[f]
    assert rows.shape == (n, calib.CHANNELS)
    return rows, total


@functools.lru_cache(maxsize=None)
def conv_outputs():
    """the output tensor of each of the 24 convolutions, in file order"""
    g = model_file.load_graph()
    return tuple(g["ops"][d["op"]]["out"] for d in model_file.graph_convs(g))


@functools.lru_cache(maxsize=None)
def layout():
    """(first, cout) per convolution, from the graph alone"""
    cout = [d["cout"] for d in model_file.graph_convs()]
    return tuple(int(v) for v in np.concatenate([[0], np.cumsum(cout)[:-1]])), tuple(cout)


def raw_outputs(convs, frames, table=None):
    """float32 [n, pixels, cout] per convolution: the value each convolution's output holds BEFORE its own table entry quantises it, in
    calib_packs.evaluate's restatement of the (simulated) evaluation.  evaluate hands every enabled tensor to calib_packs.sim_q in the order
    it is produced; the values it is handed are recorded here and told apart by that order."""
    frames = np.asarray(frames, np.int8)
    n = frames.shape[0]
    if table is None or not (np.asarray(table)["scale"] != 0).any():
        tensors = cp.evaluate(convs, frames).tensors
        return [np.ascontiguousarray(tensors[t].reshape(n, -1, tensors[t].shape[3])) for t in conv_outputs()]
    O, g, entries = model_file.OPCODE, cp.graph(), cp.entry_tensors()
    kinds = [O[k] for k in ("CONV_2D", "DEPTHWISE_CONV_2D", "LEAKY_RELU", "MAX_POOL_2D", "ADD", "QUANTIZE")]
    order = [t for t in [g["input"]] + [o["out"] for o in g["ops"] if o["op"] in kinds] if t in entries and table[entries.index(t)]["scale"] != 0]
    assert all(t in order for t in conv_outputs()), "raw_outputs: every convolution's own entry must be enabled (or none at all)"
    seen, original = [], cp.sim_q

    def recording(v, scale, zero_point):
        seen.append(np.array(v, np.float32))
        return original(v, scale, zero_point)

    cp.sim_q = recording
    try:
        cp.evaluate(convs, frames, "defined", table)
    finally:
        cp.sim_q = original
    assert len(seen) == len(order), (len(seen), len(order))
    by_tensor = dict(zip(order, seen))
    return [np.ascontiguousarray(by_tensor[t].reshape(n, -1, by_tensor[t].shape[3])) for t in conv_outputs()]


def same_doubles(got, want, what):
    """bit for bit, except that a NaN equals any NaN (calib_packs.differing)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype == np.float64 and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    cp.assert_same_floats(got, want, what)


# ---------------------------------------------------------------------------------------------------------------- planted biases
PLANTED = (2, 7, 20)                      # one convolution in each phase: 28x28 (4 channels), 14x14 (36), 7x7 (40)


@functools.lru_cache(maxsize=None)
def planted(k):
    """(.yfw bytes, biases): the shipped weights with convolution k's weights all zero and seeded 24-bit biases of both signs -- its raw
    output is bias[co] at every pixel of any finite frame, so a frame's sum is pixels * bias and the total n * pixels * bias, exactly: every
    partial sum is an integer multiple of a 24-bit number, far inside a double's 53 bits"""
    rng = np.random.default_rng(500 + k)
    convs = cp._base()
    values = (rng.integers(1, 1 << 24, convs[k][1].shape).astype(np.float64) * 2.0 ** -20 * rng.choice([-1.0, 1.0], convs[k][1].shape)).astype(np.float32)
    assert (values.astype(np.float64) * 2.0 ** 20 == np.rint(values.astype(np.float64) * 2.0 ** 20)).all()
    cp._plant(convs, k, values)
    return model_file.write_yfw([(w, b, dw) for w, b, dw in convs]), values


def planted_want(k, n, pixels):
    """float64 [cout]: n * pixels * bias"""
    return float(n * pixels) * planted(k)[1].astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------- bias correction
def bias_bound(yfm_bytes, ranges):
    """float64 [544]: s_bias[c] + 2^-23 * max(|rmin|, |rmax|) of the convolution's output range.  The first term is two roundings to the bias
    grid (the corrected float bias to float32 and to the grid, at most half a step each way against what the measurement asked for, and the
    measurement itself was taken on the grid's previous value); the second the float32 rounding of acc + bias, 2^-24 relative per value, in the
    measured and in the corrected run."""
    m, out = model_file.load_yfm(yfm_bytes), []
    for d, t in zip(model_file.graph_convs(), conv_outputs()):
        s_bias = m["tensors"][m["ops"][d["op"]]["ins"][2]]["scale"].astype(np.float32).astype(np.float64)
        out.append(s_bias + 2.0 ** -23 * max(abs(ranges[t][0]), abs(ranges[t][1])))
    return np.concatenate(out)


def host_sums(threads=16):
    """the channel_sums= injection of calib.correct_biases on the host build"""
    return lambda yfw, frames, table: calib.host_channel_sums(yfw, frames, table, threads=threads)


def mean_gap(yfw_float, yfm_bytes, frames, sums):
    """|mean_sim - mean_float| per channel over frames: the model yfm_bytes on its dequantised weights (every convolution's numbers come from
    the model, so the weights dequantized_yfw starts from do not matter) under its full table, against the float weights"""
    from calib_support import ptq
    n, h, w = frames.shape[0], frames.shape[1], frames.shape[2]
    count = calib.channel_pixels(h, w) * float(n)
    mean_float = np.asarray(sums(yfw_float, frames, calib.empty_table())) / count
    mean_sim = np.asarray(sums(ptq.dequantized_yfw(yfw_float, yfm_bytes), frames, calib.simulation_table(yfm_bytes))) / count
    return np.abs(mean_sim - mean_float)
