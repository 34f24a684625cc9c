"""What the simulation tests share (test_calib_sim_host.py, test_calib_sim_gpu.py): the numpy restatement of csrc/yf_calib_sim.h -- yfc_sim_q
and the head's record in the defined order (quant_support.restate_frame adapted to float inputs) --, the tables the tests enable, the frames,
and bit-wise comparisons.  Everything is computed once per process."""
import functools

import numpy as np

import calib_support as cs
import calib_hw_support as hw
import quant_support as qs
from calib_support import calib, model_file

LANES, GROUP = qs.LANES, qs.GROUP
WEIGHTS = "npz"                       # the float weights the shipped int8 model was quantised from
ALPHA = np.array([0x3DCCCCCD], "<u4").view("<f4")[0]


def sim_q(v, scale, zero_point):
    """yfc_sim_q in numpy, every line one float32 operation -> (float32 values on the grid, the number of values clipped)"""
    v, scale = np.asarray(v, np.float32), np.float32(scale)
    inv = np.float32(1.0 / np.float64(scale))
    lo, hi = np.float32(-128 - int(zero_point)), np.float32(127 - int(zero_point))
    with np.errstate(all="ignore"):
        t = v * inv
        r = np.rint(t)
        c = np.where(r < lo, lo, np.where(r > hi, hi, r)).astype(np.float32)
        out = c * scale
    assert t.dtype == r.dtype == out.dtype == np.float32
    return out, int(((r < lo) | (r > hi)).sum())


def restate_frame(y, x, clipped):
    """One frame's record: y simulated and x reference logits, float32 [E] -> (sum_err, sum_sq_err, sum_sq_ref, max_abs_err, saturated)"""
    y, x = np.asarray(y, np.float32).reshape(-1), np.asarray(x, np.float32).reshape(-1)
    e = y - x
    de, dx = e.astype(np.float64), x.astype(np.float64)
    terms = np.stack([de, de * de, dx * dx])
    lanes = np.zeros((3, LANES), np.float64)
    for k in range((e.size + LANES - 1) // LANES):                  # a lane adds its elements in ascending order
        seg = terms[:, k * LANES:(k + 1) * LANES]
        lanes[:, :seg.shape[1]] = lanes[:, :seg.shape[1]] + seg
    s = lanes.reshape(3, LANES // GROUP, GROUP)
    h = GROUP // 2
    while h:                                                        # s[l] = s[l] + s[l + h] for l < h
        s[:, :, :h] = s[:, :, :h] + s[:, :, h:2 * h]
        h //= 2
    total = s[:, 0, 0].copy()
    for g in range(1, LANES // GROUP):                              # the groups in order
        total = total + s[:, g, 0]
    a = np.abs(e)
    a = a[~np.isnan(a)]
    return total[0], total[1], total[2], np.float32(a.max() if a.size else 0.0), int(clipped)


def restate(ys, xs, clipped):
    """(records [n], totals [1]) as the library must give them for simulated ys and reference xs [n, ...] and the frames' clipped counts"""
    n = ys.shape[0]
    stats, totals = np.zeros(n, calib.FRAME_STATS), np.zeros(1, calib.TOTALS)
    for f in range(n):
        stats[f] = restate_frame(ys[f], xs[f], clipped[f])
    for k in ("sum_err", "sum_sq_err", "sum_sq_ref"):
        v = stats[0][k]
        for f in range(1, n):                                       # the frames in order
            v = v + stats[f][k]
        totals[0][k] = v
    totals[0]["max_abs_err"] = stats["max_abs_err"].max()
    totals[0]["saturated"] = stats["saturated"].astype(np.int64).sum()
    totals[0]["elements"] = ys[0].size * n
    return stats, totals


def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, got.dtype, want.shape, want.dtype)
    d = np.argwhere(cs.bits(got) != cs.bits(want))
    assert not d.shape[0], f"{what}: {d.shape[0]} values differ, first at {tuple(d[0])}: {got[tuple(d[0])]!r} vs {want[tuple(d[0])]!r}"


@functools.lru_cache(maxsize=None)
def ids():
    return calib.sim_tensors()


def entry_of(tensor):
    return ids().index(tensor)


def shipped_table(tensors=None):
    return calib.simulation_table(qs.shipped_yfm(), tensors)


def one_entry(tensor, scale, zero_point):
    t = calib.empty_table()
    t[entry_of(tensor)] = (np.float32(scale), int(zero_point))
    return t


@functools.lru_cache(maxsize=None)
def frames33():
    """the 27 calibration frames and 6 seeded random ones: int8 [33, 56, 56, 3]"""
    x = np.concatenate([cs.calib_frames(), np.random.default_rng(33).integers(-128, 128, (6, 56, 56, 3), dtype=np.int8)])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def float_logits(name, h, w, n):
    """the all-float logits of the host build (the reference of a simulation) on the calibration frames at 56x56, hw.frames elsewhere"""
    x = cs.calib_frames()[:n] if (h, w) == (56, 56) else hw.frames(h, w, n)
    lg, _ = calib.host_simulate(cs.yfw_bytes(name), x, calib.empty_table(), threads=16)
    lg.setflags(write=False)
    return lg


def host_all(y, x, table, general=False, threads=16):
    """(reference logits, simulated logits, totals, records) of the host build"""
    ref, _ = calib.host_simulate(y, x, calib.empty_table(), threads=threads, general=general)
    lg, totals, stats = calib.host_simulate(y, x, table, ref, threads=threads, general=general, want_stats=True)
    return ref, lg, totals, stats


def head_conv(x, yfw):
    """the network's last convolution (1x1, 32 -> 18) on x float32 [n, pixels * 32] as yf_calib_arith.h states it: acc = acc + x * w over ci
    ascending in float32, then + bias -> [n, pixels * 18]"""
    w, b, _ = model_file.read_yfw(yfw)[23]
    w = np.asarray(w, np.float32).reshape(18, 32)
    x = np.asarray(x, np.float32).reshape(x.shape[0], -1, 32)
    acc = np.zeros(x.shape[:2] + (18,), np.float32)
    for ci in range(32):
        acc = acc + x[:, :, ci, None] * w[None, None, :, ci]
    return (acc + np.asarray(b, np.float32)[None, None, :]).reshape(x.shape[0], -1)


def leaky(v):
    v = np.asarray(v, np.float32)
    return np.where(v >= 0, v, v * ALPHA).astype(np.float32)
