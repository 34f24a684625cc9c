"""What the quantisation-error tests share (test_quant_compare_host.py, test_quant_compare_gpu.py): the entries of the shipped model over the
oracle's per-op dump, a numpy restatement of the arithmetic csrc/yf_calib_compare.h defines, and bit-wise comparison of records."""
import functools
import importlib

import numpy as np

import calib_support as cs
import model_variants as mv
from calib_support import calib

binding = importlib.import_module("stm32h7-yolo_amd.binding")
LANES, GROUP = 1024, 64
WEIGHTS = "npz"                       # the float weights the shipped int8 model was quantised from


@functools.lru_cache(maxsize=None)
def shipped_yfm():
    return open(cs.SHIPPED_YFM, "rb").read()


@functools.lru_cache(maxsize=None)
def dump_offset():
    """yf_network_dump_offset of libyf_network.so: host C, callable without a GPU"""
    return binding.load().yf_network_dump_offset


@functools.lru_cache(maxsize=None)
def tensors():
    """calib.report_tensors of the shipped model: the dumped tensors the float evaluation has, and the head"""
    return tuple(calib.report_tensors(dump_offset(), shipped_yfm()))


def elements():
    return [t["elements"] for t in tensors()]


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle.oracle import Oracle
    return Oracle()


def oracle_run(frames):
    """(heads int8 [n, 882], dump int8 [n, dump bytes]) of the oracle on the shipped model"""
    heads, dump = _oracle().run(np.ascontiguousarray(frames), dump=True, threads=16)
    return np.ascontiguousarray(heads.reshape(heads.shape[0], -1)), np.ascontiguousarray(dump)


@functools.lru_cache(maxsize=None)
def real_run():
    heads, dump = oracle_run(cs.calib_frames())
    heads.setflags(write=False)
    dump.setflags(write=False)
    return heads, dump


def oracle_q(heads, dump):
    """per tensor of tensors(): the int8 values [n, elements] (a contiguous copy) out of the oracle's heads and dump"""
    sizes, offs, _ = mv.dump_layout()
    out = []
    for t in tensors():
        assert sizes[t["op"]] == t["elements"]
        out.append(np.ascontiguousarray(heads if t["offset"] is None else dump[:, offs[t["op"]]:offs[t["op"]] + sizes[t["op"]]]))
    return out


def entries_over(qs, which=None, scale=None, zero_point=None):
    """Entries of tensors() (or of the indices `which`) over the arrays qs[i] ([n, >= elements] int8, rows contiguous)"""
    idx = range(len(tensors())) if which is None else which
    return [calib.Entry(tensors()[i]["tensor"], tensors()[i]["scale"] if scale is None else scale[k],
                        tensors()[i]["zero_point"] if zero_point is None else zero_point[k], qs[k], qs[k].strides[0]) for k, i in enumerate(idx)]


@functools.lru_cache(maxsize=None)
def real_host():
    """(records, totals, float32 tensors) of the host build, one thread, on the 27 calibration frames and the oracle's dump"""
    return calib.host_compare(cs.yfw_bytes(WEIGHTS), cs.calib_frames(), entries_over(oracle_q(*real_run())), threads=1, want_tensors=True,
                              elements=elements())


# ---- the arithmetic, restated ------------------------------------------------------------------------------------------------------
def restate_frame(q, x, scale, zero_point):
    """One frame of one entry: q int8 [E], x float32 [E] -> (sum_err, sum_sq_err, sum_sq_ref, max_abs_err, saturated)"""
    d = (q.astype(np.int32) - np.int32(zero_point)).astype(np.float32) * np.float32(scale)
    e = d - x.astype(np.float32)
    de, dx = e.astype(np.float64), x.astype(np.float64)
    terms = np.stack([de, de * de, dx * dx])
    lanes = np.zeros((3, LANES), np.float64)
    for k in range((q.size + LANES - 1) // LANES):                  # a lane adds its elements in ascending order
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
    return total[0], total[1], total[2], np.float32(a.max() if a.size else 0.0), int(((q == -128) | (q == 127)).sum())


def restate(qs, xs, scales, zero_points):
    """(records [n, count], totals [count]) as the library must give them for int8 qs[i] [n, E_i] and float32 xs[i] [n, E_i]"""
    n, count = qs[0].shape[0], len(qs)
    stats, totals = np.zeros((n, count), calib.FRAME_STATS), np.zeros(count, calib.TOTALS)
    for i in range(count):
        for f in range(n):
            stats[f, i] = restate_frame(qs[i][f, :xs[i].shape[1]], xs[i][f], scales[i], zero_points[i])
        for k in ("sum_err", "sum_sq_err", "sum_sq_ref"):
            v = stats[0, i][k]
            for f in range(1, n):                                   # the frames in order
                v = v + stats[f, i][k]
            totals[i][k] = v
        totals[i]["max_abs_err"] = stats[:, i]["max_abs_err"].max()
        totals[i]["saturated"] = stats[:, i]["saturated"].astype(np.int64).sum()
        totals[i]["elements"] = xs[i].shape[1] * n
    return stats, totals


def same_records(got, want, what):
    """bit-wise equality of two record arrays of one dtype, with the first difference named"""
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {got.shape} against {want.dtype} {want.shape}"
    a = np.ascontiguousarray(got).view(np.uint8).reshape(got.shape + (got.dtype.itemsize,))
    b = np.ascontiguousarray(want).view(np.uint8).reshape(want.shape + (want.dtype.itemsize,))
    bad = np.argwhere((a != b).any(axis=-1))
    assert not bad.shape[0], (f"{what}: {bad.shape[0]} of {got.size} records differ, first at {tuple(bad[0])} (entry last): "
                              f"{got[tuple(bad[0])]!r} against {want[tuple(bad[0])]!r}")


def printed_head_lsb():
    """the shipped pair's maximum head error in LSB as profiles/calib_accuracy.txt section 4 prints it: (value, half a unit of its last digit)"""
    import os
    import re
    from conftest import ROOT
    text = open(os.path.join(ROOT, "profiles", "calib_accuracy.txt")).read()
    m = re.search(r"^\s*shipped \.yfm on the engine / host build on the npz weights\s+[\d.]+\s+[\d.]+\s+(\d+\.(\d+))\s+\d+\s*$", text, re.M)
    assert m, "profiles/calib_accuracy.txt: the shipped pair's row of section 4 was not found"
    return float(m.group(1)), 0.5 * 10.0 ** -len(m.group(2))
