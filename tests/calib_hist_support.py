"""What the histogram tests share (test_calib_hist_host.py, test_calib_hist_gpu.py): the 47 slots and their element counts, the float32 tensors
of a set of frames (calib.host_compare with want_tensors, and the input table), the numpy restatement of csrc/yf_calib_hist.h's binning, and
the host build's histograms of the 27 calibration frames, each computed once per process."""
import functools

import numpy as np

import calib_support as cs
from calib_support import calib, model_file

YFW = "yfw"


@functools.lru_cache(maxsize=None)
def slots():
    """the tensor ids in slot order, as the host build reports them"""
    return tuple(sorted(cs.host_result(YFW)[0]))


@functools.lru_cache(maxsize=None)
def elements():
    """elements per frame of every slot"""
    shapes = model_file.load_graph()["tensors"]
    return tuple(int(np.prod(shapes[t]["shape"][1:])) for t in slots())


def float_tensors(frames, yfw=None):
    """[47 float32 arrays [n, elements]]: the input through the table T[p] = float32(p / 255.0), the other 46 from the host build's evaluation"""
    x = np.ascontiguousarray(frames, np.int8).reshape(-1, 56, 56, 3)
    n = x.shape[0]
    table = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)
    entries = [calib.Entry(t, 1.0, 0, np.zeros((n, e), np.int8), e) for t, e in zip(slots()[1:], elements()[1:])]
    _, _, xs = calib.host_compare(cs.yfw_bytes(YFW) if yfw is None else yfw, x, entries, threads=16, want_tensors=True, elements=list(elements()[1:]))
    return [table[x.reshape(n, -1).astype(np.int32) + 128]] + list(xs)


def restate_bins(v, lo, hi, bins):
    """csrc/yf_calib_hist.h in numpy, float32, the same three operations: the axis from {min, max}, then the bin of every value"""
    lo, hi = np.float32(lo), np.float32(hi)
    with np.errstate(all="ignore"):
        q = np.float32(bins) / np.float32(hi - lo)
        inv = np.float32(0) if hi <= lo or not np.isfinite(q) else q
        t = (np.asarray(v, np.float32) - lo) * inv
        return np.where(t >= np.float32(bins), bins - 1, np.where(t > 0, np.trunc(t), 0)).astype(np.int64)


def restate(tensors, ranges, bins):
    """the histograms of float_tensors' arrays on the axes of `ranges`: uint64 [47, bins]"""
    out = np.zeros((len(slots()), bins), np.uint64)
    for i, (t, x) in enumerate(zip(slots(), tensors)):
        out[i] = np.bincount(restate_bins(x.reshape(-1), *ranges[t], bins), minlength=bins).astype(np.uint64)
    return out


def first_difference(got, want):
    """(tensor, bin, got, want) of the first differing count, or None"""
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    if not bad.shape[0]:
        return None
    r, k = (int(v) for v in bad[0])
    return slots()[r], k, int(got[r, k]), int(want[r, k])


def assert_same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint64, (what, got.shape, got.dtype)
    d = first_difference(got, want)
    assert d is None, f"{what}: (tensor, bin, got, want) = {d}, {int((got != want).sum())} counts differ"


def assert_conserved(counts, n, what):
    sums = counts.sum(axis=1, dtype=np.uint64)
    want = np.array(elements(), np.uint64) * np.uint64(n)
    bad = [(slots()[i], int(sums[i]), int(want[i])) for i in range(len(slots())) if sums[i] != want[i]]
    assert not bad, f"{what}: (tensor, sum of its counts, n x elements) = {bad[0]} ({len(bad)} tensors)"


@functools.lru_cache(maxsize=None)
def host_counts(bins):
    """the host build's histograms of the 27 calibration frames on the axes of their own ranges"""
    c = calib.host_histogram(cs.yfw_bytes(YFW), cs.calib_frames(), cs.host_result(YFW)[0], bins, threads=16)
    c.setflags(write=False)
    return c
