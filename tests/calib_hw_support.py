"""What the tests of calibration at h x w share (test_calib_hw_host.py, test_calib_hw_gpu.py): the sizes, the frames at each of them (the
reference's 27 sample frames brought to 160x160 as OpenCV would, seeded and structured frames at the small sizes), the host build's results,
the float32 tensors and the oracle's int8 tensors at a size, and bit-wise comparisons.  Everything is computed once per process."""
import functools
import os

import numpy as np

from conftest import GOLDEN
import calib_support as cs
import calib_hist_support as hs
import quant_support as qs
from calib_support import calib, ptq

# 8x8: one head cell, every window clipped; 16x24 and 24x8: not square (an h / w swap shows); 56x56: the LDS form's size; 160x160: the engine's other size
SMALL = ((8, 8), (16, 24), (24, 8))
SIZES = SMALL + ((56, 56), (160, 160))


def cells(h, w):
    return (h // 8) * (w // 8)


@functools.lru_cache(maxsize=None)
def frames160():
    """the reference's 27 sample frames (tests/golden/real_frames_56.bin) at 160x160 through ptq.resize_linear_u8: int8 [27, 160, 160, 3]"""
    x = np.fromfile(os.path.join(GOLDEN, "real_frames_56.bin"), np.int8).reshape(-1, 56, 56, 3)
    assert x.shape[0] == 27
    u = (x.astype(np.int16) + 128).astype(np.uint8)
    out = np.stack([ptq.resize_linear_u8(f, 160, 160) for f in u]).reshape(27, 160, 160, 3)
    out = np.ascontiguousarray((out.astype(np.int16) - 128).astype(np.int8))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def real56():
    x = np.fromfile(os.path.join(GOLDEN, "real_frames_56.bin"), np.int8).reshape(-1, 56, 56, 3)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def frames(h, w, n, seed=0):
    """n frames int8 [n, h, w, 3]: black, white and a one-pixel checkerboard first (where n allows), then seeded random ones.  At 160x160 the
    first of the 27 upscaled frames instead: real content."""
    if (h, w) == (160, 160):
        assert n <= 27
        return frames160()[:n]
    rng = np.random.default_rng(1000 * h + w + seed)
    x = rng.integers(-128, 128, (n, h, w, 3), dtype=np.int8)
    yy, xx = np.mgrid[:h, :w]
    structured = [np.full((h, w, 3), -128, np.int8), np.full((h, w, 3), 127, np.int8),
                  np.where(((yy + xx) & 1)[..., None] == 1, np.int8(127), np.int8(-128)) + np.zeros((h, w, 3), np.int8)]
    for i, s in enumerate(structured[:max(n - 2, 0)]):
        x[i] = s
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def host_result(name, h, w, n):
    """(ranges, logits [n, h / 8, w / 8, 18]) of the host build on frames(h, w, n); at (56, 56) on the 27 calibration frames, general form"""
    x = cs.calib_frames() if (h, w) == (56, 56) else frames(h, w, n)
    r, lg = calib.host_run(cs.yfw_bytes(name), x, threads=16, general=True)
    lg.setflags(write=False)
    return r, lg


def elements(h, w):
    """elements per frame of the 47 slots at h x w"""
    return tuple(calib.elements_at(e, h, w) for e in hs.elements())


def float_tensors(x, name="yfw"):
    """[47 float32 arrays [n, elements]] of frames x [n, h, w, 3]: the input through the table, the other 46 from host_compare's evaluation"""
    n, h, w, _ = x.shape
    el = elements(h, w)
    table = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)
    entries = [calib.Entry(t, 1.0, 0, np.zeros((n, e), np.int8), e) for t, e in zip(hs.slots()[1:], el[1:])]
    _, _, xs = calib.host_compare(cs.yfw_bytes(name), x, entries, threads=16, want_tensors=True, elements=list(el[1:]), general=True)
    return [table[x.reshape(n, -1).astype(np.int32) + 128]] + list(xs)


@functools.lru_cache(maxsize=None)
def dump_layout(h, w):
    """(sizes, offsets) of the oracle's per-op dump at h x w, from the shapes the restatement gives every op output"""
    from oracle.np_restatement import NpModel
    _, outs = NpModel(cs.SHIPPED_YFM).run(np.zeros((h, w, 3), np.int8), dump=True)
    sizes = [int(np.asarray(o).size) for o in outs]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    assert int(offs[-1]) == qs._oracle().dump_bytes(h, w)
    return sizes, offs


def oracle_q(x):
    """per tensor of quant_support.tensors(): the shipped model's int8 values [n, elements at h x w] of the oracle on frames x"""
    n, h, w, _ = x.shape
    heads, dump = qs._oracle().run(np.ascontiguousarray(x), dump=True, threads=16)
    heads = np.ascontiguousarray(heads.reshape(n, -1))
    sizes, offs = dump_layout(h, w)
    out = []
    for t in qs.tensors():
        e = calib.elements_at(t["elements"], h, w)
        if t["offset"] is None:
            assert heads.shape[1] == e
            out.append(heads)
        else:
            assert sizes[t["op"]] == e, (t, sizes[t["op"]], e)
            out.append(np.ascontiguousarray(dump[:, offs[t["op"]]:offs[t["op"]] + e]))
    return out


def lsb_errors(heads, logits, scale, zp):
    """|dequantised head - float logit| / output scale"""
    return np.abs((heads.astype(np.float64) - zp) * float(scale) - logits.astype(np.float64)) / float(scale)


def rmse(heads, logits, scale, zp):
    """of the dequantised head against the float logits, in real units"""
    e = (heads.astype(np.float64) - zp) * float(scale) - logits.astype(np.float64)
    return float(np.sqrt(np.mean(e * e)))


def union(a, b):
    """the element-wise union of two range dicts"""
    return {t: (min(a[t][0], b[t][0]), max(a[t][1], b[t][1])) for t in a}
