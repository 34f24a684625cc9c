"""Designed weight packs for the float calibration library, and a plain numpy restatement of the arithmetic csrc/yf_calib_arith.h and
csrc/yf_calib_sim.h DEFINE, written from the definition's text and the graph alone (model_file.load_graph) -- none of the four headers'
tables is copied here.  What test_calib_packs_host.py and test_calib_packs_gpu.py share.

THE RESTATEMENT (evaluate): float32 numpy arrays, one elementwise operation per line.  The input is T[q + 128], T[p] = float32(p / 255.0);
a convolution is acc = 0, then for fy, for fx, for ci over whole output planes: p = x * w, acc = acc + p, the product and the sum rounded
separately; a tap in the padding updates nothing (a masked update, as the definition words it; with finite weights adding `0 * w` gives
the same bits, since an accumulator that starts at +0 is never -0); then + bias, y >= 0 ? y : y * float32(0x3dcccccd), the ADD a + b,
the pools from -inf with t > y in window order, the concatenations.
Modes: "defined"; "contracted" (every step float32(float64(acc) + float64(x) * float64(w)): what an fma build would compute);
"flushed" (subnormal operands and results are zero: what a build that flushes float32 subnormals would compute).  The two mutated modes
exist for the certificates only: they show that a pack would notice such a build.  With a table (50 entries of calib.SIM_ENTRY) the enabled
tensors are put on their int8 grids where they are produced: t = v * inv, r = rint(t), clip, count, c * scale.

THE PACKS are weight sets built in memory from the shipped .yfw, seeded, written nowhere.  The device: a convolution k whose weights are
all zero leaves acc at +0, so its output is bias[co] exactly at every pixel, for any finite frame -- that PLANTS cout chosen float32 values
in a tensor; the weights of convolution k + 1 then decide what its channels become.  A non-finite value in any channel of a pixel turns
every channel of every later dense convolution into NaN at that pixel (0 * inf is NaN), so what one weight set can reach is limited and
the value classes are spread over several sets:
  subnormal     conv 2 plants four values around 2^-126, conv 3 (weights below 1, subnormal biases) sums them and its LeakyReLU gives
                subnormals and one -0 (28x28); conv 20 plants forty, the depthwise conv 21 has taps of opposite sign, so its border
                differs from its interior, and convs 22 and 23 carry subnormals into the logits (7x7)
  overflow      conv 2 plants +-3e38, conv 3 doubles them: tensor 56 has finite, +inf, -inf and NaN channels in front of a LeakyReLU (57),
                a pool (58: the all-NaN windows give -inf) and, through the pool, a concatenation (71); from tensor 62 on every
                tensor is NaN at every element and its range slot keeps the sentinels (+inf, -inf)
  overflow_add  conv 7 plants, conv 8 overflows: tensor 67 has finite, +-inf and NaN channels and meets the finite tensor 62 in the
                residual ADD (68)
  overflow_gate no plant: convs 0 to 3 are wired so that tensor 56 is NaN where the frame's red value is 0 or 255 and finite elsewhere.  The
                pack's frames (black, white, random extremes) make it NaN at every element; real frames do not: the accumulation case
  rint_a/rint_b conv 22 plants 32 values, conv 23 selects and sums them (weights 0, +-1, +-2): under an entry for tensor 100 with scale 0.5
                and zero point 3 the 18 logits are ties of both signs and parities, |t| < 0.5, the six values around lo and hi, 2^23 - 0.5
                to 2^24, subnormal t, t = +-inf from 3e38 * 2, and a NaN; an entry for tensor 98 (a convolution's output in front of a
                LeakyReLU) meets the 32 planted values themselves
  rint_pool / rint_pool_b   conv 3 plants 18 values whose LeakyReLU results the pool 58 hands to the QUANTIZE entry of tensor 103: over
                the two sets the same classes as on tensor 100, except the NaN (a pool never gives one: its all-NaN window is -inf)
  shipped_npz / shipped_yfw   the two real weight sets
"""
import collections
import functools

import numpy as np

import calib_support as cs
from calib_support import calib, model_file

F32 = np.float32
TINY = F32(2.0 ** -126)                   # the smallest normal float32
SUB = F32(2.0 ** -131)
BIG = F32(3e38)
SIZES = ((8, 8), (16, 24), (56, 56))      # 8x8: one head cell, every window clipped; 16x24: not square; 56x56: the LDS form's size
N_FRAMES = 3
RINT_SCALE, RINT_ZP = F32(0.5), 3         # lo = -131, hi = 124; t = 2 v exactly


# ---------------------------------------------------------------------------------------------------------------- comparisons
def _bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype in (np.float32, np.float64), a.dtype
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def differing(got, want):
    """the indices at which two float arrays of one shape and type differ: by their bits (both zeros are told apart), except that a NaN
    equals any NaN -- x86 and the GPU give inf - inf different signs and payloads, which is not the library's business"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, got.dtype, want.shape, want.dtype)
    return np.argwhere((_bits(got) != _bits(want)) & ~(np.isnan(got) & np.isnan(want)))


def same_floats(got, want):
    return differing(got, want).shape[0] == 0


def assert_same_floats(got, want, what):
    d = differing(got, want)
    if d.shape[0]:
        i = tuple(d[0])
        raise AssertionError(f"{what}: {d.shape[0]} of {np.asarray(got).size} values differ, first at {i}: {np.asarray(got)[i]!r} "
                             f"({int(_bits(got)[i]):#x}) against {np.asarray(want)[i]!r} ({int(_bits(want)[i]):#x})")


def assert_same_records(got, want, what):
    """two record arrays (calib.FRAME_STATS or calib.TOTALS): the float and double fields under same_floats, the others equal"""
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {got.shape} against {want.dtype} {want.shape}"
    for name in got.dtype.names:
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        if a.dtype.kind == "f":
            assert_same_floats(a, b, f"{what}, field {name}")
        else:
            bad = np.argwhere(a != b)
            assert not bad.shape[0], f"{what}, field {name}: first at {tuple(bad[0])}: {a[tuple(bad[0])]} against {b[tuple(bad[0])]}"


def assert_same_ranges(got, want, what):
    """{tensor: (min, max)} by bits; a NaN end is a failure whatever the other side holds"""
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for t in sorted(got):
        a, b = np.array(got[t], F32), np.array(want[t], F32)
        assert not np.isnan(a).any(), f"{what}: tensor {t} has a NaN end {tuple(a)}"
        assert (_bits(a) == _bits(b)).all(), f"{what}: tensor {t}: {tuple(a)!r} against {tuple(b)!r}"


# ---------------------------------------------------------------------------------------------------------------- the restatement
@functools.lru_cache(maxsize=None)
def graph():
    return model_file.load_graph()


@functools.lru_cache(maxsize=None)
def slot_tensors():
    """the 47 observed tensors in slot order (ascending id): the input and every CONV_2D, DEPTHWISE_CONV_2D, LEAKY_RELU, ADD and MAX_POOL_2D
    output of the graph"""
    O, g = model_file.OPCODE, graph()
    kinds = [O[k] for k in ("CONV_2D", "DEPTHWISE_CONV_2D", "LEAKY_RELU", "ADD", "MAX_POOL_2D")]
    return tuple(sorted([g["input"]] + [o["out"] for o in g["ops"] if o["op"] in kinds]))


@functools.lru_cache(maxsize=None)
def entry_tensors():
    """the tensor of each of the 50 entries of a simulation table: the slots, then the QUANTIZE outputs in ascending id"""
    O, g = model_file.OPCODE, graph()
    return slot_tensors() + tuple(sorted(o["out"] for o in g["ops"] if o["op"] == O["QUANTIZE"]))


def _ftz(a):
    a = np.asarray(a, F32)
    return np.where(np.abs(a) < TINY, np.copysign(F32(0), a), a).astype(F32)


class _Arith:
    def __init__(self, mode):
        assert mode in ("defined", "contracted", "flushed"), mode
        self.mode = mode

    def mac(self, acc, x, w):
        if self.mode == "contracted":
            return (acc.astype(np.float64) + x.astype(np.float64) * w.astype(np.float64)).astype(F32)
        if self.mode == "flushed":
            p = _ftz(_ftz(x) * _ftz(w))
            return _ftz(_ftz(acc) + p)
        p = x * w
        return acc + p

    def add(self, a, b):
        if self.mode == "flushed":
            return _ftz(_ftz(a) + _ftz(b))
        return a + b

    def mul(self, a, b):
        if self.mode == "flushed":
            return _ftz(_ftz(a) * _ftz(b))
        return a * b


def _taps(size, out, k, stride, before):
    """per tap f: (first, count, source) -- the outputs first .. first + count - 1 are those whose tap f lies inside the input; the first of
    them reads input index `source`"""
    res = []
    for f in range(k):
        o0 = max(0, -((f - before) // stride))
        o1 = min(out - 1, (size - 1 + before - f) // stride)
        res.append((o0, o1 - o0 + 1, o0 * stride + f - before))
    return res


def _windows(x, k, stride, top, left, oh, ow):
    """for fy, for fx: (the output region the tap updates, the input values it reads there)"""
    _, h, w, _ = x.shape
    ty, tx = _taps(h, oh, k, stride, top), _taps(w, ow, k, stride, left)
    for fy in range(k):
        oy, ny, iy = ty[fy]
        for fx in range(k):
            ox, nx, ix = tx[fx]
            if ny < 1 or nx < 1:
                continue
            region = (slice(None), slice(oy, oy + ny), slice(ox, ox + nx))
            yield fy, fx, region, x[:, iy:iy + (ny - 1) * stride + 1:stride, ix:ix + (nx - 1) * stride + 1:stride, :]


def _conv(x, w, depthwise, stride, top, left, oh, ow, ar):
    cout = w.shape[3] if depthwise else w.shape[0]
    acc = np.zeros((x.shape[0], oh, ow, cout), F32)
    for fy, fx, region, src in _windows(x, w.shape[1], stride, top, left, oh, ow):
        if depthwise:
            acc[region] = ar.mac(acc[region], src, w[0, fy, fx, :])
        else:
            for ci in range(x.shape[3]):
                acc[region] = ar.mac(acc[region], src[..., ci, None], w[:, fy, fx, ci])
    return acc


def _pool(x, k, stride, top, left, oh, ow):
    y = np.full((x.shape[0], oh, ow, x.shape[3]), -np.inf, F32)
    for _, _, region, t in _windows(x, k, stride, top, left, oh, ow):
        y[region] = np.where(t > y[region], t, y[region])
    return y


def _same_padding(size, k, stride):
    out = -(-size // stride)
    return out, max((out - 1) * stride + k - size, 0) // 2


def sim_q(v, scale, zero_point):
    """a tensor on its grid -> (the values, the number clipped per frame)"""
    scale = F32(scale)
    inv = F32(1.0 / np.float64(scale))
    lo, hi = F32(-128 - int(zero_point)), F32(127 - int(zero_point))
    t = v * inv
    r = np.rint(t)
    below = r < lo
    above = r > hi
    c = np.where(below, lo, np.where(above, hi, r)).astype(F32)
    out = c * scale
    assert t.dtype == r.dtype == out.dtype == F32
    return out, (below | above).reshape(v.shape[0], -1).sum(axis=1).astype(np.int64)


Result = collections.namedtuple("Result", "tensors logits clipped")


def evaluate(convs, frames, mode="defined", table=None):
    """convs: [(weights, bias, depthwise)] as model_file.read_yfw gives them; frames int8 [n, h, w, 3] -> Result(tensors {id: float32
    [n, oh, ow, c]} for the 47 observed tensors, logits [n, h / 8, w / 8, 18], clipped int64 [n])"""
    O, g, ar = model_file.OPCODE, graph(), _Arith(mode)
    frames = np.asarray(frames, np.int8)
    n = frames.shape[0]
    T = np.array([F32(p / 255.0) for p in range(256)], F32)
    entry = {t: i for i, t in enumerate(entry_tensors())}
    vals, pads, tensors, clipped = {}, {}, {}, np.zeros(n, np.int64)

    def produced(t, v):
        assert v.dtype == F32, (t, v.dtype)
        if table is not None and t in entry and table[entry[t]]["scale"] != 0:
            v, k = sim_q(v, table[entry[t]]["scale"], table[entry[t]]["zero_point"])
            clipped[:] = clipped + k
        vals[t] = v
        if t in slot_tensors():
            tensors[t] = v

    conv_at = 0
    with np.errstate(all="ignore"):
        produced(g["input"], T[frames.astype(np.int32) + 128])
        for o in g["ops"]:
            x = vals[o["ins"][0]]
            if o["op"] == O["PAD"]:
                p = np.asarray(g["tensors"][o["ins"][1]]["data"]).reshape(4, 2)
                assert not p[0].any() and not p[3].any()
                vals[o["out"]], pads[o["out"]] = x, (int(p[1][0]), int(p[1][1]), int(p[2][0]), int(p[2][1]))
            elif o["op"] in (O["CONV_2D"], O["DEPTHWISE_CONV_2D"]):
                w, b, dw = convs[conv_at]
                conv_at += 1
                w, b = np.asarray(w, F32), np.asarray(b, F32)
                assert bool(dw) == (o["op"] == O["DEPTHWISE_CONV_2D"]) and o["sw"] == o["sh"] and w.shape[1] == w.shape[2]
                k, s = w.shape[1], o["sw"]
                if o["padding"] == 1:                                              # VALID over the explicit PAD in front
                    top, bottom, left, right = pads.get(o["ins"][0], (0, 0, 0, 0))
                    oh, ow = (x.shape[1] + top + bottom - k) // s + 1, (x.shape[2] + left + right - k) // s + 1
                else:
                    (oh, top), (ow, left) = _same_padding(x.shape[1], k, s), _same_padding(x.shape[2], k, s)
                acc = _conv(x, w, bool(dw), s, top, left, oh, ow, ar)
                produced(o["out"], ar.add(acc, b))
            elif o["op"] == O["LEAKY_RELU"]:
                alpha = np.array([o["alpha_bits"]], "<u4").view("<f4")[0]
                scaled = ar.mul(x, alpha)
                produced(o["out"], np.where(x >= 0, x, scaled).astype(F32))
            elif o["op"] == O["MAX_POOL_2D"]:
                assert o["padding"] == 0 and o["fw"] == o["fh"] and o["sw"] == o["sh"]
                (oh, top), (ow, left) = _same_padding(x.shape[1], o["fh"], o["sh"]), _same_padding(x.shape[2], o["fw"], o["sw"])
                produced(o["out"], _pool(x, o["fh"], o["sh"], top, left, oh, ow))
            elif o["op"] == O["ADD"]:
                produced(o["out"], ar.add(x, vals[o["ins"][1]]))
            elif o["op"] == O["QUANTIZE"]:
                produced(o["out"], x)
            elif o["op"] == O["CONCATENATION"]:
                assert o["axis"] == 3
                vals[o["out"]] = np.concatenate([x, vals[o["ins"][1]]], axis=3)
            else:
                raise AssertionError(f"op {o['op']} is not restated")
    assert conv_at == len(convs) and sorted(tensors) == list(slot_tensors())
    return Result(tensors, vals[g["output"]], clipped)


def ranges_of(tensors):
    """{tensor: (min, max)} as the library reports them: a NaN never becomes an extreme, a tensor without a number keeps (+inf, -inf), and a
    zero comes out as +0"""
    out = {}
    for t, v in tensors.items():
        v = v[~np.isnan(v)]
        lo, hi = (v.min(), v.max()) if v.size else (F32(np.inf), F32(-np.inf))
        out[t] = (float(F32(lo) + F32(0)), float(F32(hi) + F32(0)))
    return out


# ---------------------------------------------------------------------------------------------------------------- the packs
Pack = collections.namedtuple("Pack", "name convs yfw tables extremes")


def _f32(bits):
    return np.array([bits], "<u4").view("<f4")[0]


ALPHA = _f32(0x3DCCCCCD)


def unleak(target):
    """a negative float32 b with float32(b * alpha) == target, target < 0"""
    target = F32(target)
    b = F32(np.float64(target) / np.float64(ALPHA))
    for _ in range(64):
        got = F32(b * ALPHA)
        if got == target:
            return b
        b = np.nextafter(b, F32(-np.inf) if got > target else F32(0), dtype=F32)
    raise AssertionError(f"no float32 whose LeakyReLU is {target!r}")


def one_entry(tensor, scale, zero_point):
    t = calib.empty_table()
    t[entry_tensors().index(tensor)] = (F32(scale), int(zero_point))
    return t


def _base():
    return [[np.array(w, F32), np.array(b, F32), dw] for w, b, dw in model_file.read_yfw(cs.yfw_bytes("yfw"))]


def _plant(convs, k, values):
    values = np.asarray(values, F32)
    assert values.shape == convs[k][1].shape and np.isfinite(values).all(), (k, values.shape, convs[k][1].shape)
    convs[k][0], convs[k][1] = np.zeros_like(convs[k][0]), values


def _dense(convs, k, rows, bias=None):
    """conv k (1x1): output channel co = sum of weight * input channel over rows[co] = [(input channel, weight), ...]"""
    w = np.zeros_like(convs[k][0])
    assert w.shape[1] == 1 and len(rows) == w.shape[0], (k, w.shape, len(rows))
    for co, row in enumerate(rows):
        for ci, v in row:
            w[co, 0, 0, ci] = F32(v)
    convs[k][0] = w
    if bias is not None:
        convs[k][1] = np.asarray(bias, F32).reshape(convs[k][1].shape)


def _subnormal():
    rng, c = np.random.default_rng(126), _base()
    _plant(c, 2, [1.5 * TINY, 0.75 * TINY, -1.25 * TINY, -0.5 * TINY])
    w = (rng.uniform(0.05, 0.95, c[3][0].shape) * rng.choice([-1.0, 1.0], c[3][0].shape)).astype(F32)
    b = (rng.uniform(1, 64, 18) * rng.choice([-1.0, 1.0], 18) * 2.0 ** -140).astype(F32)
    w[0], b[0] = 0, -2.0 ** -149                        # tensor 56 channel 0 is the smallest negative float32: its LeakyReLU underflows to -0
    w[1], b[1] = 0, 2.0 ** -149
    c[3][0], c[3][1] = w, b
    _plant(c, 20, (rng.uniform(0.25, 4.0, 40) * rng.choice([-1.0, 1.0], 40)).astype(F32) * TINY)
    a = rng.uniform(0.1, 0.9, 40).astype(F32)
    signs = np.array([[1, -1, 1], [-1, 0.5, -1], [1, -1, 1]], F32)        # (the full window sums to a/2 x the channel's value; a border misses taps)
    c[21][0] = (signs[None, :, :, None] * a[None, None, None, :]).astype(F32)
    c[21][1] = (rng.uniform(1, 64, 40) * rng.choice([-1.0, 1.0], 40) * 2.0 ** -140).astype(F32)
    c[22][1], c[23][1] = np.zeros_like(c[22][1]), np.zeros_like(c[23][1])
    tiny_scale = F32(2.0 ** -127)                       # a subnormal scale whose reciprocal is finite: t = v * 2^127
    table = calib.empty_table()
    for t in (57, 97, 100):
        table[entry_tensors().index(t)] = (tiny_scale, 0)
    return c, {"57+97+100 at 2^-127": table, "56 at 2^-126": one_entry(56, TINY, 127)}


def _overflow():
    rng, c = np.random.default_rng(38), _base()
    _plant(c, 2, [BIG, -BIG, 1.0, -2.0])
    rows = [[(0, 2)], [(1, 2)], [(0, 2), (1, 2)], [(2, 1), (3, 1)], [(0, -2)], [(0, 2), (2, 1)], [(1, 2), (3, -1)], [(1, -2), (0, 2)]]
    rows += [[(2, rng.uniform(-2, 2)), (3, rng.uniform(-2, 2))] for _ in range(10)]
    _dense(c, 3, rows)
    return c, {"56": one_entry(56, RINT_SCALE, RINT_ZP), "103": one_entry(103, RINT_SCALE, RINT_ZP), "57 and 58": _two(57, 58)}


def _two(a, b):
    t = one_entry(a, RINT_SCALE, RINT_ZP)
    t[entry_tensors().index(b)] = (F32(0.25), -7)
    return t


def _overflow_add():
    rng, c = np.random.default_rng(68), _base()
    planted = rng.uniform(-2, 2, 36).astype(F32)
    planted[:4] = [BIG, BIG, 1.0, 0.5]
    _plant(c, 7, planted)
    rows = [[(0, 2)], [(0, -2)], [(0, 2), (1, -2)], [(2, 1), (3, 1)], [(0, 2), (2, 3)], [(k, rng.uniform(-1, 1)) for k in range(2, 36)]]
    _dense(c, 8, rows)
    return c, {"67": one_entry(67, RINT_SCALE, RINT_ZP), "68": one_entry(68, RINT_SCALE, RINT_ZP)}


def _overflow_gate():
    """x the red value of a pixel: tensor 52 holds A = 3e38 x and B = 3e38 (1 - x); the depthwise conv 1 passes them; conv 2 forms 1.25 A,
    1.25 B, -1.25 A and -1.25 B, of which two are infinite where x is 0 or 1 and none is elsewhere; conv 3 adds the four with small
    positive weights: inf - inf where x is 0 or 1, a finite sum elsewhere"""
    rng, c = np.random.default_rng(55), _base()
    w0, b0 = c[0][0] * F32(0.25), c[0][1].copy()
    w0[:2], b0[:2] = 0, [0, BIG]
    w0[0, 1, 1, 0], w0[1, 1, 1, 0] = BIG, -BIG
    c[0][0], c[0][1] = w0, b0
    w1 = np.zeros_like(c[1][0])
    w1[0, 1, 1, :] = 1
    c[1][0], c[1][1] = w1, np.zeros_like(c[1][1])
    _dense(c, 2, [[(0, 1.25)], [(1, 1.25)], [(0, -1.25)], [(1, -1.25)]])
    c[3][0] = rng.uniform(0.01, 0.1, c[3][0].shape).astype(F32)
    return c, {"55": one_entry(55, RINT_SCALE, RINT_ZP)}


# the 32 values conv 22 plants in the rint packs: 21 positive ones (their LeakyReLU is themselves) for conv 23 to select, 11 negative
RINT_PLANTED = [0.25, 0.5, 1.25, F32(0.15), 65.5, 65.75, 66, 62, 62.25, 62.5, 2.0 ** 22 - 0.25, 2.0 ** 22, 2.0 ** 22 + 0.5, 2.0 ** 23, BIG, SUB, 1.75, 2.25,
                1.0, F32(0.1), F32(50.15),
                -0.25, -0.75, -1.25, -F32(0.15), -65.5, -65.75, -66, -(2.0 ** 22 - 0.25), -(2.0 ** 23), -BIG, -SUB]


def _pick(value, weight=1):
    return (RINT_PLANTED.index(value), weight)


def _rint(which):
    c = _base()
    _plant(c, 22, RINT_PLANTED)
    if which == "a":        # t = 2 v:  0.5  1.5  2.5  -0.5  -1.5  -2.5  0.3  -0.3  lo  lo-.5  lo-1  hi  hi+.5  hi+1  2^23-.5  2^23  2^23+1  2^24
        rows = [[_pick(0.25)], [_pick(0.25), _pick(0.5)], [_pick(1.25)], [_pick(0.25, -1)], [_pick(0.25, -1), _pick(0.5, -1)], [_pick(1.25, -1)],
                [_pick(F32(0.15))], [_pick(F32(0.15), -1)], [_pick(65.5, -1)], [_pick(65.75, -1)], [_pick(66, -1)], [_pick(62)], [_pick(62.25)],
                [_pick(62.5)], [_pick(2.0 ** 22 - 0.25)], [_pick(2.0 ** 22)], [_pick(2.0 ** 22 + 0.5)], [_pick(2.0 ** 23)]]
    else:                   # t:  +inf  -inf  NaN  +inf (the logit itself)  sub  -sub  -(2^23-.5)  -2^23  -(2^23+1)  -2^24  3.5  -3.5  4.5  -4.5  2  -2  0.2  100.3
        rows = [[_pick(BIG)], [_pick(BIG, -1)], [_pick(BIG, 2), _pick(-BIG, 20)], [_pick(BIG, 2)], [_pick(SUB)], [_pick(SUB, -1)],
                [_pick(2.0 ** 22 - 0.25, -1)], [_pick(2.0 ** 22, -1)], [_pick(2.0 ** 22 + 0.5, -1)], [_pick(2.0 ** 23, -1)], [_pick(1.75)], [_pick(1.75, -1)],
                [_pick(2.25)], [_pick(2.25, -1)], [_pick(1.0)], [_pick(1.0, -1)], [_pick(F32(0.1))], [_pick(F32(50.15))]]
    _dense(c, 23, rows, np.zeros(18, F32))
    tables = {"100": one_entry(100, RINT_SCALE, RINT_ZP), "100 at 2^-100": one_entry(100, 2.0 ** -100, 0)}
    if which == "a":
        tables["98"] = one_entry(98, RINT_SCALE, RINT_ZP)
    return c, tables


# what the pool hands the QUANTIZE entry of tensor 103 in rint_pool and rint_pool_b: the LeakyReLU of conv 3's planted biases.  Conv 3 has 18
# channels, so the classes take two weight sets; a negative value is met only where it is the LeakyReLU of some float32 (unleak finds it)
POOL_VALUES = {"a": [0.25, 0.75, 1.25, F32(0.15), 62, 62.25, 62.5, 2.0 ** 22 - 0.25, 2.0 ** 40, F32(-(2.0 ** 45)) * ALPHA, SUB,
                     -0.25, -0.75, -F32(0.15), -65.5, -65.75, -66, -(2.0 ** 22)],
               "b": [2.0 ** 22 + 0.5, -(2.0 ** 22 + 0.5), 2.0 ** 23, -(2.0 ** 23), 2.0 ** 22, -(2.0 ** 22 - 0.25), -1.25, -SUB, 1.75, -1.75, 2.25, -2.25,
                     F32(0.1), -F32(0.1), F32(50.15), -F32(50.15), 1.0, -1.0]}


def _rint_pool(which):
    c = _base()
    _plant(c, 3, [v if v > 0 else unleak(v) for v in POOL_VALUES[which]])
    return c, {"103": one_entry(103, RINT_SCALE, RINT_ZP), "103 at 2^-100": one_entry(103, 2.0 ** -100, 0), "56": one_entry(56, RINT_SCALE, RINT_ZP)}


def _shipped(name):
    import quant_support as qs
    c = [[np.array(w, F32), np.array(b, F32), dw] for w, b, dw in model_file.read_yfw(cs.yfw_bytes(name))]
    return c, {"the shipped model's 50 entries": calib.simulation_table(qs.shipped_yfm()), "66": one_entry(66, 0.03125, -100)}


_BUILDERS = collections.OrderedDict([
    ("subnormal", _subnormal), ("overflow", _overflow), ("overflow_add", _overflow_add), ("overflow_gate", _overflow_gate),
    ("rint_a", lambda: _rint("a")), ("rint_b", lambda: _rint("b")), ("rint_pool", lambda: _rint_pool("a")),
    ("rint_pool_b", lambda: _rint_pool("b")),
    ("shipped_npz", lambda: _shipped("npz")), ("shipped_yfw", lambda: _shipped("yfw"))])
NAMES = tuple(_BUILDERS)


@functools.lru_cache(maxsize=None)
def pack(name):
    convs, tables = _BUILDERS[name]()
    convs = [(w, b, dw) for w, b, dw in convs]
    for w, b, _ in convs:
        w.setflags(write=False)
        b.setflags(write=False)
    return Pack(name, convs, model_file.write_yfw(convs), tables, name == "overflow_gate")


@functools.lru_cache(maxsize=None)
def frames(name, h, w):
    """the pack's three frames at h x w: black, white, and a seeded random one -- of pixels at 0 or 255 only where the pack asks for extremes"""
    rng = np.random.default_rng(100 * h + w)
    x = np.empty((N_FRAMES, h, w, 3), np.int8)
    x[0], x[1] = -128, 127
    x[2] = rng.choice(np.array([-128, 127], np.int8), (h, w, 3)) if pack(name).extremes else rng.integers(-128, 128, (h, w, 3), dtype=np.int8)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def restated(name, h, w, mode="defined"):
    return evaluate(pack(name).convs, frames(name, h, w), mode)


@functools.lru_cache(maxsize=None)
def simulated(name, h, w, label):
    return evaluate(pack(name).convs, frames(name, h, w), "defined", pack(name).tables[label])


def flat_tensors(result):
    """the 47 tensors [n, elements] in slot order: what calib_hist_support.restate and the comparisons take"""
    return [np.ascontiguousarray(result.tensors[t].reshape(N_FRAMES, -1)) for t in slot_tensors()]


def inner_ranges(result):
    """per tensor a finite range INSIDE its data (the quartiles of its finite values), so that the rest, +-inf and NaN with it, lands in the
    end bins; (-1, 1) for a tensor without a finite value"""
    out = {}
    for t in slot_tensors():
        v = np.sort(result.tensors[t][np.isfinite(result.tensors[t])])
        out[t] = (float(v[v.size // 4]), float(v[(3 * v.size) // 4])) if v.size else (-1.0, 1.0)
    return out


@functools.lru_cache(maxsize=None)
def compare_entries(name, h, w):
    """([calib.Entry] over the 46 stage tensors with seeded int8 values -- -128 and 127 among them --, their scales, zero points and values)"""
    r, rng = restated(name, h, w), np.random.default_rng(46)
    ids = slot_tensors()[1:]
    qs = [rng.integers(-128, 128, (N_FRAMES, r.tensors[t][0].size), dtype=np.int8) for t in ids]
    scales = [F32(2.0 ** -(i % 7)) * F32(1 + (i % 3)) for i in range(len(ids))]
    zps = [int(v) for v in rng.integers(-128, 128, len(ids))]
    return [calib.Entry(t, s, z, q, q.shape[1]) for t, s, z, q in zip(ids, scales, zps, qs)], scales, zps, qs


# ---------------------------------------------------------------------------------------------------------------- the certificates
def count_classes(v):
    """how many values of an array fall in each class"""
    v = np.asarray(v, F32)
    a = np.abs(v)
    return {"finite": int(np.isfinite(v).sum()), "+inf": int((v == np.inf).sum()), "-inf": int((v == -np.inf).sum()), "nan": int(np.isnan(v).sum()),
            "subnormal": int(((a > 0) & (a < TINY)).sum()), "-0": int(((v == 0) & np.signbit(v)).sum()), "+0": int(((v == 0) & ~np.signbit(v)).sum())}


def rint_classes(v, scale, zero_point):
    """the classes of t = v * inv that yfc_sim_rint's two bodies could treat differently -> {class: count}"""
    inv = F32(1.0 / np.float64(F32(scale)))
    lo, hi = F32(-128 - zero_point), F32(127 - zero_point)
    with np.errstate(all="ignore"):
        t = (np.asarray(v, F32) * inv).reshape(-1)
        a, fl = np.abs(t), np.floor(np.abs(t))
        tie, even = np.isfinite(t) & (a - fl == 0.5) & (a < 2.0 ** 22), fl % 2 == 0
    out = {}
    for sign, mask in (("+", ~np.signbit(t)), ("-", np.signbit(t))):
        out[f"{sign}tie, even below"] = int((tie & mask & even & (fl > 0)).sum())
        out[f"{sign}tie, odd below"] = int((tie & mask & ~even).sum())
        out[f"{sign}0.5"] = int((mask & (a == 0.5)).sum())
        out[f"{sign}below 0.5"] = int((mask & (a < 0.5) & (a >= TINY)).sum())
        out[f"{sign}subnormal"] = int((mask & (a < TINY) & (a > 0)).sum())
        out[f"{sign}2^23 - 0.5"] = int((mask & (a == 2.0 ** 23 - 0.5)).sum())
        out[f"{sign}2^23"] = int((mask & (a == 2.0 ** 23)).sum())
        out[f"{sign}2^23 + 1"] = int((mask & (a == 2.0 ** 23 + 1)).sum())
        out[f"{sign}2^24"] = int((mask & (a == 2.0 ** 24)).sum())
        out[f"{sign}inf"] = int((mask & np.isinf(t)).sum())
    for name, x in (("lo", lo), ("lo - 0.5", lo - F32(0.5)), ("lo - 1", lo - 1), ("hi", hi), ("hi + 0.5", hi + F32(0.5)), ("hi + 1", hi + 1)):
        out[name] = int((t == x).sum())
    out["nan"] = int(np.isnan(t).sum())
    return out
