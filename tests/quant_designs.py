"""Designed quantisations of the shipped model as .yfm images -- TEST INFRASTRUCTURE (tests/test_quant_designs_host.py, tests/test_quant_designs_gpu.py).

A sibling of tests/requant_models.py.  Where A and W move every number a little, each design here puts one admission bound of the host table
builder (csrc/yf_host_prep.c: build_chan, build_chan_fp32, the add block) into the tables, so that a failure names the bound:
  R1        every channel of conv2d_1 and conv2d_6 (dense, LUT epilogue), conv2d_17 (dense, EPI_ADD), conv2d_53 (the head), conv2d_3 (depthwise,
            stride 1) and conv2d_10 (depthwise, stride 2) at rshift 1
  R20       channels at rshift 20 in the convs with the most taps: conv2d_47 (dense, LUT epilogue), conv2d_34 (dense, EPI_ADD), conv2d_53,
            conv2d_15 (depthwise, stride 1), conv2d_27 (depthwise, stride 2)
  RMIX      R1's convs with the shifts {1, 20, 2, 19} on the four channels of every pass; the last pass of the 18-channel layers (requant2)
            has its two live channels at 1 and 20
  M         multipliers 2^30 + 1 and 2^31 - 1 on channels whose accumulator bound is 2^29 - 1, at shifts 2 and 20 (saturation only; the fp32
            rounding refuses it)
  Z0        output zero point -128 on every conv output, the three add outputs and the head
  Z255      output zero point 127 on eight conv outputs (every kind of epilogue), the three add outputs and the head
  ZIN127, ZINm128  zero points 127 / -128 on the tensors whose halo the device fills: the inputs of PAD #9 and #26 and of the SAME-padded
            depthwise convs (the network input stays at -128: the parser insists)
  ADD       add #18 at rso 20 with s1/s2 = 1/64 and zpo 127; add #35 at the lowest live rso (ADD_LOW_RSO) with s1/s2 = 64 and zpo -128
  LUT       LEAKY_RELU and QUANTIZE tables at s_in/s_out = 1/16 and 16
  SAT       what exists in saturation only: add #41 at rso 1, and the float32 epilogue's own bound -- channels with acc_max * fs one unit under
            2^21 behind output zero points -128 and 127
How a shift is reached.  rshift follows from s_in * s_w / s_out = M * 2^-31 * 2^-rshift.  A targeted channel gets the filter scale that gives
the wanted (M, rshift) on the model's activation scales, and its int8 weights and int32 bias are the shipped ones times old/new filter scale
(the real function stays roughly what it was).  Towards rshift 1 that coarsens the filter to a few units; where every weight would round to 0
the largest one keeps its sign.  Towards rshift 20 the weights saturate at +-127 and the accumulator is the bias: every convolution but
conv2d_1 is 1x1 or depthwise, at most 48 taps, so 255 * sum|w| * 2^-20 is at most 1.5 output steps.  Such a channel is given a byte level of
its own and its bias' is centred (_centre_on_ties) so that the mean accumulator lies on the tie half a step above that level: the input then
decides between two neighbouring bytes through the rounding, which is all a model of this shape can ask of rshift 20, and a tensor's 16
distinct bytes come from the levels differing between its channels.
How a zero point or an activation scale is moved.  _retune divides the filter scales of the convs that read the tensor by the factor its step
was multiplied with, so their multipliers and shifts stay the shipped ones and the design stays about its own bound.
Everything is seeded and deterministic and reads nothing outside the repository; the converter's constraints are re-imposed and the biases
re-derived as tests/requant_models.py does.  design_table() states per design the bound aimed at and what the generator reached;
tests/test_quant_designs_host.py asserts it from the host builder's own tables, and that module's liveness test states what "live" means.
"""
import os

import numpy as np

import requant_models as rm
from oracle.np_restatement import quantize_multiplier

model_file = rm.model_file
CONV, DWCONV, ADD, LEAKY, QUANTIZE = 3, 4, 0, 98, 114
REF, TIES_UP, SINGLE, FP32 = 0, 1, 3, 0x10
ROUNDINGS = (REF, TIES_UP, SINGLE, FP32)
ACC_LIMIT = 1 << 29
ADD_OPS = (18, 35, 41)
HALO_TENSORS = (52, 57, 64, 73, 80, 86, 95)           # inputs of the SAME depthwise convs #3 #15 #32 #38 #49 and of PAD #9 #26
ADD_LOW_RSO = 9                                       # the lowest rso at which add #35 of design ADD meets the liveness conditions (22 distinct bytes; 11 at rso 8)
_CACHE = {}


def _f32(x):
    return np.asarray(x, np.float32)


def _conv_in(m, op):
    """the tensor whose quantisation a convolution's input has: the one before an explicit PAD"""
    ops, t = m["ops"], m["ops"][op]["ins"][0]
    return ops[op - 1]["ins"][0] if op and ops[op - 1]["op"] == rm.PAD and ops[op - 1]["out"] == t else t


def conv_ops(m):
    return [i for i, o in enumerate(m["ops"]) if o["op"] in (CONV, DWCONV)]


def channel_view(m, op):
    """[cout, taps] int64 copy of a conv's weights"""
    o = m["ops"][op]
    wt = m["tensors"][o["ins"][1]]
    w = wt["data"].reshape(wt["shape"]).astype(np.int64)
    return w.reshape(w.shape[0], -1) if o["op"] == CONV else w.reshape(-1, w.shape[3]).T


def _store_channel(m, op, ch, taps):
    o = m["ops"][op]
    wt = m["tensors"][o["ins"][1]]
    w = wt["data"].reshape(wt["shape"])
    if o["op"] == CONV:
        w[ch] = np.asarray(taps, np.int8).reshape(w[ch].shape)
    else:
        w[0, :, :, ch] = np.asarray(taps, np.int8).reshape(w.shape[1], w.shape[2])


def multiplier(m, op, ch):
    """(M, rshift) of a conv channel as QuantizeMultiplier gives them on the model's scales"""
    T, o = m["tensors"], m["ops"][op]
    mq, sh = quantize_multiplier(float(T[_conv_in(m, op)]["scale"][0]) * float(_f32(T[o["ins"][1]]["scale"][ch])) / float(T[o["out"]]["scale"][0]))
    return mq, -sh


def acc_bound(m, op, ch):
    """|bias'| + 255 * sum|w| of a channel, bias' = bias - zp_in * sum(w)"""
    taps = channel_view(m, op)[ch]
    bias = int(m["tensors"][m["ops"][op]["ins"][2]]["data"][ch])
    return abs(bias - m["tensors"][_conv_in(m, op)]["zp"] * int(taps.sum())) + 255 * int(np.abs(taps).sum())


def _solve_filter_scale(s_in, s_out, rs, mq):
    """the float32 filter scale whose QuantizeMultiplier on (s_in, s_out) has shift -rs and the multiplier nearest `mq` inside (2^30, 2^31)"""
    s_w = np.float32(mq / 2.0 ** 31 * 2.0 ** -rs * float(s_out) / float(s_in))
    cand = s_w.view(np.uint32) + np.arange(-4, 5, dtype=np.int64)
    best = None
    for bits in cand:
        c = np.uint32(bits).view(np.float32)
        got, sh = quantize_multiplier(float(s_in) * float(c) / float(s_out))
        if sh == -rs and (1 << 30) < got < (1 << 31) and (best is None or abs(got - mq) < abs(best[1] - mq)):
            best = (c, got)
    assert best is not None, (rs, mq)
    return best[0]


def retarget(m, old, op, ch, rs, mq=3 << 29, byte=None):
    """Channel ch of conv `op` at shift rs and a multiplier near mq, its weights and bias rescaled from the shipped ones (module docstring).
    Where the weights no longer reach four output steps, bias' goes half a step off an output level: the byte `byte`, or the one it was nearest."""
    T, o = m["tensors"], m["ops"][op]
    t_in, wt, bt, to = T[_conv_in(m, op)], T[o["ins"][1]], T[o["ins"][2]], T[o["out"]]
    s_old = np.float32(old["tensors"][o["ins"][1]]["scale"][ch])
    s_new = _solve_filter_scale(t_in["scale"][0], to["scale"][0], rs, mq)
    wt["scale"][ch] = s_new
    g = float(s_old) / float(s_new)
    taps0 = channel_view(old, op)[ch]
    taps = np.clip(np.rint(taps0 * g), -127, 127).astype(np.int64)
    if not taps.any():
        k = int(np.argmax(np.abs(taps0)))
        taps[k] = 1 if taps0[k] >= 0 else -1
    _store_channel(m, op, ch, taps)
    s_in_old = float(old["tensors"][_conv_in(old, op)]["scale"][0])
    bias_real = float(old["tensors"][o["ins"][2]]["data"][ch]) * s_in_old * float(s_old)
    step = float(t_in["scale"][0]) * float(s_new)                                   # the real value of one accumulator unit
    bias2 = int(np.rint(bias_real / step)) - t_in["zp"] * int(taps.sum())          # bias' = bias - zp_in * sum(w) on the new scales
    out_step = float(to["scale"][0]) / step                                         # accumulator units per output step
    if 255 * int(np.abs(taps).sum()) < 4 * out_step:
        level = int(np.clip(np.rint(bias2 / out_step), -100 - to["zp"], 100 - to["zp"])) if byte is None else byte - to["zp"]
        bias2 = int(np.rint((level + 0.5) * out_step))
    lim = ACC_LIMIT - 1 - 255 * int(np.abs(taps).sum())
    bias2 = int(np.clip(bias2, -lim, lim))
    bt["data"][ch] = bias2 + t_in["zp"] * int(taps.sum())
    m.setdefault("_keep", []).append((op, ch))


def _finish(m, old, targeted=()):
    """bias scales follow s_in * s_w; the biases of the channels no design wrote are re-derived for the scales as they stand"""
    T = m["tensors"]
    keep = {(op, ch): int(T[m["ops"][op]["ins"][2]]["data"][ch]) for op, ch in targeted}
    rm._rederive_biases(m, old)
    for (op, ch), b in keep.items():
        T[m["ops"][op]["ins"][2]]["data"][ch] = b
    return model_file.write_yfm(m)


def _constraints(m):
    T = m["tensors"]
    for o in m["ops"]:
        if o["op"] in (rm.PAD, rm.MAXPOOL):
            T[o["out"]]["scale"], T[o["out"]]["zp"] = T[o["ins"][0]]["scale"].copy(), T[o["ins"][0]]["zp"]
    for o in m["ops"]:
        if o["op"] == rm.CONCAT:
            for i in o["ins"][:2]:
                T[i]["scale"], T[i]["zp"] = T[o["out"]]["scale"].copy(), T[o["out"]]["zp"]
    for o in m["ops"]:                                   # a PAD or pool behind a concat input that moved
        if o["op"] in (rm.PAD, rm.MAXPOOL):
            assert T[o["out"]]["zp"] == T[o["ins"][0]]["zp"] and T[o["out"]]["scale"][0] == T[o["ins"][0]]["scale"][0]


def _scale(m, t, factor):
    m["tensors"][t]["scale"] = _f32(m["tensors"][t]["scale"] * np.float32(factor))


class Design:
    """name; bound (what it aims at); targets: {tflite op: channels} whose output tensors the liveness conditions and the dump comparison look at;
    clamp: the design is about a clamp (both ends must be hit); saturation_only; refused_by: the roundings whose admission refuses it"""

    def __init__(self, name, bound, fn, clamp=False, saturation_only=False, refused_by=(), note="", not_live=None):
        self.name, self.bound, self.fn, self.clamp, self.saturation_only, self.refused_by, self.note = name, bound, fn, clamp, saturation_only, tuple(refused_by), note
        self.not_live = dict(not_live or {})             # tflite op -> why its output cannot meet the liveness conditions (arithmetic, not observation)

    def build(self):
        if self.name not in _CACHE:
            old, m = model_file.load_yfm(rm.SHIPPED), model_file.load_yfm(rm.SHIPPED)
            targets = self.fn(m, old)
            _CACHE[self.name] = (_finish(m, old, m.pop("_keep", [])), targets)      # _keep: the (op, channel) whose bias word the design wrote
        return _CACHE[self.name]

    def bytes(self):
        return self.build()[0]

    def targets(self):
        return self.build()[1]

    def model(self):
        return model_file.load_yfm(self.bytes())

    def admitted(self, rounding):
        return rounding not in self.refused_by

    def write(self, directory):
        path = os.path.join(str(directory), f"yoloface_int8_{self.name}.yfm")
        with open(path, "wb") as f:
            f.write(self.bytes())
        return path

    def __repr__(self):
        return self.name


def _cout(m, op):
    return channel_view(m, op).shape[0]


# ---- R1, R20, RMIX ------------------------------------------------------------------------------------------------------------------
def _r_design(shifts, convs, mq=3 << 29):
    def fn(m, old):
        targets = {}
        for op in convs:
            n = _cout(m, op)
            # a design of high shifts alone takes every second pass of a wide layer (the passes between keep the layer's output a function of its
            # input) and always the last pass, the half-filled one of an 18-channel layer
            chs = [c for c in range(n) if min(shifts) < 14 or n <= 18 or (c // 4) % 2 == 0 or c // 4 == (n - 1) // 4]
            for i, c in enumerate(chs):
                retarget(m, old, op, c, shifts[c % 4 % len(shifts)], mq, byte=-110 + (220 * i) // max(len(chs) - 1, 1))
            targets[op] = chs
        for op in sorted(convs):                         # in graph order: a conv is centred on the inputs the finished convs before it give it
            _centre_on_ties(m, op, [c for c in targets[op] if multiplier(m, op, c)[1] >= 14])
        return targets
    return fn


def _centre_on_ties(m, op, chs):
    """The channels `chs` of conv `op` sit at a high shift: their weights move the output by a fraction of a step, so whether the input decides anything
    depends on where bias' lies.  Measure the mean of sum w (x - zp_in) per channel -- the oracle on the six golden frames, the channel set for the
    measurement to bias' = 0 and a multiplier under which 255 * sum|w| is 60 output steps -- and move bias' so that the mean accumulator lies on the tie
    half a step above the channel's level."""
    if not chs:
        return
    import tempfile
    from oracle.oracle import Oracle
    T, o = m["tensors"], m["ops"][op]
    t_in, wt, bt, to = T[_conv_in(m, op)], T[o["ins"][1]], T[o["ins"][2]], T[o["out"]]
    final = {c: (np.float32(wt["scale"][c]), int(bt["data"][c])) for c in chs}
    probe = {}
    for c in chs:
        taps = channel_view(m, op)[c]
        ratio = 60.0 / (255.0 * int(np.abs(taps).sum()))
        rs = int(np.floor(-np.log2(ratio)))                                          # ratio = f * 2^-rs, f in [0.5, 1)
        wt["scale"][c] = _solve_filter_scale(t_in["scale"][0], to["scale"][0], rs, int(ratio * 2.0 ** rs * 2.0 ** 31))
        bt["data"][c] = t_in["zp"] * int(taps.sum())                                 # bias' = 0
        mq, rs = multiplier(m, op, c)
        probe[c] = mq / 2.0 ** 31 * 2.0 ** -rs
    image = model_file.write_yfm(_with_bias_scales(m))
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "probe.yfm")
        with open(path, "wb") as f:
            f.write(image)
        x = np.fromfile(os.path.join(rm.ROOT, "tests", "golden", "golden_inputs.bin"), np.int8).reshape(-1, 56, 56, 3)
        dump = Oracle(path).run(x, dump=True, threads=4)[1]
    shapes = [tuple(T[q["out"]]["shape"][1:]) for q in m["ops"]]
    off = int(sum(int(np.prod(s)) for s in shapes[:op]))
    y = dump[:, off:off + int(np.prod(shapes[op]))].reshape((-1,) + shapes[op]).astype(np.float64) - to["zp"]
    for c in chs:
        s_w, bias = final[c]
        wt["scale"][c] = s_w
        bt["data"][c] = bias - int(np.rint(y[..., c].mean() / probe[c]))


def _with_bias_scales(m):
    """m with every bias tensor's scales set to s_in * s_w as the parser and the oracle's loader expect (the bias words untouched)"""
    T = m["tensors"]
    for i in conv_ops(m):
        tw, tb = m["ops"][i]["ins"][1:3]
        T[tb]["scale"] = _f32(_f32(T[_conv_in(m, i)]["scale"][0]) * _f32(T[tw]["scale"]))
    return m


# ---- M ------------------------------------------------------------------------------------------------------------------------------
M_LO, M_HI = (1 << 30) + 1, (1 << 31) - 1
# conv -> (the end its channels 0..3 aim at, output zero point).  One end per conv: the filter scales just above and just below a power of two are
# neighbours, so M - 2^30 of the one and (2^31 - M) / 2 of the other add up to the 64..128 that one float32 step of a filter scale moves M by,
# whatever the output scale: both ends cannot be near on one tensor.  Dense convs, depthwise convs and the head.
M_CONVS = {47: (M_LO, -128), 51: (M_HI, 127), 15: (M_LO, 127), 38: (M_HI, -128), 53: (M_HI, -128), 42: (M_LO, 127)}
M_PLAN = [(20, 1), (20, -1), (2, 1), (2, -1)]          # (rshift, sign of bias') of channels 0..3


def _solve_end(s_in, s_out, rs, mq):
    """(s_w, M): the float32 filter scale whose multiplier comes nearest to an END of (2^30, 2^31) from inside, at shift -rs"""
    centre = np.float32(mq / 2.0 ** 31 * 2.0 ** -rs * float(s_out) / float(s_in)).view(np.uint32)
    best = None
    for bits in centre + np.arange(-2, 3, dtype=np.int64):
        c = np.uint32(bits).view(np.float32)
        got, sh = quantize_multiplier(float(s_in) * float(c) / float(s_out))
        if sh == -rs and (1 << 30) < got < (1 << 31) and (best is None or abs(got - mq) < abs(best[1] - mq)):
            best = (c, got)
    assert best is not None
    return best


def _search_out_scale(s_in, s_out, mq, window=1 << 15):
    """the float32 neighbour of s_out (within `window` steps) at which the channels of M_PLAN, each on its best filter scale, miss `mq` by the least;
    the same arithmetic as _solve_end, on arrays"""
    outs = (np.float32(s_out).view(np.uint32).astype(np.int64) + np.arange(-window, window + 1)).astype(np.uint32).view(np.float32).astype(np.float64)
    total = np.zeros(outs.shape)
    for rs, _ in M_PLAN:
        centre = (mq / 2.0 ** 31 * 2.0 ** -rs * outs / float(s_in)).astype(np.float32).view(np.uint32).astype(np.int64)
        miss = np.full(outs.shape, np.inf)
        for d in range(-2, 3):
            c = (centre + d).astype(np.uint32).view(np.float32).astype(np.float64)
            got = np.rint(float(s_in) * c / outs * 2.0 ** (31 + rs))
            miss = np.where((got > 2.0 ** 30) & (got < 2.0 ** 31), np.minimum(miss, np.abs(got - mq)), miss)
        total += miss
    return outs[int(np.argmin(total))].astype(np.float32)


def _m_design(m, old):
    T, targets = m["tensors"], {}
    for op, (mq, zp) in M_CONVS.items():
        o = m["ops"][op]
        t_in, to = T[_conv_in(m, op)], T[o["out"]]
        to["zp"] = zp
        _retune(m, o["out"], float(_search_out_scale(t_in["scale"][0], to["scale"][0], mq)) / float(to["scale"][0]))
        for ch, (rs, sign) in enumerate(M_PLAN):
            T[o["ins"][1]]["scale"][ch] = _solve_end(t_in["scale"][0], to["scale"][0], rs, mq)[0]
            taps = channel_view(m, op)[ch]
            bias2 = sign * (ACC_LIMIT - 1 - 255 * int(np.abs(taps).sum()))
            T[o["ins"][2]]["data"][ch] = bias2 + t_in["zp"] * int(taps.sum())
            m.setdefault("_keep", []).append((op, ch))
        targets[op] = list(range(len(M_PLAN)))
    return targets


# ---- Z0, Z255, ZIN --------------------------------------------------------------------------------------------------------------------
def _producer(m, t):
    return next(i for i, o in enumerate(m["ops"]) if o["out"] == t)


def _consumer_convs(m, t):
    """the convolutions that read tensor t, directly or through an explicit PAD"""
    return [i for i, o in enumerate(m["ops"]) if o["op"] in (CONV, DWCONV) and _conv_in(m, i) == t]


def _retune(m, t, factor, zp=None):
    """tensor t's step times `factor` (and its zero point), the filter scales of the convs that read it divided by it: their multipliers and
    shifts stay what they were, and _finish re-derives their biases for the same real function"""
    _scale(m, t, factor)
    if zp is not None:
        m["tensors"][t]["zp"] = zp
    for op in _consumer_convs(m, t):
        w = m["tensors"][m["ops"][op]["ins"][1]]
        w["scale"] = _f32(w["scale"] / np.float32(factor))


def _z0_design(m, old):
    """zp_out = -128 on every conv and add output, at half the step: the real range is [0, 255 s], the negative side clamps"""
    T, targets = m["tensors"], {}
    for i, o in enumerate(m["ops"]):
        if o["op"] in (CONV, DWCONV, ADD):
            T[o["out"]]["zp"] = -128
            _scale(m, o["out"], 0.5)
            targets[i] = list(range(T[o["out"]]["shape"][3]))
    return targets


Z255_CONVS = (1, 3, 5, 10, 17, 34, 40, 53)             # conv2d_1, depthwise at stride 1 and 2, dense -> dense, the three dense -> add, the head


def _z255_design(m, old):
    """zp_out = 127 on the listed conv outputs and the three add outputs.  Only values <= 0 are representable then, so each conv's biases move its
    output down by the zero point's move (its bytes stay roughly the shipped ones under another zero point); a LEAKY_RELU behind it sees negative
    values only and its output is re-quantised for them (a fifth of the step, zero point 100)."""
    T, ops, targets, keep = m["tensors"], m["ops"], {}, []
    for op in Z255_CONVS:
        to = T[ops[op]["out"]]
        for ch in range(_cout(m, op)):
            mq, rs = multiplier(m, op, ch)
            T[ops[op]["ins"][2]]["data"][ch] -= int(np.rint((127 - to["zp"]) / (mq / 2.0 ** 31 * 2.0 ** -rs)))
            keep.append((op, ch))
        to["zp"] = 127
        targets[op] = list(range(_cout(m, op)))
        nxt = [i for i, o in enumerate(ops) if o["op"] == LEAKY and o["ins"][0] == ops[op]["out"]]
        for i in nxt:
            _retune(m, ops[i]["out"], 0.2, 100)
    for op in ADD_OPS:
        T[ops[op]["out"]]["zp"] = 127
        targets[op] = list(range(T[ops[op]["out"]]["shape"][3]))
    _constraints(m)
    m.setdefault("_keep", []).extend(keep)
    return targets


def _zin_design(zp):
    def fn(m, old):
        T, targets = m["tensors"], {}
        for t in HALO_TENSORS:
            # zero point 127: only values <= 0 are representable, so the step is an eighth (LeakyReLU's negative side in 200 levels) and the
            # convs behind keep their multipliers
            _retune(m, t, 0.125 if zp == 127 else 1.0, zp)
            targets[_producer(m, t)] = list(range(T[t]["shape"][3]))
        _constraints(m)
        return targets
    return fn


# ---- ADD ----------------------------------------------------------------------------------------------------------------------------
def _set_add_out(m, op, rso, zpo, mo=3 << 29):
    """the add's output scale for (mo, rso): twice_max / (2^20 * so) = mo * 2^-31 * 2^-rso; the convs behind keep their multipliers"""
    T, o = m["tensors"], m["ops"][op]
    twice = float(np.float32(2) * max(np.float32(T[o["ins"][0]]["scale"][0]), np.float32(T[o["ins"][1]]["scale"][0])))
    so = np.float32(twice / 2.0 ** 20 / (mo / 2.0 ** 31 * 2.0 ** -rso))
    for bits in so.view(np.uint32) + np.array([0, 1, -1, 2, -2], np.int64):
        c = np.uint32(bits).view(np.float32)
        got, sh = quantize_multiplier(twice / float(np.float32(1 << 20) * c))
        if sh == -rso and got > (1 << 30):
            _retune(m, o["out"], float(c) / float(T[o["out"]]["scale"][0]), zpo)
            T[o["out"]]["scale"] = _f32([c])
            return
    raise AssertionError((op, rso))


def _tie_input(m, t, scale):
    """an add input's scale set to `scale` with its bytes left as they are: the producing conv's filter scales (and so its real function) move along,
    its bias words stay; the other convs that read it keep their multipliers"""
    f = float(scale) / float(m["tensors"][t]["scale"][0])
    _retune(m, t, f)
    m["tensors"][t]["scale"] = _f32([np.float32(scale)])
    p = _producer(m, t)
    if m["ops"][p]["op"] in (CONV, DWCONV):
        w = m["tensors"][m["ops"][p]["ins"][1]]
        w["scale"] = _f32(w["scale"] * np.float32(f))
        m.setdefault("_keep", []).extend((p, ch) for ch in range(_cout(m, p)))


def _add_design(m, old):
    T = m["tensors"]
    _tie_input(m, 67, np.float32(T[62]["scale"][0]) * np.float32(64))      # add #18: s1/s2 = 1/64 exactly (a power of two is one float32 operation)
    _set_add_out(m, 18, 20, 127)
    _tie_input(m, 83, np.float32(T[78]["scale"][0]) / np.float32(64))      # add #35: s1/s2 = 64
    _set_add_out(m, 35, ADD_LOW_RSO, -128)
    return {18: list(range(6)), 35: list(range(8))}


# ---- SAT: the bounds that exist in saturation only ---------------------------------------------------------------------------------------
FZ_CONVS = {5: -128, 15: 127, 12: -128, 38: 127}        # convs whose channels have a float32 bound of their own (tests/test_model_variants_host.py), -> zp_out


def fp32_scale(m, op, ch):
    T, o = m["tensors"], m["ops"][op]
    return np.float32(np.float32(np.float32(T[_conv_in(m, op)]["scale"][0]) * np.float32(T[o["ins"][1]]["scale"][ch])) / np.float32(T[o["out"]]["scale"][0]))


def fp32_acc_bound(m, op, ch):
    """the largest accumulator bound build_chan_fp32 admits for the channel: (double)acc_max * (double)fs < 2^21, and below 2^29"""
    fs = float(fp32_scale(m, op, ch))
    a = int(2097152.0 / fs)
    while float(a) * fs >= 2097152.0:
        a -= 1
    while float(a + 1) * fs < 2097152.0:
        a += 1
    return min(a, ACC_LIMIT - 1)


def _sat_design(m, old):
    """add #41 at rso 1 (one output step is 2^-18 of its inputs' steps: every sum but 0 saturates), and the float32 epilogue's own bound: two channels each
    of four convs with acc_max * fs one accumulator unit under 2^21, behind output zero points -128 and 127"""
    T, targets = m["tensors"], {}
    _set_add_out(m, 41, 1, T[90]["zp"])
    targets[41] = list(range(8))
    for op, zp in FZ_CONVS.items():
        T[m["ops"][op]["out"]]["zp"] = zp
    for op in FZ_CONVS:
        t_in = T[_conv_in(m, op)]
        for ch, sign in ((0, 1), (1, -1)):
            taps = channel_view(m, op)[ch]
            bias2 = sign * (fp32_acc_bound(m, op, ch) - 255 * int(np.abs(taps).sum()))
            T[m["ops"][op]["ins"][2]]["data"][ch] = bias2 + t_in["zp"] * int(taps.sum())
            m.setdefault("_keep", []).append((op, ch))
        targets[op] = [0, 1]
    return targets


# ---- LUT ----------------------------------------------------------------------------------------------------------------------------
LUT_LEAKY_16TH = (4, 16, 28, 39, 52)                   # LEAKY_RELU ops at s_in/s_out = 1/16
LUT_LEAKY_16 = (2, 11, 14, 24, 33, 37, 48, 50)         # ... at 16
LUT_QUANTIZE = {21: 16, 45: 1 / 16, 44: 16}


def _lut_design(m, old):
    T, ops = m["tensors"], m["ops"]

    def tie(t_out, t_in, ratio):                         # s_out = s_in / ratio: one float32 operation on a power of two; the convs behind keep their multipliers
        _retune(m, t_out, float(np.float32(T[t_in]["scale"][0]) / np.float32(ratio)) / float(T[t_out]["scale"][0]))
        T[t_out]["scale"] = _f32([np.float32(T[t_in]["scale"][0]) / np.float32(ratio)])
    for op in LUT_LEAKY_16TH:
        tie(ops[op]["out"], ops[op]["ins"][0], 1 / 16)
    for op in LUT_LEAKY_16:
        tie(ops[op]["out"], ops[op]["ins"][0], 16)
    tie(71, 57, 16)                                      # QUANTIZE #21: tensor 58 (= 57, pool) -> 103 (= 71, concat)
    tie(93, 73, 1 / 16)                                  # QUANTIZE #45: tensor 74 (= 73, pool) -> 101 (= 93)
    tie(92, 93, 1 / 16)                                  # QUANTIZE #44: tensor 92 -> 102 (= 93): s92 = 16 * s93
    _constraints(m)
    return {op: list(range(T[ops[op]["out"]]["shape"][3])) for op in LUT_LEAKY_16TH + LUT_LEAKY_16 + tuple(LUT_QUANTIZE)}


R_CONVS = (1, 3, 6, 10, 17, 53)                        # R1 and RMIX: conv2d_1 and a 1x1 (LUT epilogue), a dense -> add, the head, depthwise at stride 1 and 2
R20_CONVS = (47, 15, 27, 34, 53)                       # R20: the widest filters (a shift of 20 leaves 255 * sum|w| under 1.5 output steps even at 48 taps)
LUT_CAP = "a table at s_in/s_out = 1/16 or of a QUANTIZE at 16 has at most 256 / 16 + 2 = 18 output levels"
DESIGNS = [
    Design("R1", "conv rshift = 1", _r_design([1], R_CONVS)),
    Design("R20", "conv rshift = 20", _r_design([20], R20_CONVS, mq=(1 << 31) - (1 << 24))),
    Design("RMIX", "rshift {1, 20, 2, 19} inside one pass", _r_design([1, 20, 2, 19], R_CONVS)),
    Design("M", "mq = 2^30 + 1 and 2^31 - 1 with acc_max = 2^29 - 1, at rshift 2 and 20", _m_design, clamp=True, saturation_only=True, refused_by=(FP32,),
           note="not live: an accumulator within 1 % of 2^29 leaves the output 2^29 * 2^-20 / 100 <= 5 steps to move in at rshift 20 and saturates at lower shifts; "
                "YF_ROUND_FP32 refuses it (acc_max * fs >= 2^21 at rshift 2) and has no multiplier"),
    Design("Z0", "zp_out = -128 (Z = 0) on every conv output, the add outputs and the head", _z0_design),
    Design("Z255", "zp_out = 127 (Z = 255) on conv outputs, the add outputs and the head", _z255_design),
    Design("ZIN127", "zp_in = 127 on the tensors with device-filled halos", _zin_design(127)),
    Design("ZINm128", "zp_in = -128 on the tensors with device-filled halos", _zin_design(-128)),
    Design("ADD", f"add rso = 20 and rso = {ADD_LOW_RSO}, s1/s2 = 1/64 and 64, zpo = 127 and -128", _add_design),
    Design("LUT", "LEAKY_RELU and QUANTIZE at s_in/s_out = 1/16 and 16", _lut_design, not_live={op: LUT_CAP for op in LUT_LEAKY_16TH + tuple(LUT_QUANTIZE)}),
    Design("SAT", "add rso = 1; acc_max * fs just under 2^21 at Z = 0 and Z = 255", _sat_design, clamp=True, saturation_only=True,
           note="rso = 1 exists only in saturation (one output step is 2^-18 of an input step), and so does acc * fs near 2^21"),
]
BY_NAME = {d.name: d for d in DESIGNS}
NAMES = tuple(BY_NAME)


def build(name):
    return BY_NAME[name].bytes()


# ---- the exported table ----------------------------------------------------------------------------------------------------------------
def reached(design):
    """what the generator reached, from the design's own bytes: the shift histogram, the multiplier range and max acc_max / 2^29 of the targeted conv
    channels, the Z = zp_out + 128 of the targeted tensors, the adds' rso"""
    m = design.model()
    T, ops = m["tensors"], m["ops"]
    hist, mqs, acc, zs = {}, [], 0.0, set()
    for op, chs in design.targets().items():
        zs.add(T[ops[op]["out"]]["zp"] + 128)
        if ops[op]["op"] in (CONV, DWCONV):
            for ch in chs:
                mq, rs = multiplier(m, op, ch)
                hist[rs] = hist.get(rs, 0) + 1
                mqs.append(mq)
                acc = max(acc, acc_bound(m, op, ch) / ACC_LIMIT)
    rso = []
    for op in ADD_OPS:
        o = ops[op]
        twice = float(np.float32(2) * max(np.float32(T[o["ins"][0]]["scale"][0]), np.float32(T[o["ins"][1]]["scale"][0])))
        rso.append(-quantize_multiplier(twice / float(np.float32(1 << 20) * np.float32(T[o["out"]]["scale"][0])))[1])
    return dict(shifts=dict(sorted(hist.items())), mq=(min(mqs), max(mqs)) if mqs else None, acc=acc, Z=sorted(zs), rso=rso,
                zp_in=sorted({T[t]["zp"] for t in HALO_TENSORS}))


def design_table():
    """per design: name, bound aimed at, what was reached, the roundings that refuse it, a note where a bound could not be made live"""
    return [dict(name=d.name, bound=d.bound, reached=reached(d), refused_by=[hex(r) for r in d.refused_by], saturation_only=d.saturation_only,
                 not_live=sorted(d.not_live), note=d.note or "; ".join(sorted(set(d.not_live.values())))) for d in DESIGNS]


# ---- admission edges: one step inside and one step outside each rule of build_chan, build_chan_fp32 and the add block -------------------------
INTEGER = (REF, TIES_UP, SINGLE)


def _image(fn):
    old, m = model_file.load_yfm(rm.SHIPPED), model_file.load_yfm(rm.SHIPPED)
    fn(m, old)
    return _finish(m, old, m.pop("_keep", []))


def _edge_shift(rs):
    def fn(m, old):
        for op, ch in ((5, 2), (15, 17), (53, 17)):      # a dense conv, a depthwise one, the head's half-filled last pass
            retarget(m, old, op, ch, rs)
    return fn


def _edge_pow2(exact):
    def fn(m, old):
        T = m["tensors"]
        T[54]["scale"], T[55]["scale"] = _f32([2.0 ** -4]), _f32([2.0 ** -3])          # conv2d_5: s_in * s_w / s_out = 2^-9 exactly = 2^30 * 2^-31 * 2^-8
        w = T[m["ops"][5]["ins"][1]]["scale"]
        w[2] = np.float32(2.0 ** -8) if exact else np.nextafter(np.float32(2.0 ** -8), np.float32(1))
    return fn


def _edge_bias(design, op, ch, step):
    """design's image with channel ch of conv `op` one accumulator unit further out (step 1) or as it is (step 0)"""
    m = BY_NAME[design].model()
    b = m["tensors"][m["ops"][op]["ins"][2]]["data"]
    bias2 = int(b[ch]) - m["tensors"][_conv_in(m, op)]["zp"] * int(channel_view(m, op)[ch].sum())
    b[ch] += step * (1 if bias2 > 0 else -1)
    return model_file.write_yfm(m)


def _edge_rso(op, rso):
    def fn(m, old):
        _set_add_out(m, op, rso, m["tensors"][m["ops"][op]["out"]]["zp"])
    return fn


def admission_edges():
    """[(rule, image inside, image outside, the roundings that refuse the one outside, the roundings that admit the one inside)]"""
    every = INTEGER + (FP32,)
    return [
        ("rshift 1 | 0", _image(_edge_shift(1)), _image(_edge_shift(0)), INTEGER, every),
        ("rshift 20 | 21", _image(_edge_shift(20)), _image(_edge_shift(21)), INTEGER, every),
        ("mq 2^30 + 128 | 2^30", _image(_edge_pow2(False)), _image(_edge_pow2(True)), INTEGER, every),
        ("acc_max 2^29 - 1 | 2^29", _edge_bias("M", 47, 0, 0), _edge_bias("M", 47, 0, 1), every, INTEGER),
        ("acc_max 2^29 - 1 | 2^29, depthwise, bias' < 0", _edge_bias("M", 15, 1, 0), _edge_bias("M", 15, 1, 1), every, INTEGER),
        ("add rso 20 | 21", _image(_edge_rso(18, 20)), _image(_edge_rso(18, 21)), every, every),
        ("add rso 1 | so = 0", _image(_edge_rso(41, 1)), _image(_edge_rso(41, 0)), every, every),
        ("acc_max * fs < 2^21 | >= 2^21", _edge_bias("SAT", 5, 0, 0), _edge_bias("SAT", 5, 0, 1), (FP32,), every),
        ("acc_max * fs < 2^21 | >= 2^21, depthwise, bias' < 0", _edge_bias("SAT", 38, 1, 0), _edge_bias("SAT", 38, 1, 1), (FP32,), every),
    ]


# ---- liveness, and the record (profiles/quant_designs.txt) ---------------------------------------------------------------------------------
def frames_56():
    """the 56x56 frames of the GPU modules (tests/test_model_file_gpu.py, frames): the golden six, the real ones and noise, 67 in all"""
    golden = os.path.join(rm.ROOT, "tests", "golden")
    real = np.fromfile(os.path.join(golden, "real_frames_56.bin"), np.int8).reshape(-1, 56, 56, 3)
    gold = np.fromfile(os.path.join(golden, "golden_inputs.bin"), np.int8).reshape(-1, 56, 56, 3)
    return np.concatenate([gold, real, np.random.default_rng(67).integers(-128, 128, (67 - 6 - real.shape[0], 56, 56, 3), dtype=np.int8)])


def liveness(design, orc, x):
    """per targeted tflite op: (distinct byte values, share at -128, share at 127) of the oracle's dump restricted to the targeted channels"""
    T = design.model()["tensors"]
    shapes = [tuple(T[o["out"]]["shape"][1:]) for o in design.model()["ops"]]
    sizes = [int(np.prod(s)) for s in shapes]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    dump = orc.run(x, dump=True, threads=8)[1]
    out = {}
    for op, chs in design.targets().items():
        v = dump[:, offs[op]:offs[op] + sizes[op]].reshape((-1,) + shapes[op])[..., chs]
        out[op] = (int(np.unique(v).size), float(np.mean(v == -128)), float(np.mean(v == 127)))
    return out


def report():
    """the text of profiles/quant_designs.txt up to its hand-written notes: python tests/quant_designs.py"""
    import tempfile
    from oracle.oracle import Oracle
    lines, x = [], frames_56()
    with tempfile.TemporaryDirectory() as d:
        shipped = Oracle().run(x, threads=8)
        for row, design in zip(design_table(), DESIGNS):
            r = row["reached"]
            lines.append(f"{row['name']:8s} aims at: {row['bound']}")
            lines.append(f"         reached: shifts of the targeted channels {r['shifts'] or '-'}; M {r['mq'] or '-'}; max acc_max / 2^29 {r['acc']:.6f}; "
                         f"Z of the targeted tensors {r['Z']}; rso {r['rso']}; halo zero points {r['zp_in']}")
            lines.append(f"         refused by: {', '.join(row['refused_by']) or 'no rounding'}; saturation only: {'yes' if row['saturation_only'] else 'no'}"
                         + (f"; note: {row['note']}" if row["note"] else ""))
            orc = Oracle(design.write(d))
            lines.append(f"         heads: {int((orc.run(x, threads=8) != shipped).sum())} of {shipped.size} bytes differ from the shipped model's on the 67 frames")
            for op, (distinct, lo, hi) in liveness(design, orc, x).items():
                lines.append(f"         tflite op {op:2d}, {len(design.targets()[op]):2d} channels: {distinct:3d} distinct bytes, {100 * lo:5.1f} % at -128, {100 * hi:5.1f} % at 127"
                             + ("   (not live: see the note)" if op in design.not_live else ""))
    return "\n".join(lines)


if __name__ == "__main__":
    print(report())
