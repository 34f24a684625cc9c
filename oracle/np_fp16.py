"""fp16-faithful evaluation of the yoloface graph in numpy -- TEST INFRASTRUCTURE, next to np_fp32.py (same graph, same weight packs).

It states what the fused fp16 kernel (stm32h7-yolo_amd/csrc/yf_fp16.hip) computes when every accumulator is exact: on the designed weight packs of
tests/fp16_packs.py the kernel has one right answer and this module gives it bit for bit; on real weights it differs from the kernel only by the
order in which a float32 accumulator meets its terms.  Differences from np_fp32.py:

  * weights are rounded to fp16 (yf_fp16_create: `(half_t)wf[...]`, a C cast = round to nearest even; yf_fp16.hip:1114-1115, 1126); biases stay
    float32 (memcpy, :1131) and are the accumulator's initial value (:278, :352, :440, :507, :733, :772)
  * an accumulator is the float64 sum of the exact fp16 x fp16 products and the float32 bias, rounded ONCE to float32 (accumulate="f64"); the modes
    "f32_forward" / "f32_reverse" add the terms one by one in float32, first to last / last to first, to measure what order can do
  * LeakyReLU is max(x, float32(0.1) * x) in float32 (leaky_pack2, :192-199: v_pk_mul_f32 by 0.1f, v_max_f32)
  * float32 -> fp16 is round to nearest even (pack2, :184-187: v_cvt_pk_f16_f32; numpy's astype(float16) is the same rounding), at
      - every stage output: the 3x3 stages (:451, :500), the dense stages (:287-288), the tail's register chain (:755-756, :782)
      - the 4-channel intermediate of the fused pair conv2d_5 -> conv2d_6: `mid`, :360 (linear, no activation)
      - the residual adds: the STORED fp16 operand is widened and added to the float32 accumulator -- one more float32 addition -- and the sum is
        rounded to fp16 once (:281-285 conv2d_17; :751-754 conv2d_34 and conv2d_40, operands t18 / t22 in registers as packed fp16)
      - the register-resident 7x7 tail: every layer's packed outputs are the next layer's B operand (:755-756), the depthwise ones go through
        the exchange buffer as fp16 (:767, :782)
  * max-pools run on fp16 values (pkmaxh = v_pk_max_f16, :578-582; clamped windows, the padding takes no part): exact, no rounding
  * the head (conv2d_53) leaves the accumulator as float32, no fp16 rounding (EPI_HEAD, :745-749)
  * the input frame is fp16 already (the caller's cast)

`hook` lets a test state a deliberately WRONG evaluation without copying this file: a dict {(name, layer): value or function of the default}, see
_h() and the names used below ("taps", "pad", "weights", "bias", "slope", "pool", "concat", "residual_pre").
"""
import numpy as np

from oracle.np_fp32 import load_yfw  # noqa: F401  (the same pack reader)

# depthwise, cin, cout, k, stride, LeakyReLU behind it, output width
LAYERS = [(0, 3, 8, 3, 2, 1, 28), (1, 8, 8, 3, 1, 1, 28), (0, 8, 4, 1, 1, 0, 28), (0, 4, 18, 1, 1, 1, 28), (1, 18, 18, 3, 2, 1, 14), (0, 18, 6, 1, 1, 0, 14),
          (0, 6, 36, 1, 1, 1, 14), (1, 36, 36, 3, 1, 1, 14), (0, 36, 6, 1, 1, 0, 14), (0, 6, 18, 1, 1, 1, 14), (0, 36, 24, 1, 1, 1, 14), (1, 24, 24, 3, 2, 1, 7),
          (0, 24, 8, 1, 1, 0, 7), (0, 8, 40, 1, 1, 1, 7), (1, 40, 40, 3, 1, 1, 7), (0, 40, 8, 1, 1, 0, 7), (0, 8, 40, 1, 1, 1, 7), (1, 40, 40, 3, 1, 1, 7),
          (0, 40, 8, 1, 1, 0, 7), (0, 8, 24, 1, 1, 1, 7), (0, 48, 40, 1, 1, 1, 7), (1, 40, 40, 3, 1, 1, 7), (0, 40, 32, 1, 1, 1, 7), (0, 32, 18, 1, 1, 0, 7)]
POOLS = [(8, 3), (4, 1)]            # pool_8 (28 -> 14), pool_25 (14 -> 7): kernel, padding; stride 2


def walk(ops, x):
    """The graph, once: ops.conv(layer, x, res=None, res_layer=None), ops.pool(which, x), ops.concat(layer, pooled, x)."""
    c = ops.conv
    x = c(0, x); x = c(1, x); x = c(2, x); t4 = c(3, x)
    x = c(4, t4); t7 = c(5, x); x = c(6, t7); x = c(7, x); x = c(8, x, res=t7, res_layer=5); x = c(9, x)
    t15 = c(10, ops.concat(10, ops.pool(0, t4), x))
    x = c(11, t15); t18 = c(12, x); x = c(13, t18); x = c(14, x); t22 = c(15, x, res=t18, res_layer=12)
    x = c(16, t22); x = c(17, x); x = c(18, x, res=t22, res_layer=15); x = c(19, x)
    x = c(20, ops.concat(20, ops.pool(1, t15), x)); x = c(21, x); x = c(22, x)
    return c(23, x)


def _h(hook, name, layer, default):
    f = hook.get((name, layer)) if hook else None
    return default if f is None else (f(default) if callable(f) else f)


def conv_terms(i, x16, conv, hook=None):
    """The exact products of conv `i` on x16 [N,H,W,Cin] (fp16): float64 [N,OH,OW,Cout,T] (T: taps row-major, input channels fastest), and the float32 bias."""
    w, b = _h(hook, "weights", i, (conv["w"], conv["b"]))
    w = np.asarray(w, np.float32).astype(np.float16).astype(np.float64)
    b = _h(hook, "bias", i, np.asarray(b, np.float32))
    x = x16.astype(np.float64)
    n, h, wd, cin = x.shape
    if conv["k"] == 1:
        return x[:, :, :, None, :] * w.reshape(conv["cout"], cin), b
    s = conv["stride"]
    oh, ow = (h + 2 - 3) // s + 1, (wd + 2 - 3) // s + 1
    py, px = _h(hook, "pad", i, (1, 1))                      # zero rows above / columns left of the data (the graph: 1 and 1)
    xp = np.zeros((n, h + 4, wd + 4, cin))
    xp[:, py:py + h, px:px + wd] = x
    patches = [xp[:, ky:ky + (oh - 1) * s + 1:s, kx:kx + (ow - 1) * s + 1:s] for ky in range(3) for kx in range(3)]
    patches = _h(hook, "taps", i, patches)
    if conv["dw"]:
        return np.stack([p * w[t // 3, t % 3] for t, p in enumerate(patches)], axis=-1), b
    return np.concatenate([p[:, :, :, None, :] * w[:, t // 3, t % 3, :] for t, p in enumerate(patches)], axis=-1), b


def accumulate_terms(terms, bias, mode):
    if mode == "f64":
        return (terms.sum(axis=-1) + bias.astype(np.float64)).astype(np.float32)
    order = range(terms.shape[-1]) if mode == "f32_forward" else range(terms.shape[-1] - 1, -1, -1)
    assert mode in ("f32_forward", "f32_reverse"), mode
    acc = np.broadcast_to(bias.astype(np.float32), terms.shape[:-1]).copy()
    for t in order:
        acc += terms[..., t].astype(np.float32)             # a product of two fp16 values is exact in float32
    return acc


class _Ops:
    def __init__(self, convs, accumulate, hook, on_acc):
        self.convs, self.mode, self.hook, self.on_acc = convs, accumulate, hook, on_acc
        self.pre32, self.out = {}, {}

    def conv(self, i, x, res=None, res_layer=None):
        self.out[("in", i)] = x
        terms, bias = conv_terms(i, x, self.convs[i], self.hook)
        acc = accumulate_terms(terms, bias, self.mode)
        r32 = None
        if res is not None:
            r32 = self.pre32[res_layer] if _h(self.hook, "residual_pre", i, False) else res.astype(np.float32)
            acc = acc + r32                                   # float32 + float32
        if self.on_acc is not None:
            self.on_acc(i, terms, bias, None if res is None else res.astype(np.float64))
        if LAYERS[i][5]:
            acc = np.maximum(acc, np.float32(_h(self.hook, "slope", i, 0.1)) * acc)
        self.pre32[i] = acc
        y = acc if i == 23 else acc.astype(np.float16)
        self.out[i] = y
        return y

    def pool(self, which, x):
        k, pad = POOLS[which]
        k, pad, zero_pad = _h(self.hook, "pool", which, (k, pad, False))
        n, h, w, c = x.shape
        oh, ow = h // 2, w // 2
        y = np.empty((n, oh, ow, c), x.dtype)
        for oy in range(oh):
            for ox in range(ow):
                y0, x0 = 2 * oy - pad, 2 * ox - pad
                win = x[:, max(y0, 0):min(y0 + k, h), max(x0, 0):min(x0 + k, w)].reshape(n, -1, c).max(axis=1)
                if zero_pad and (y0 < 0 or x0 < 0 or y0 + k > h or x0 + k > w):
                    win = np.maximum(win, x.dtype.type(0))
                y[:, oy, ox] = win
        self.out["pool%d" % which] = y
        return y

    def concat(self, layer, pooled, x):
        cat = np.concatenate([pooled, x], axis=-1)
        return _h(self.hook, "concat", layer, cat)


def run_fp16(convs, frame_f16, accumulate="f64", intermediates=False, hook=None, on_acc=None):
    """frame(s) fp16 [56,56,3] or [N,56,56,3] -> logits float32 [7,7,18] or [N,7,7,18]; with intermediates=True also a dict {layer index | 'pool0' |
    'pool1': tensor, ('in', layer index): the tensor that conv reads}.  on_acc(layer, terms, bias, residual) sees every accumulator's exact terms (the exactness certificate of tests/fp16_packs.py)."""
    x = np.asarray(frame_f16)
    assert x.dtype == np.float16, "the kernel takes fp16 frames: cast first"
    single = x.ndim == 3
    ops = _Ops(convs, accumulate, hook, on_acc)
    y = walk(ops, x[None] if single else x)
    y = y[0] if single else y
    return (y, ops.out) if intermediates else y
