"""Designed weight packs for the fp16 kernel (helper module, like model_variants.py): packs on which the kernel has ONE right answer.

A PROBE pack puts one layer L under test and turns every other conv into routing (one weight of 1.0 per output channel, one tap per depthwise
channel, bias 0): a designed frame -- values 0 or multiples of 1/16 in [1/16, 1], never fp16 subnormals (subnormal inputs are out of scope) -- reaches
L's input through a known index map, L has every weight and bias non-zero (both signs, small integers times powers of two), and routing convs
bring a group of L's output channels and one spatial phase to the 7x7x18 head.  The conv right behind L also carries a bias that lifts L's negative
outputs above zero, so that they cross the later LeakyReLUs unchanged; the residual branches beside the data's path are zeroed, the pool halves
of conv2d_23 / conv2d_47 have zero weights.  POOL packs put distinct values on every pixel of a pool's input planes (positive planes and
all-negative ones), ADD packs keep both operands of a residual add live with an operand that its own fp16 rounding changes, and the packs of
conv2d_23 / conv2d_47 are the CONCAT packs: both halves of their input carry different live data.

The certificate (certify): every accumulator's terms -- products, bias, residual operand -- are multiples of one power of two q and the sum of their
magnitudes is below 2^24 q, so every float32 summation order is exact.  Nothing here is written to the repository: packs are built in memory
(seeded, deterministic) and written to a temporary file by the GPU test.
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle.np_fp16 import LAYERS, POOLS, run_fp16, walk, load_yfw      # noqa: E402

SHIPPED = os.path.join(ROOT, "stm32h7-yolo_amd", "model", "yoloface_fp32.yfw")
TRIPLES = [(6, 7, 8), (13, 14, 15), (16, 17, 18)]
PHASE_TAPS = [(1, 1), (1, 2), (2, 1), (2, 2)]            # the taps of a stride-2 3x3 conv that never read the halo
N_FRAMES = 2
# profiles/fp16_faithful.txt: 4 x the largest spread between run_fp16's three accumulation modes over the 38 tolerance frames and the three weight sets
FAITHFUL_ATOL = 3.759e-2
FAITHFUL_RTOL = 3.787e-2


def blank():
    return [dict(dw=bool(d), cin=ci, cout=co, k=k, stride=s, w=np.zeros((3, 3, co) if d else (co, k, k, ci), np.float32), b=np.zeros(co, np.float32))
            for d, ci, co, k, s, _, _ in LAYERS]


def to_yfw(convs, path=None):
    import importlib
    mf = importlib.import_module("stm32h7-yolo_amd.model_file")
    return mf.write_yfw([(c["w"].reshape(1, 3, 3, -1) if c["dw"] else c["w"], c["b"], c["dw"]) for c in convs], path)


def _triple_of(i):
    for t in TRIPLES:
        if i in t:
            return t
    return None


def _on_path(i, L):
    """is conv i on the data's path of a pack whose layer under test is L (an index; pools: the conv behind them minus a half)"""
    t = _triple_of(i)
    return t is None or (L in t)


# ------------------------------------------------------------------------------------------------ routing in front of L
ALL_TAPS = [(1, 1), (1, 2), (2, 1), (2, 2), (0, 1), (1, 0), (0, 0), (0, 2), (2, 0)]      # the halo-free ones first


def _front(convs, upto, rng, combo=False, distinct=False):
    """convs[0 .. upto-1] as routing.  combo: conv2d_5 folds three source channels into ONE 11-bit value (pool packs).
    distinct (probe packs): the tensor that conv `upto` reads -- both halves of a concat included -- has pairwise DIFFERENT planes in all its channels,
    although the bottlenecks in front of it pass 4, 6 or 8: a routing depthwise conv gives every copy of a plane its own tap (another shift), and a
    routing 1x1 whose output nothing can shift any more adds two-term mixes a + b, then a + b / 2, of its distinct inputs.  Planes are tracked as descriptors."""
    nlive = 3
    desc = []                                            # per channel of the current tensor: what plane it holds
    path = [i for i in range(upto) if _on_path(i, upto if upto < 24 else -1)]
    # tensors with a second reader that no depthwise conv precedes: conv2d_6's output feeds pool_8 (the pool half of conv 10's input), conv 10's feeds pool_25
    must_mix = {3: upto in (4, 10), 10: upto in (11, 20)}
    for n, i in enumerate(path):
        c = convs[i]
        nxt = path[n + 1] if n + 1 < len(path) else upto
        if i == 0:
            for o in range(6 if combo else 8):
                ky, kx = [(1, 1), (1, 2), (2, 1)][o // 3]
                c["w"][o, ky, kx, o % 3] = 1.0
            nlive = 8
            desc = [(((o,), 1.0),) for o in range(8)]       # a plane = a sorted tuple of ((source, taps ...), coefficient): equal descriptors <=> equal planes
        elif c["dw"]:
            if not distinct:
                c["w"][1, 1, :] = 1.0
                continue
            taps = ALL_TAPS if c["stride"] == 2 else [(1, 1)] + ALL_TAPS[1:]
            used, out = set(), []
            for ch in range(c["cout"]):
                t, d = next((t, d) for t in taps for d in [tuple(sorted((b + (t,), k) for b, k in desc[ch]))] if d not in used)
                used.add(d); out.append(d)
                c["w"][t[0], t[1], ch] = 1.0
            desc = out
        elif combo and i == 2:
            for m in range(2):
                c["w"][m, 0, 0, 3 * m:3 * m + 3] = [2.0, 2.0 ** -3, 2.0 ** -7]
            nlive = 2
        elif not distinct:
            base = 18 if i == 10 else 24 if i == 20 else 0
            for o in range(c["cout"]):
                c["w"][o, 0, 0, base + o % nlive] = 1.0
            nlive = c["cout"]
        else:
            base = 18 if i == 10 else 24 if i == 20 else 0
            uniq = []                                    # (channel, descriptor) of the distinct input planes, in channel order
            for ch, d in enumerate(desc):
                if d not in [u[1] for u in uniq]:
                    uniq.append((base + ch, d))
            shifts_later = nxt < upto and convs[nxt]["dw"] and not must_mix.get(i, False)
            nu = len(uniq)                               # the mixes: a + b of every unordered pair first (no finer grid), then a + b / 2 of every ordered one
            pairs = [(a, b, 1.0) for a in range(nu) for b in range(a + 1, nu)] + [(a, (a + k) % nu, 0.5) for k in range(1, nu) for a in range(nu)]

            def mixed(a, b, wb):
                m = dict(uniq[a][1])
                for base_, k in uniq[b][1]:
                    m[base_] = m.get(base_, 0.0) + wb * k
                return tuple(sorted(m.items()))
            pairs = iter(pairs)
            seen = {u[1] for u in uniq}
            out = []
            for o in range(c["cout"]):
                if o < len(uniq) or shifts_later:
                    ch, d = uniq[o % len(uniq)]
                    c["w"][o, 0, 0, ch] = 1.0
                else:
                    a, b, wb, d = next((a, b, wb, d) for a, b, wb in pairs for d in [mixed(a, b, wb)] if d not in seen)
                    seen.add(d)
                    c["w"][o, 0, 0, uniq[a][0]], c["w"][o, 0, 0, uniq[b][0]] = 1.0, wb
                out.append(d)
            desc = out
            nlive = c["cout"]
    return nlive


def _designed(c, rng, T, grid_in=2.0 ** -4):
    """every weight and bias non-zero, both signs, {1,2,3} x 2^-e.  grid_in: the power of two that divides every input value.  The products' grid
    grid_in 2^-e stays >= 2^-10, so that 0.1 x of a negative output is no fp16 subnormal, and e is as large as that allows (and at least what keeps
    |accumulator| small: T 3 2^-e <= 2.25), which keeps the lifting bias small enough for an exact sum (the certificate checks the actual values)"""
    e_max = 10 + int(round(math.log2(grid_in)))
    e = min(max(3, math.ceil(math.log2(T / 0.75))), e_max)
    shape = c["w"].shape
    mag = rng.integers(1, 4, shape).astype(np.float32)
    ex = e + (rng.integers(0, 2, shape) if e < e_max else np.zeros(shape, np.int64))
    sign = np.where(rng.integers(0, 2, shape) == 1, 1.0, -1.0)
    per_out = sign.reshape(9, -1).T if c["dw"] else sign.reshape(c["cout"], -1)       # views: both signs in every output channel
    for row in per_out:
        if (row == row[0]).all():
            row[0] = -row[0]
    c["w"][...] = sign * mag * np.exp2(-ex.astype(np.float64))
    c["b"][...] = np.where(rng.integers(0, 2, c["cout"]) == 1, 1.0, -1.0) * rng.integers(1, 4, c["cout"]) * 0.125
    w2 = c["w"].reshape(-1, c["cout"]) if c["dw"] else c["w"].reshape(c["cout"], -1).T
    assert (c["w"] != 0).all() and (w2 > 0).any(axis=0).all() and (w2 < 0).any(axis=0).all()


# ------------------------------------------------------------------------------------------------ routing behind L
def _back(convs, first, pos, phases, L):
    """convs[first ..] route the channels at positions `pos` of the current tensor to head channels 0 .. len(pos)-1; returns the conv that lifts"""
    phases = list(phases)
    lift = None
    for i in range(first, 24):
        c = convs[i]
        if not _on_path(i, L):
            continue
        if i == 10:
            pos = [p + 18 for p in pos]                     # conv2d_19's output is the conv half of concat_22 ...
        if i == 20:
            pos = [p + 24 for p in pos]                     # ... and conv2d_42's the conv half of concat_46
        if lift is None:
            lift = i
        if c["dw"]:
            ky, kx = phases.pop(0) if c["stride"] == 2 else (1, 1)
            for p in pos:
                c["w"][ky, kx, p] = 1.0
        else:
            for j, p in enumerate(pos):
                c["w"][j, 0, 0, p] = 1.0
            pos = list(range(len(pos)))
    assert not phases
    return lift


def _group_size(L):
    return min([18] + [LAYERS[i][2] for i in range(L + 1, 24) if _on_path(i, L)])


def _n_phases(first):
    return 4 ** sum(1 for i in range(first, 24) if LAYERS[i][0] and LAYERS[i][4] == 2)


def _phase_list(first, ph):
    n = sum(1 for i in range(first, 24) if LAYERS[i][0] and LAYERS[i][4] == 2)
    return [PHASE_TAPS[(ph >> (2 * k)) & 3] for k in range(n)]


def _frames(rng, n=N_FRAMES, blocky=False):
    """random sixteenths; blocky: every 8x8 block of pixels has its own largest value, so that the maxima of the pool windows (16x16 pixels) vary
    (the packs of conv2d_23 / conv2d_47: a live pool half)"""
    f = rng.integers(0, 17, (n, 56, 56, 3))
    if blocky:
        cap = np.repeat(np.repeat(rng.integers(1, 17, (n, 7, 7, 1)), 8, axis=1), 8, axis=2)
        f = np.minimum(f, cap)
    return (f / 16.0).astype(np.float16)


def _set_lift(pack, lift, live_pos, tensor_key, linear):
    """the bias of conv `lift` on the live channels: a power of two above the most negative value of the tensor it reads (from the reference's own run)"""
    if lift is None or lift == 23:
        return
    _, inter = run_fp16(pack["convs"], pack["frames"], intermediates=True)
    lo = float(inter[tensor_key].astype(np.float64).min())
    if lo >= 0:
        return
    B = 2.0 ** math.ceil(math.log2(-lo * (1 if linear else 2)))
    c = pack["convs"][lift]
    for p in live_pos:
        c["b"][p] = B
    pack["lift"] = (lift, B)


def input_of(convs, frames, L):
    """the tensor conv L reads on these frames [N,H,W,Cin] (fp16), from the reference's own run"""
    return run_fp16(convs, frames, intermediates=True)[1][("in", L)]


def probe_pack(L, group, phase, seed=0):
    rng = np.random.default_rng([seed, L, group, phase])
    convs = blank()
    _front(convs, L, rng, distinct=True)
    d, cin, cout, k, s, act, _ = LAYERS[L]
    frames = _frames(rng, blocky=L in (10, 20))
    grid_in = float(_lowbit(input_of(convs, frames, L).astype(np.float64)).min())
    _designed(convs[L], rng, 9 if d else cin * k * k, grid_in)
    gs = _group_size(L)
    chans = list(range(group * gs, min((group + 1) * gs, cout)))
    lift = _back(convs, L + 1, chans, _phase_list(L + 1, phase), L)
    pack = dict(name=f"conv{L:02d}-g{group}-p{phase}", kind="conv", layer=L, convs=convs, frames=frames)
    if lift is not None:
        nxt = convs[lift]
        live = chans if nxt["dw"] else list(range(len(chans)))
        _set_lift(pack, lift, live, L, linear=not act)
    return pack


def probe_packs(L):
    gs, cout = _group_size(L), LAYERS[L][2]
    return [probe_pack(L, g, ph) for g in range((cout + gs - 1) // gs) for ph in range(_n_phases(L + 1))]


# ------------------------------------------------------------------------------------------------ pool packs
def _digit_frames(rng, width, n=N_FRAMES):
    """frames whose conv2d_1 routing (combo front) gives every pixel of a width x width grid of t1 an own 11-bit number n = 128 + perm: the digits
    n >> 8, (n >> 4) & 15, n & 15 (sixteenths) in the three colours of frame pixel (2y, 2x) (tap (1,1)) and, with another permutation, (2y, 2x+1)"""
    f = np.zeros((n, 56, 56, 3), np.float64)
    step = 28 // width                               # the grid's pixels on t1: every step-th
    for k in range(n):
        for m in range(2):
            num = 128 + rng.permutation(width * width).reshape(width, width)
            dig = np.stack([num >> 8, (num >> 4) & 15, num & 15], axis=-1) / 16.0
            f[k, 0:56:2 * step, m:56:2 * step] = dig
    return f.astype(np.float16)


def pool_pack(which, group, phase, negative, seed=0):
    rng = np.random.default_rng([seed, 100 + which, group, phase, int(negative)])
    convs = blank()
    sign = -1.0 if negative else 1.0
    if which == 0:                                   # pool_8 reads t4 = conv2d_6's output
        _front(convs, 3, rng, combo=True)
        for o in range(18):
            convs[3]["w"][o, 0, 0, o % 2] = sign
        gs, nch, first, base = 8, 18, 10, 0
    else:                                            # pool_25 reads t15 = conv2d_23's output
        nl = _front(convs, 10, rng, combo=True)
        assert nl == 18
        for o in range(24):
            convs[10]["w"][o, 0, 0, 18 + o % 18] = sign
        gs, nch, first, base = 18, 24, 20, 0
    chans = list(range(group * gs, min((group + 1) * gs, nch)))
    c = convs[first]
    for j, p in enumerate(chans):
        c["w"][j, 0, 0, base + p] = sign             # a negative plane comes back positive: -1 x, exact
    _back(convs, first + 1, list(range(len(chans))), _phase_list(first + 1, phase), "pool")
    return dict(name=f"pool{which}-g{group}-p{phase}-{'neg' if negative else 'pos'}", kind="pool", layer=which, convs=convs,
                frames=_digit_frames(rng, 28 if which == 0 else 14))


def pool_packs(which):
    first, gs, nch = (10, 8, 18) if which == 0 else (20, 18, 24)
    return [pool_pack(which, g, ph, neg) for g in range((nch + gs - 1) // gs) for ph in range(_n_phases(first + 1)) for neg in (False, True)]


# ------------------------------------------------------------------------------------------------ add packs
ADD_LAYERS = [8, 15, 18]
ADD_PRODUCER = [5, 12, 15]


def add_pack(which, phase, seed=0):
    """both operands live: the producer of the residual operand sums three inputs at scales 1, 2^-6, 2^-9 (14 bits: its fp16 rounding is not the
    identity), the branch routes the operand through and its last conv takes -33/64 of it, so that the sum 31/64 t needs its own rounding too"""
    rng = np.random.default_rng([seed, 200 + which, phase])
    convs = blank()
    P, A = ADD_PRODUCER[min(which, 1)], ADD_LAYERS[which]
    _front(convs, P, rng)
    cp = convs[P]
    for j in range(cp["cout"]):
        for m, sc in enumerate((1.0, 2.0 ** -6, 2.0 ** -9)):
            cp["w"][j, 0, 0, (j + m * cp["cout"]) % cp["cin"]] = sc
    live_triples = [TRIPLES[0]] if which == 0 else [TRIPLES[1]] if which == 1 else [TRIPLES[1], TRIPLES[2]]
    for a, b, c in live_triples:
        n = convs[c]["cout"]
        for o in range(convs[a]["cout"]):
            convs[a]["w"][o, 0, 0, o % n] = 1.0
        convs[b]["w"][1, 1, :] = 1.0
        for j in range(n):
            convs[c]["w"][j, 0, 0, j] = -33.0 / 64
    n = convs[A]["cout"]
    _back(convs, 9 if which == 0 else 19, list(range(n)), _phase_list(A + 1, phase), -1)
    return dict(name=f"add{which}-p{phase}", kind="add", layer=A, convs=convs, frames=_frames(rng))


def add_packs(which):
    return [add_pack(which, ph) for ph in range(_n_phases(ADD_LAYERS[which] + 1))]


# ------------------------------------------------------------------------------------------------ the whole set, by test case
def case_names():
    return [f"conv{L:02d}" for L in range(24)] + ["pool0", "pool1", "add0", "add1", "add2"]


_cache = {}


def packs_of(case):
    if case not in _cache:
        _cache[case] = (probe_packs(int(case[4:])) if case.startswith("conv") else pool_packs(int(case[4:])) if case.startswith("pool")
                        else add_packs(int(case[3:])))
    return _cache[case]


# ------------------------------------------------------------------------------------------------ certificate
def _lowbit(t):
    """the largest power of two that divides each non-zero float64 (inf where t == 0)"""
    m, e = np.frexp(np.abs(t))
    mi = (m * 2.0 ** 53).astype(np.int64)
    low = (mi & -mi).astype(np.float64)
    with np.errstate(divide="ignore", over="ignore"):
        return np.where(t == 0, np.inf, np.ldexp(low, e - 53))


def certify(convs, frames, logits=False):
    """[] when every accumulator of every layer is exact in any float32 order, else a list of (layer, count of failing accumulators, worst ratio); logits=True: (that list, run_fp16's logits of the same run)"""
    bad = []

    def on_acc(i, terms, bias, res):
        parts = [terms, np.broadcast_to(bias.astype(np.float64), terms.shape[:-1])[..., None]]
        if res is not None:
            parts.append(res[..., None])
        t = np.concatenate(parts, axis=-1)
        q = _lowbit(t).min(axis=-1)
        ratio = np.abs(t).sum(axis=-1) / (q * 2.0 ** 24)          # q = inf (all terms zero): ratio 0
        if (ratio >= 1).any():
            bad.append((i, int((ratio >= 1).sum()), float(ratio.max())))

    y = run_fp16(convs, frames, on_acc=on_acc)
    return (bad, y) if logits else bad


# ------------------------------------------------------------------------------------------------ coverage: which elements reach the head
class _IdOps:
    """walk() on index tensors [H,W,C]: the tensor under test gets the ids 0 .. size-1, routing convs move ids, everything else is -1"""
    def __init__(self, convs, target):
        self.convs, self.target = convs, target

    def conv(self, i, x, res=None, res_layer=None):
        d, cin, cout, k, s, _, ow = LAYERS[i]
        if self.target == ("conv", i):
            return np.arange(ow * ow * cout).reshape(ow, ow, cout)
        out = np.full((ow, ow, cout), -1, np.int64)
        c = self.convs[i]
        if (x >= 0).any():
            if c["dw"]:
                xp = np.full((x.shape[0] + 2, x.shape[1] + 2, cout), -1, np.int64)
                xp[1:-1, 1:-1] = x
                for ch in range(cout):
                    nz = np.argwhere(c["w"][:, :, ch] != 0)
                    if len(nz) == 1:
                        ky, kx = nz[0]
                        out[:, :, ch] = xp[ky:ky + (ow - 1) * s + 1:s, kx:kx + (ow - 1) * s + 1:s, ch]
                    else:
                        assert len(nz) == 0 or (x[:, :, ch] < 0).all(), f"conv {i} channel {ch} is not routing"
            elif k == 3:
                xp = np.full((x.shape[0] + 2, x.shape[1] + 2, cin), -1, np.int64)
                xp[1:-1, 1:-1] = x
                for o in range(cout):
                    nz = np.argwhere(c["w"][o] != 0)
                    assert len(nz) <= 1, f"conv {i} output {o} is not routing"
                    if len(nz):
                        ky, kx, ch = nz[0]
                        out[:, :, o] = xp[ky:ky + (ow - 1) * s + 1:s, kx:kx + (ow - 1) * s + 1:s, ch]
            else:
                w = c["w"].reshape(cout, cin)
                for o in range(cout):
                    nz = [p for p in np.nonzero(w[o])[0] if (x[:, :, p] >= 0).any()]
                    assert len(nz) <= 1, f"conv {i} output {o} mixes live channels {nz}"
                    if nz:
                        out[:, :, o] = x[:, :, nz[0]]
        if res is not None:
            assert not ((out >= 0) & (res >= 0)).any()
            out = np.where(out >= 0, out, res)
        return out

    def pool(self, which, x):
        w = x.shape[0] // 2
        if self.target == ("pool", which):
            return np.arange(w * w * x.shape[2]).reshape(w, w, x.shape[2])
        return np.full((w, w, x.shape[2]), -1, np.int64)

    def concat(self, layer, pooled, x):
        return np.concatenate([pooled, x], axis=-1)


def head_ids(pack, target=None):
    """[7,7,18]: for every head element the element of the tensor under test it shows (flat index), or -1"""
    target = target or ("pool" if pack["kind"] == "pool" else "conv", pack["layer"])
    x0 = np.arange(56 * 56 * 3).reshape(56, 56, 3) if target == ("input", 0) else np.full((56, 56, 3), -1, np.int64)
    return walk(_IdOps(pack["convs"], target), x0)


def coverage(case):
    """(elements of the case's tensor seen at some head element of some pack, elements of the tensor)"""
    packs = packs_of(case)
    if packs[0]["kind"] == "pool":
        w = 14 if packs[0]["layer"] == 0 else 7
        size = w * w * (18 if packs[0]["layer"] == 0 else 24)
    else:
        _, _, cout, _, _, _, w = LAYERS[packs[0]["layer"]]
        size = w * w * cout
    seen = np.zeros(size, bool)
    for p in packs:
        ids = head_ids(p)
        seen[ids[ids >= 0]] = True
    return int(seen.sum()), size


def describe(pack, flat):
    """a head element's flat index -> text that names the element of the tensor under test behind it"""
    hid = int(head_ids(pack).reshape(-1)[flat])
    y, x, c = np.unravel_index(flat, (7, 7, 18))
    if hid < 0:
        return f"head[{y},{x},{c}] (routes nothing)"
    if pack["kind"] == "pool":
        w, ch = (14, 18) if pack["layer"] == 0 else (7, 24)
        what = f"pool_{'8' if pack['layer'] == 0 else '25'}"
    else:
        _, _, ch, _, _, _, w = LAYERS[pack["layer"]]
        what = f"conv {pack['layer']}"
    ty, tx, tc = np.unravel_index(hid, (w, w, ch))
    return f"head[{y},{x},{c}] = {what} output[{ty},{tx},{tc}]"


# ------------------------------------------------------------------------------------------------ distinct frames through every batch slot
def routing_pack():
    """input -> head by routing alone: the head is a gather of the frame (head_ids(pack, ('input', 0)))"""
    rng = np.random.default_rng(77)
    convs = blank()
    _front(convs, 24, rng)
    for c in (convs[k] for t in TRIPLES for k in t):
        c["w"][...] = 0
    return dict(name="routing", kind="routing", layer=-1, convs=convs, frames=None)


def indexed_frames(n, seed=5):
    """n frames, every one different: pixel value ((base + digit of the frame index) mod 16 + 1) / 16, the digit (base 16, three of them) chosen by the
    pixel's position mod 3 -- the frame index can be read off any three neighbouring values"""
    base = np.random.default_rng(seed).integers(0, 16, 56 * 56 * 3).astype(np.uint8)
    idx = np.arange(n, dtype=np.int64)
    digits = np.stack([(idx >> 0) & 15, (idx >> 4) & 15, (idx >> 8) & 15], axis=1).astype(np.uint8)       # n < 4096
    assert n <= 4096
    code = digits[:, np.arange(56 * 56 * 3) % 3]
    lut = (np.arange(1, 17) / 16.0).astype(np.float16)
    return np.ascontiguousarray(lut[(base[None, :] + code) % 16]).reshape(n, 56, 56, 3)       # (fancy indexing hands back a transposed layout)


# ------------------------------------------------------------------------------------------------ real weights: shipped, jittered, permuted
def tolerance_frames():
    """the 8 + 30 frames of test_baseline_config4_fp16_tolerance and test_fp16_tolerance_on_structured_extreme_frames, as uint8"""
    rng = np.random.default_rng(3)
    u8 = rng.integers(0, 256, (8, 56, 56, 3), dtype=np.uint8)
    gold = np.fromfile(os.path.join(ROOT, "tests", "golden", "golden_inputs.bin"), np.int8).reshape(-1, 56, 56, 3)
    u8[:6] = (gold.astype(np.int16) + 128).astype(np.uint8)
    frames = [np.full((56, 56, 3), v, np.uint8) for v in (0, 255)]
    for r in (0, 255):
        for g in (0, 255):
            for b in (0, 255):
                frames.append(np.broadcast_to(np.array([r, g, b], np.uint8), (56, 56, 3)).copy())
    yy, xx = np.mgrid[0:56, 0:56]
    for period in (1, 2, 4, 7):
        for pat in ((xx // period) % 2, (yy // period) % 2, ((xx // period) + (yy // period)) % 2):
            frames.append(np.broadcast_to(np.where(pat[..., None] == 1, 255, 0).astype(np.uint8), (56, 56, 3)).copy())
    frames += list(np.where(np.random.default_rng(7).integers(0, 2, (6, 56, 56, 3)) == 1, 255, 0).astype(np.uint8))
    return np.concatenate([u8, np.stack(frames)])


def real_weight_sets():
    """{'shipped', 'jitter' (every weight and bias x (1 +- 2 %), seeded), 'permuted' (the channels of the 4-, 6- and 8-channel bottlenecks permuted
    consistently: the same function, another slot layout and summation order)}"""
    shipped = load_yfw(SHIPPED)
    rng = np.random.default_rng(2024)
    jit = [dict(c, w=(c["w"] * (1 + 0.02 * rng.uniform(-1, 1, c["w"].shape))).astype(np.float32),
                b=(c["b"] * (1 + 0.02 * rng.uniform(-1, 1, c["b"].shape))).astype(np.float32)) for c in shipped]
    perm = [dict(c, w=c["w"].copy(), b=c["b"].copy()) for c in shipped]

    def out_perm(i, p):
        perm[i]["w"], perm[i]["b"] = perm[i]["w"][p], perm[i]["b"][p]

    def in_perm(i, p):
        perm[i]["w"] = perm[i]["w"][..., p]

    p4, p6, p8 = rng.permutation(4), rng.permutation(6), rng.permutation(8)
    out_perm(2, p4); in_perm(3, p4)
    out_perm(5, p6); in_perm(6, p6); out_perm(8, p6); in_perm(9, p6)
    out_perm(12, p8); in_perm(13, p8); out_perm(15, p8); in_perm(16, p8); out_perm(18, p8); in_perm(19, p8)
    return dict(shipped=shipped, jitter=jit, permuted=perm)


def measure_spread():
    """per weight set: the largest pairwise difference between the three accumulation modes of run_fp16 over the 38 tolerance frames, absolute (over
    logits of magnitude <= 1) and relative (over the others) -- what summation order and the fp16 flips it causes can do to this net"""
    x16 = (tolerance_frames().astype(np.float32) / 255).astype(np.float16)
    out = {}
    for name, convs in real_weight_sets().items():
        r = np.stack([run_fp16(convs, x16, accumulate=m) for m in ("f64", "f32_forward", "f32_reverse")]).astype(np.float64)
        spread = r.max(axis=0) - r.min(axis=0)
        mag = np.abs(r[0])
        small = mag <= 1
        out[name] = (float(spread[small].max()), float((spread[~small] / mag[~small]).max()), float(spread.max()), float(mag.max()))
    return out


if __name__ == "__main__":
    for name, (a, r, worst, mag) in measure_spread().items():
        print(f"{name:9s} spread: abs (|logit| <= 1) {a:.3e}   rel (|logit| > 1) {r:.3e}   largest anywhere {worst:.3e}   largest |logit| {mag:.2f}")
    for case in case_names():
        print(case, len(packs_of(case)), "packs, coverage", coverage(case))
