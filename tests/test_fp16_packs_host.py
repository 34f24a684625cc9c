"""The designed fp16 weight packs (tests/fp16_packs.py) and the fp16-faithful reference (oracle/np_fp16.py) on the CPU: every accumulator of every
pack is exact in any float32 order, the reference's three accumulation modes agree bit for bit, the packs show every output element of every conv,
pool and add at the head, and each of a list of subtly wrong evaluations changes some pack's expected head.  The kernel meets the same packs in
test_fp16_packs_gpu.py."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fp16_packs as fp            # noqa: E402
from oracle.np_fp16 import LAYERS, run_fp16                   # noqa: E402

MODES = ("f64", "f32_forward", "f32_reverse")
_expected = {}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def expected(pack):
    if pack["name"] not in _expected:
        _expected[pack["name"]] = run_fp16(pack["convs"], pack["frames"])
    return _expected[pack["name"]]


@pytest.mark.parametrize("case", fp.case_names())
def test_certificate_reference_agreement_and_coverage(case):
    """per pack and frame: the certificate (all terms of an accumulator multiples of one power of two q, sum of magnitudes < 2^24 q) holds for every
    accumulator of all 24 convs; the three accumulation modes of run_fp16 give the same float32 bits; the frames are 0 or sixteenths in [1/16, 1]; the pack
    is deterministic; and together the case's packs bring 100 % of the output elements of the tensor under test to some head element"""
    packs = fp.packs_of(case)
    for p in packs:
        f = p["frames"].astype(np.float64) * 16
        assert p["frames"].dtype == np.float16 and (f == np.round(f)).all() and f.min() >= 0 and f.max() <= 16, p["name"]
        bad, want = fp.certify(p["convs"], p["frames"], logits=True)
        assert bad == [], (p["name"], bad)
        _expected[p["name"]] = want
        assert np.isfinite(want).all() and len(np.unique(bits(want))) > 20, p["name"]               # a live head, not a constant
        for m in MODES[1:]:
            assert np.array_equal(bits(run_fp16(p["convs"], p["frames"], accumulate=m)), bits(want)), (p["name"], m)
    seen, size = fp.coverage(case)
    assert seen == size, f"{case}: {seen} of {size} output elements reach a head element"
    again = fp.probe_packs(int(case[4:]))[0] if case.startswith("conv") else fp.pool_packs(int(case[4:]))[0] if case.startswith("pool") else fp.add_packs(int(case[3:]))[0]
    assert fp.to_yfw(again["convs"]) == fp.to_yfw(packs[0]["convs"]) and np.array_equal(again["frames"], packs[0]["frames"])


def test_layer_under_test_has_every_weight_live():
    """at L: every weight and bias non-zero, both signs in every output channel, values small integers times powers of two (exact in fp16)"""
    for L in range(24):
        c = fp.packs_of(f"conv{L:02d}")[0]["convs"][L]
        w = c["w"].reshape(-1, c["cout"]) if c["dw"] else c["w"].reshape(c["cout"], -1).T
        assert (w != 0).all() and (c["b"] != 0).all() and (w > 0).any(axis=0).all() and (w < 0).any(axis=0).all(), L
        assert np.array_equal(c["w"].astype(np.float16).astype(np.float32), c["w"]) and np.isin(np.abs(w) * 128 % 1, 0).all(), L


def test_layer_under_test_reads_pairwise_distinct_planes():
    """every input channel of L carries its own data (the bottlenecks in front pass 4, 6 or 8 planes; the routing front makes cin different ones of them
    with per-channel taps and two-term mixes): a mix-up of input channels, 4-channel k-groups or k-steps changes the result"""
    for L in range(24):
        for p in (fp.packs_of(f"conv{L:02d}")[0], fp.packs_of(f"conv{L:02d}")[-1]):
            x = fp.input_of(p["convs"], p["frames"], L).astype(np.float64)
            planes = x.transpose(3, 0, 1, 2).reshape(x.shape[3], -1)
            assert len(np.unique(planes, axis=0)) == x.shape[3] == LAYERS[L][1], (p["name"], len(np.unique(planes, axis=0)))


def test_pool_packs_have_distinct_values_and_negative_planes():
    for which in (0, 1):
        for p in fp.packs_of(f"pool{which}"):
            _, inter = run_fp16(p["convs"], p["frames"], intermediates=True)
            plane = inter[3 if which == 0 else 10].astype(np.float64)                     # the pool's input: [N, W, W, C]
            n, w, _, c = plane.shape
            flat = np.sort(plane.reshape(n, w * w, c), axis=1)
            assert (np.diff(flat, axis=1) != 0).all(), p["name"]
            assert (plane < 0).all() if p["name"].endswith("neg") else (plane > 0).all(), p["name"]


def test_concat_packs_carry_two_live_halves():
    for L, pool_key, conv_key in ((10, "pool0", 9), (20, "pool1", 19)):
        p = fp.packs_of(f"conv{L}")[0]
        _, inter = run_fp16(p["convs"], p["frames"], intermediates=True)
        a, b = inter[pool_key].astype(np.float64), inter[conv_key].astype(np.float64)
        assert len(np.unique(a)) > 8 and len(np.unique(b)) > 8 and not np.array_equal(a[..., :8], b[..., :8])


def test_shipped_weights_stay_within_the_fp32_tolerance():
    """run_fp16 on the shipped pack against run_fp32 on the 8 + 30 frames of the two tolerance tests of test_gpu_parity.py: atol 2e-2 + rtol 2e-2"""
    from oracle.np_fp32 import run_fp32
    convs = fp.real_weight_sets()["shipped"]
    x32 = fp.tolerance_frames().astype(np.float32) / 255
    ref = np.stack([run_fp32(convs, f) for f in x32])
    got = run_fp16(convs, x32.astype(np.float16))
    err = np.abs(got - ref)
    assert np.all(err <= 2e-2 + 2e-2 * np.abs(ref)), f"worst use of the tolerance {(err / (2e-2 + 2e-2 * np.abs(ref))).max():.3f}"


def test_the_bound_of_the_faithful_comparison_is_the_measured_spread():
    """profiles/fp16_faithful.txt: the literals FAITHFUL_ATOL / FAITHFUL_RTOL of fp16_packs.py are 4 x the spread of the three accumulation modes, measured here again"""
    FAITHFUL_ATOL, FAITHFUL_RTOL = fp.FAITHFUL_ATOL, fp.FAITHFUL_RTOL
    s = fp.measure_spread()
    a, r = max(v[0] for v in s.values()), max(v[1] for v in s.values())
    assert abs(FAITHFUL_ATOL / (4 * a) - 1) < 0.01 and abs(FAITHFUL_RTOL / (4 * r) - 1) < 0.01, (a, r)
    text = open(os.path.join(ROOT, "profiles", "fp16_faithful.txt")).read()
    assert f"{FAITHFUL_ATOL:.3e}" in text and f"{FAITHFUL_RTOL:.3e}" in text


# ------------------------------------------------------------------------------------------------ sensitivity
def _shift(p):
    return p[:4] + [p[5]] + p[5:]                            # the centre tap reads its right neighbour


def _swap_taps(p):
    q = list(p); q[0], q[8] = q[8], q[0]; return q


def _swap_channels(wb):
    w, b = wb
    perm = np.arange(b.size); perm[[0, 1]] = [1, 0]
    return (w[..., perm] if w.ndim == 3 else w[perm]), b[perm]


def _swap_inputs(a, b):
    def f(wb):
        w, bias = wb
        perm = np.arange(w.shape[-1]); perm[[a, b]] = [b, a]
        return w[..., perm], bias
    return f


def _conv_half_at_18(cat):
    out = np.zeros_like(cat)
    out[..., :18] = cat[..., :18]
    out[..., 20:] = cat[..., 18:34]                          # weight c >= 18 meets buffer channel c: two padding zeros, then conv channel c - 20
    return out


CONV3 = [i for i in range(24) if LAYERS[i][3] == 3]
DEFECTS = ([(f"tap shifted, conv {i}", f"conv{i:02d}", {("taps", i): _shift}) for i in CONV3]
           + [(f"two taps swapped, conv {i}", f"conv{i:02d}", {("taps", i): _swap_taps}) for i in CONV3]
           + [(f"pad 0 on the left, conv {i}", f"conv{i:02d}", {("pad", i): (1, 0)}) for i in CONV3]
           + [(f"stride-2 phase off by one, conv {i}", f"conv{i:02d}", {("pad", i): (0, 0)}) for i in CONV3 if LAYERS[i][4] == 2]
           + [(f"output channels 0 and 1 swapped, conv {i}", f"conv{i:02d}", {("weights", i): _swap_channels}) for i in range(24)]
           + [(f"input channels {a} and {b} swapped, conv {i}", f"conv{i:02d}", {("weights", i): _swap_inputs(a, b)})
              for i in range(24) if not LAYERS[i][0] for a, b in ((0, 1), (0, 4), (0, 8), (1, 5), (4, 8)) if b < LAYERS[i][1]]
           + [("conv2d_23's conv half read at channel 18", "conv10", {("concat", 10): _conv_half_at_18})]
           + [(f"pool {w} window one short", f"pool{w}", {("pool", w): (k - 1, pad, False)}) for w, (k, pad) in enumerate(((8, 3), (4, 1)))]
           + [(f"pool {w}: zero padding takes part", f"pool{w}", {("pool", w): (k, pad, True)}) for w, (k, pad) in enumerate(((8, 3), (4, 1)))]
           + [(f"LeakyReLU slope 0.125, conv {i}", f"conv{i:02d}", {("slope", i): 0.125}) for i in range(24) if LAYERS[i][5]]
           + [(f"bias dropped, conv {i}", f"conv{i:02d}", {("bias", i): np.zeros_like}) for i in range(24)]
           + [(f"residual operand before its rounding, add {k}", f"add{k}", {("residual_pre", L): True}) for k, L in enumerate(fp.ADD_LAYERS)])


@pytest.mark.parametrize("what,case,hook", DEFECTS, ids=[d[0] for d in DEFECTS])
def test_a_subtly_wrong_evaluation_changes_some_packs_head(what, case, hook):
    """the defect goes into run_fp16 through its hook; some pack of the layer's case must then expect another head, i.e. would fail a kernel with that defect"""
    for p in fp.packs_of(case):
        if not np.array_equal(bits(run_fp16(p["convs"], p["frames"], hook=hook)), bits(expected(p))):
            return
    pytest.fail(f"no pack of {case} sees: {what}")


def test_routing_pack_is_an_exact_gather_of_the_frame():
    """the pack of the distinct-frames GPU test: certificate, and run_fp16 = the gather head_ids() states, on frames of distinct indices"""
    p = fp.routing_pack()
    frames = fp.indexed_frames(4096)[[0, 1, 511, 512, 513, 1024, 3584, 3591, 4095]]
    assert fp.certify(p["convs"], frames) == []
    ids = fp.head_ids(p, ("input", 0)).reshape(-1)
    live = ids >= 0
    want = np.zeros((len(frames), 882), np.float32)
    want[:, live] = frames.reshape(len(frames), -1)[:, ids[live]].astype(np.float32)
    for m in MODES:
        assert np.array_equal(bits(run_fp16(p["convs"], frames, accumulate=m)).reshape(len(frames), -1), bits(want)), m
    assert live.sum() >= 4 * 49 and len(np.unique(fp.indexed_frames(4096).reshape(4096, -1), axis=0)) == 4096
