"""The float side of the image path without a GPU: the host build of csrc/yf_images_float.h (the functions the kernels call) against numpy.
The 256 halves of pixel / 255., the exponential E (the float32 nearest to the float64 e^x) on the whole float32 domain, the decode of
float32 logits against a numpy restatement of h5_predition.py:51-72 (tests/float_support.py), and the distance between that decode and
the script run literally with numpy's own float32 exp."""
import numpy as np
import pytest

import float_support as fs
from images_support import REF_SIZES


@pytest.fixture(scope="module")
def lib():
    return fs.float_host()


@pytest.fixture(scope="module")
def real_logits():
    return fs.fp32_logits(fs.real_frames_u8())


def test_halves_equal_every_numpy_route(lib):
    v = np.arange(256)
    got = fs.host_halves(lib)
    via_f32 = (v / 255.).astype(np.float32).astype(np.float16)              # the script's float64, the model's float32, the network's fp16
    f32_div = (v.astype(np.float32) / np.float32(255)).astype(np.float16)
    direct = (v / 255.).astype(np.float16)
    for want in (via_f32, f32_div, direct):
        assert np.array_equal(got, want.view(np.uint16))
    assert got[0] == 0 and got[255] == 0x3C00


def _same_floats(a, b):
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def _check_exp(lib, x, what):
    x = np.ascontiguousarray(x, np.float32)
    got, want = fs.host_exp(lib, x), fs.exp_rounded(x)
    bad = ~_same_floats(got, want)
    # (should an argument ever disagree on another libm: decide with exact arithmetic which side is the nearest float32 first)
    assert not bad.any(), (what, int(bad.sum()), x[bad][:4].view(np.uint32), got[bad][:4], want[bad][:4])
    return want


def test_exp_on_a_sample_of_the_working_range(lib):
    x = np.random.default_rng(2).uniform(-30, 30, 4_000_000).astype(np.float32)
    _check_exp(lib, x, "sample")


def test_exp_over_the_whole_domain(lib):
    x = np.arange(0, 2 ** 32, 4099, dtype=np.uint64).astype(np.uint32).view(np.float32)
    want = _check_exp(lib, x, "every 4099th pattern")
    assert np.isnan(want).any() and np.isinf(want).any() and (want == 0).any() and ((want > 0) & (want < np.float32(2.0 ** -126))).any()


def test_exp_at_the_edges_of_the_domain(lib):
    f32 = np.finfo(np.float32)
    centres = [0.0, -0.0, np.inf, -np.inf, np.log(float(f32.max)), np.log(2.0 ** -126), np.log(2.0 ** -149), np.log(2.0 ** -150), 1.0, -1.0]
    bits = np.float32(centres).view(np.uint32).astype(np.int64)
    x = ((bits[:, None] + np.arange(-24, 25)[None, :]) & 0xFFFFFFFF).astype(np.uint32).view(np.float32).reshape(-1)
    x = np.concatenate([x, np.float32([np.nan]), np.uint32([0x7FC00001, 0xFFC00000, 0x7F800001]).view(np.float32)])
    want = _check_exp(lib, x, "edges")
    fin = np.sort(x[np.isfinite(x)])
    w = fs.exp_rounded(fin)
    # the neighbourhoods hold the transitions themselves: the largest argument that stays finite and its successor, the first subnormal
    # result, the last nonzero result
    assert (np.isfinite(w) & (fin > 88)).any() and (np.isinf(w) & (fin > 88) & (fin < 89)).any()
    assert ((w >= f32.tiny) & (fin < -87)).any() and ((w > 0) & (w < f32.tiny) & (fin > -88)).any()
    assert ((w > 0) & (fin < -103)).any() and ((w == 0) & (fin > -104)).any()
    assert np.isnan(want[-4:]).all()
    got = fs.host_exp(lib, np.float32([np.inf, -np.inf, 0.0, -0.0]))
    assert got[0] == np.inf and got[1] == 0 and not np.signbit(got[1]) and got[2] == 1 and got[3] == 1


def test_sigmoid_is_two_float32_operations_around_exp(lib):
    x = np.concatenate([np.random.default_rng(3).uniform(-30, 30, 1_000_000).astype(np.float32), fs.special_logits().reshape(-1)])
    with np.errstate(over="ignore"):
        want = np.float32(1) / (np.float32(1) + fs.exp_rounded(-x))
    assert _same_floats(fs.host_exp(lib, x, "yfi_sigmoid_f32_host"), want).all()


def _check_decode(lib, logits, scales, caps=(147,)):
    """the host decode of every frame against the restatement, record for record and byte for byte; returns the total of records"""
    total = 0
    for f, t in enumerate(logits):
        for ws, hs in scales:
            want, _ = fs.decode_restated(t, f, ws, hs)
            for cap in caps:
                count, got = fs.host_decode(lib, t, f, ws, hs, cap)
                assert count == want.shape[0], (f, ws, hs, cap, count, want.shape[0])
                assert fs.same_bytes(got, want[:cap]), (f, ws, hs, cap)
            total += want.shape[0]
    return total


SCALES = [(1.0, 1.0), fs.scales_of(410, 410), fs.scales_of(16384, 16384), fs.scales_of(410, 362)]


def test_decode_on_the_real_frames(lib, real_logits):
    assert real_logits.shape == (27, 7, 7, 18)
    fired = [fs.decode_restated(t, f, 1.0, 1.0)[0].shape[0] for f, t in enumerate(real_logits)]
    assert sum(fired) == 47 and sum(1 for k in fired if k == 0) == 1, fired
    _check_decode(lib, real_logits, SCALES + [fs.scales_of(w, h) for (w, h) in REF_SIZES[:3]], caps=(147, 1))


def test_decode_on_seeded_logits(lib):
    logits = fs.seeded_logits()
    total = _check_decode(lib, logits[:128], SCALES, caps=(147, 20))
    total += _check_decode(lib, logits[128:], SCALES[1:2])
    assert total > 512 * 10                                          # P(N(0, 3) > ln(7/3)) = 0.39: about 57 of 147 fire


def test_decode_on_specials(lib):
    logits = fs.special_logits()
    total = _check_decode(lib, logits, SCALES, caps=(147, 100, 3))
    assert total > 0
    # the threshold: of ln(7/3)'s float32 neighbourhood some fire and some do not, and all 147 candidates of the full frames do
    nb = fs.threshold_neighbours()
    conf = np.float32(1) / (np.float32(1) + fs.exp_rounded(-nb))
    assert (conf > np.float32(0.7)).any() and not (conf > np.float32(0.7)).all()
    assert fs.host_decode(lib, logits[-1], 0, 1.0, 1.0, 100)[0] == 147
    # INT32_MIN edges occur (NaN and infinite boxes), and so do records whose exponential overflowed or went subnormal
    recs = np.concatenate([fs.decode_restated(t, f, *SCALES[2])[0] for f, t in enumerate(logits)])
    assert (recs["x1"] == -2 ** 31).any() and (recs["x2"] == -2 ** 31).any()


def test_distance_to_the_script_run_literally(lib, real_logits, capsys):
    """h5_predition.py as it literally runs (numpy's own float32 exp) against the library's E on the 27 real frames at the reference's sizes:
    the same candidates fire, an edge differs by at most 1.  The number of differing edges is a description of this numpy build."""
    four_ulp = 4 * np.spacing(np.float32(0.7))
    differ = edges = fired = 0
    nearest = np.inf
    for f, (t, (w, h)) in enumerate(zip(real_logits, REF_SIZES)):
        ws, hs = fs.scales_of(w, h)
        mine, conf_mine = fs.decode_restated(t, f, ws, hs)
        lit, conf_lit = fs.decode_restated(t, f, ws, hs, E=fs.exp_numpy_f32)
        near = (np.abs(conf_mine - np.float32(0.7)) <= four_ulp) | (np.abs(conf_lit - np.float32(0.7)) <= four_ulp)
        assert not near.any(), "a confidence within 4 ulp of 0.7f: these inputs are wrong for this test"
        nearest = min(nearest, float(np.min(np.abs(conf_mine.astype(np.float64) - np.float32(0.7)) / np.spacing(np.float32(0.7)))))
        key = lambda r: list(zip(r["anchor"].tolist(), r["row"].tolist(), r["col"].tolist()))      # noqa: E731
        assert key(mine) == key(lit), f
        count, got = fs.host_decode(lib, t, f, ws, hs, 147)
        assert fs.same_bytes(got, mine)
        for e in ("x1", "y1", "x2", "y2"):
            d = np.abs(mine[e].astype(np.int64) - lit[e].astype(np.int64))
            assert (d <= 1).all(), (f, e, d.max())
            differ += int((d != 0).sum())
            edges += d.size
        fired += count
    assert fired == 47 and edges == 188
    with capsys.disabled():
        print(f"\n[float decode vs numpy's float32 exp] {fired} candidates fire on both sides, {differ} of {edges} edges differ by 1; "
              f"the confidence nearest to 0.7f is {nearest:.0f} ulp away")
