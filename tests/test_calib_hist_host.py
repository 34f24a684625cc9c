"""Histogram calibration on the CPU: the host build of csrc/yf_calib_hist.h (yf_calib_host_histogram) pinned by hand-computed cases and
required to equal a numpy restatement count for count; ptq.clip_ranges; the .yfm of every method through the library's parser and table
builder; the refusals.  No GPU."""
import numpy as np
import pytest

import calib_support as cs
import calib_hist_support as hs
import model_variants as mv
from calib_support import calib, ptq, model_file
from test_model_file_host import hp, parse, prepare_model, ROUNDINGS      # noqa: F401  (hp is a fixture)

YFW = cs.yfw_bytes("yfw")
WIDE = {t: (-1.0, 1.0) for t in hs.slots()}


def _input_row(frames, rng, bins):
    return calib.host_histogram(YFW, frames, {**WIDE, 0: rng}, bins)[0].tolist()


# ---------------------------------------------------------------------------------------------------------------- yfc_hist_bin, by hand
def test_bin_of_the_ends_and_of_values_outside_by_hand():
    """The input tensor's values are known by hand: byte -128 is 0.0, byte 127 is 1.0, byte -77 is 51 / 255 = 0.2 (float32 0x3e4ccccd).
    One frame: 5 bytes of 0.0, 7 of 0.2, the other 9396 of 1.0."""
    f = np.full((1, 56, 56, 3), 127, np.int8)
    f.reshape(-1)[:5] = -128
    f.reshape(-1)[5:12] = -77
    assert _input_row(f, (0.0, 1.0), 4) == [12, 0, 0, 9396]               # v == min: bin 0; 0.2 * 4 = 0.8: bin 0; v == max: the LAST bin, not one past it
    assert _input_row(f, (0.0, 1.0), 5) == [5, 7, 0, 0, 9396]             # float32(0.2) * 5 = 1.0000000149 -> 1.0: bin 1
    assert _input_row(f, (0.0, 1.0), 1) == [9408]                         # bins = 1
    assert _input_row(f, (0.1, 0.5), 4) == [5, 7, 0, 9396]                # below the range: bin 0; (0.2 - 0.1) * 10 = 1.0: bin 1; above the range: the last bin
    assert _input_row(f, (0.2, 0.2), 4) == [9408, 0, 0, 0]                # max == min: inv = 0, everything in bin 0
    assert _input_row(f, (1.0, 1.0), 1) == [9408]
    assert _input_row(f, (0.0, 1.0), 4096) == [5] + [0] * 818 + [7] + [0] * 3275 + [9396]   # 0.2 * 4096 = 819.2
    assert hs.restate_bins([0.0, 0.2, 1.0, -3.0, 7.0, np.nan, np.inf, -np.inf], 0.0, 1.0, 5).tolist() == [0, 1, 4, 0, 4, 0, 4, 0]


def test_nan_and_infinities_by_hand():
    """A .yfw of finite weights that drives tensors to +inf, -inf and NaN on a white frame: conv 0 has 3e38 on channel 0, -3e38 on channel 1
    and a constant 0.25 on the others; the depthwise conv behind it has +1 / -1 alternating on channel 0 (inf - inf), +1 on channel 1 and a
    constant 0.75 on the others.  On the axis {-1, 1} with 4 bins: +inf in bin 3, -inf and NaN in bin 0, 0.25 in bin 2, 0.75 in bin 3."""
    convs = [(w.copy(), b.copy(), dw) for w, b, dw in model_file.read_yfw(YFW)]
    w0, b0, _ = convs[0]
    w0[...] = 0
    w0[0], w0[1] = 3e38, -3e38
    b0[:] = (0, 0, 0.25, 0.25, 0.25, 0.25, 0.25, 0.25)
    w1, b1, _ = convs[1]
    w1[...] = 0
    w1[0, :, :, 0] = np.array([1, -1, 1, -1, 1, -1, 1, -1, 1], np.float32).reshape(3, 3)
    w1[0, :, :, 1] = 1
    b1[:] = (0, 0, 0.75, 0.75, 0.75, 0.75, 0.75, 0.75)
    yfw = model_file.write_yfw(convs)
    white = np.full((1, 56, 56, 3), 127, np.int8)
    xs = hs.float_tensors(white, yfw)
    at = {t: i for i, t in enumerate(hs.slots())}
    assert np.isposinf(xs[at[51]]).sum() == 784 and np.isneginf(xs[at[51]]).sum() == 784
    assert np.isnan(xs[at[53]]).sum() == 784 and np.isneginf(xs[at[53]]).sum() == 784
    got = calib.host_histogram(yfw, white, WIDE, 4)
    assert got[at[51]].tolist() == got[at[52]].tolist() == [784, 0, 6 * 784, 784]
    assert got[at[53]].tolist() == got[at[54]].tolist() == [2 * 784, 0, 0, 6 * 784]
    hs.assert_same(got, hs.restate(xs, WIDE, 4), "NaN soup")
    hs.assert_conserved(got, 1, "NaN soup")


# ---------------------------------------------------------------------------------------------------------------- against the restatement
def _frame_sets():
    return [("3 real frames", cs.calib_frames()[:3]), ("structured extremes", mv.structured_extreme_frames())]


@pytest.fixture(scope="module")
def evaluated():
    """name -> (frames, their ranges, their 47 float32 tensors)"""
    return {name: (x, calib.host_run(YFW, x, threads=16, want_logits=False)[0], hs.float_tensors(x)) for name, x in _frame_sets()}


@pytest.mark.parametrize("bins", [2048, 16, 1])
@pytest.mark.parametrize("name", [s[0] for s in _frame_sets()])
def test_host_histogram_equals_the_numpy_restatement(evaluated, name, bins):
    x, ranges, tensors = evaluated[name]
    assert tuple(sorted(ranges)) == hs.slots() and len(tensors) == 47
    got = calib.host_histogram(YFW, x, ranges, bins, threads=16)
    hs.assert_same(got, hs.restate(tensors, ranges, bins), f"{name}, {bins} bins")
    hs.assert_conserved(got, x.shape[0], f"{name}, {bins} bins")
    if bins > 1:
        assert (got[:, 0] > 0).all() and (got[:, -1] > 0).all()           # the minimum and the maximum were counted, in the end bins


def test_slot_order_is_ascending_tensor_id():
    lib = calib.load_host()
    minmax, ids = np.zeros((47, 2), np.float32), np.zeros(47, np.int32)
    import ctypes
    err = ctypes.create_string_buffer(400)
    assert lib.yf_calib_host_run(YFW, len(YFW), cs.calib_frames()[:1].ctypes.data, 1, minmax.ctypes.data, ids.ctypes.data, None, 1, err, 400) == 1
    assert tuple(ids.tolist()) == hs.slots() == tuple(sorted(ids.tolist()))


def test_accumulation_and_threads():
    x, ranges = cs.calib_frames(), cs.host_result("yfw")[0]
    for bins in (2048, 16):
        whole = hs.host_counts(bins)
        hs.assert_conserved(whole, 27, f"27 frames, {bins} bins")
        parts = calib.host_histogram(YFW, x[:13], ranges, bins, threads=4)
        assert calib.host_histogram(YFW, x[13:], ranges, bins, threads=4, counts=parts) is parts
        hs.assert_same(parts, whole, f"[0:13] then [13:27], {bins} bins")
        one = calib.host_histogram(YFW, x, ranges, bins, threads=1)
        assert one.tobytes() == whole.tobytes()                           # 1 thread and 16 threads


def test_ranges_narrower_than_the_data_overflow_into_the_end_bins():
    x = cs.calib_frames()
    narrow = calib.host_run(YFW, x[:1], want_logits=False)[0]
    got = calib.host_histogram(YFW, x[:3], narrow, 16, threads=3)
    hs.assert_conserved(got, 3, "narrow axes")
    hs.assert_same(got, hs.restate(hs.float_tensors(x[:3]), narrow, 16), "narrow axes")


# ---------------------------------------------------------------------------------------------------------------- clip_ranges
def _f32_bits(r):
    return {t: tuple(np.array(v, np.float32).view(np.uint32).tolist()) for t, v in r.items()}


def test_minmax_and_percentile_one_return_the_bounds_bit_for_bit():
    ranges, counts = cs.host_result("yfw")[0], hs.host_counts(2048)
    assert _f32_bits(ptq.clip_ranges(counts, ranges, "minmax")) == _f32_bits(ranges)
    full = ptq.clip_ranges(counts, ranges, "percentile", percentile=1.0)
    assert _f32_bits(full) == _f32_bits(ranges) and full == ranges
    assert ptq.quantize_model(YFW, full) == cs.host_model("yfw")
    with pytest.raises(ValueError, match="method"):
        ptq.clip_ranges(counts, ranges, "entropy")
    with pytest.raises(ValueError, match="counts"):
        ptq.clip_ranges(counts[:46], ranges, "mse")


def _synthetic(row, lo=-1.0, hi=9.0):
    """47 tensors on the axis {lo, hi}, every one with the histogram `row`"""
    ranges = {t: (lo, hi) for t in hs.slots()}
    return np.tile(np.asarray(row, np.uint64), (47, 1)), ranges


def test_an_outlier_is_cut():
    """10^6 values spread evenly over the first tenth of 1000 bins and one value in the last bin, on {-1, 9}: edge[100] = 0.0.
    percentile 0.9999: tail = floor(0.00005 * 1000001) = 50; no leading bin holds <= 50 (10^4 each), the 900 empty bins and the outlier do."""
    row = np.zeros(1000, np.uint64)
    row[:100] = 10 ** 4
    row[-1] = 1
    counts, ranges = _synthetic(row)
    got = ptq.clip_ranges(counts, ranges, "percentile", 0.9999)
    assert got[51] == (-1.0, -1.0 + 100 * 10.0 / 1000) and got[100] == got[51]
    assert got[0] == (-1.0, 9.0)                                          # keep: the input is never clipped
    assert ptq.clip_ranges(counts, ranges, "percentile", 0.9999, keep=(0, 100))[100] == (-1.0, 9.0)
    assert ptq.clip_ranges(counts, ranges, "percentile", 0.9999, keep=())[0] == got[51]
    mse = ptq.clip_ranges(counts, ranges, "mse")
    assert mse[51][0] == -1.0 and mse[51][1] < 9.0 - 10.0 / 1000 + 1e-12 and mse[0] == (-1.0, 9.0)
    assert ptq.clip_error(row, -1.0, 9.0, *mse[51]) < ptq.clip_error(row, -1.0, 9.0, -1.0, 9.0)
    assert ptq.clip_ranges(counts, ranges, "mse", keep=(0, 51))[51] == (-1.0, 9.0)


def test_a_uniform_histogram_keeps_the_full_range_under_mse():
    counts, ranges = _synthetic(np.full(2048, 1000, np.uint64), -3.0, 5.0)
    assert ptq.clip_ranges(counts, ranges, "mse") == ranges
    counts, ranges = _synthetic(np.full(1, 7, np.uint64))                 # one bin: (0, 0) is the only candidate
    assert ptq.clip_ranges(counts, ranges, "mse") == ranges


def test_the_fallback_to_the_fullest_bin():
    """tail >= every cumulative count short of the whole: percentile 0 gives tail = total / 2, and with half the values in bin 2 and half in
    bin 5 of 8, a = 5 leading bins and b = 5 trailing bins hold <= tail: a + b >= bins."""
    row = np.array([0, 0, 50, 0, 0, 50, 0, 0], np.uint64)
    counts, ranges = _synthetic(row, 0.0, 8.0)
    got = ptq.clip_ranges(counts, ranges, "percentile", 0.0)
    assert got[51] == (2.0, 3.0)                                          # argmax takes the first of the two fullest bins
    empty, ranges = _synthetic(np.zeros(8, np.uint64), 0.0, 8.0)
    assert ptq.clip_ranges(empty, ranges, "percentile", 0.5) == ranges    # total 0: the range stays
    assert ptq.clip_ranges(empty, ranges, "mse") == ranges


@pytest.fixture(scope="module")
def clipped():
    ranges, counts = cs.host_result("yfw")[0], hs.host_counts(2048)
    return {"percentile": ptq.clip_ranges(counts, ranges, "percentile", 0.9999), "mse": ptq.clip_ranges(counts, ranges, "mse")}


def test_mse_never_models_more_error_than_minmax(clipped):
    ranges, counts = cs.host_result("yfw")[0], hs.host_counts(2048)
    assert clipped["mse"][0] == ranges[0] and clipped["percentile"][0] == ranges[0]
    moved = 0
    for i, t in enumerate(hs.slots()[1:], 1):
        lo, hi = ranges[t]
        new, old = ptq.clip_error(counts[i], lo, hi, *clipped["mse"][t]), ptq.clip_error(counts[i], lo, hi, lo, hi)
        assert new <= old, (t, new, old)
        assert lo <= clipped["mse"][t][0] <= clipped["mse"][t][1] <= hi and lo <= clipped["percentile"][t][0] <= clipped["percentile"][t][1] <= hi
        moved += clipped["mse"][t] != ranges[t]
    print(f"mse moved {moved} of 46 ranges; percentile 0.9999 moved {sum(clipped['percentile'][t] != ranges[t] for t in hs.slots())}")


@pytest.mark.parametrize("method", ["percentile", "mse"])
def test_the_model_of_every_method_is_admitted_by_the_library(hp, clipped, method):
    image = ptq.quantize_model(YFW, clipped[method])
    assert image != cs.host_model("yfw") and len(image) == len(cs.host_model("yfw"))
    assert model_file.write_yfm(model_file.load_yfm(image)) == image
    rc, text, mf = parse(hp, image)
    assert rc == 0, text
    T = model_file.load_yfm(image)["tensors"]
    assert (mf.out_scale_bits, mf.out_zero_point) == (int(cs.bits(T[100]["scale"])[0]), T[100]["zp"])
    assert (cs.bits(T[0]["scale"])[0], T[0]["zp"]) == (0x3B808081, -128)
    for rounding in ROUNDINGS:
        rc, tab, _ = prepare_model(hp, mf, rounding)
        assert rc == 0 and tab, (method, rounding)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_name_their_cause():
    x, ranges = cs.calib_frames()[:2], cs.host_result("yfw")[0]

    def refused(match, frames=x, r=ranges, bins=16):
        with pytest.raises(calib.CalibError, match=match):
            calib.host_histogram(YFW, frames, r, bins)

    refused(r"bins is 0, expected 1 to 4096", bins=0)
    refused(r"bins is 4097, expected 1 to 4096", bins=4097)
    refused(r"n is 0, expected at least 1", frames=np.zeros((0, 56, 56, 3), np.int8))
    refused(r"tensor 57: the range is \{-?nan, ", r={**ranges, 57: (float("nan"), 1.0)})
    refused(r"tensor 100: the range is \{.*, inf\}, expected two finite float32", r={**ranges, 100: (ranges[100][0], float("inf"))})
    refused(r"tensor 68: max -2 is below min 3", r={**ranges, 68: (3.0, -2.0)})
    with pytest.raises(ValueError, match="46 tensors"):
        calib.host_histogram(YFW, x, {t: v for t, v in ranges.items() if t != 74}, 16)
    lib = calib.load_host()
    import ctypes
    err = ctypes.create_string_buffer(400)
    mm = np.array([ranges[t] for t in hs.slots()], np.float32)
    counts = np.zeros((47, 16), np.uint64)
    for args, text in (((None, 2, mm.ctypes.data, 16, counts.ctypes.data), b"frames is NULL"),
                       ((x.ctypes.data, 2, None, 16, counts.ctypes.data), b"minmax is NULL"),
                       ((x.ctypes.data, 2, mm.ctypes.data, 16, None), b"counts is NULL")):
        assert lib.yf_calib_host_histogram(YFW, len(YFW), *args, 1, err, 400) <= 0 and text in err.value
    assert not counts.any()
