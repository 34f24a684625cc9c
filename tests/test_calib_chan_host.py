"""Per-channel sums of every convolution's raw output, on the CPU (libyf_calib_host.so: csrc/yf_calib_chan.h compiled for the host): bit for bit
against the plain restatement of calib_chan_support over calib_packs.evaluate's raw outputs, exact on planted biases, the head's sums against
the logits of the same call; bias correction (calib.correct_biases) through the channel_sums= injection against a bound that is derived,
not measured; ptq.with_biases; refusals.  No GPU."""
import numpy as np
import pytest

import calib_chan_support as ch
import calib_packs as cp
import calib_sim_support as ss
import calib_support as cs
from calib_support import calib, ptq, model_file

Y = "yfw"
# 8x8: 16 pixels in stage 0, a single partial chunk; 16x24: 96, one full chunk and a half one; 56x56: 784, twelve full chunks and 16
SIZES = ((8, 8), (16, 24), (56, 56))


def _tables():
    return [("all disabled", calib.empty_table()), ("all enabled", ss.shipped_table())]


@pytest.mark.parametrize("h,w", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
@pytest.mark.parametrize("what,table", _tables(), ids=[t[0] for t in _tables()])
def test_host_build_equals_the_restatement(h, w, what, table):
    pack, x = cp.pack("shipped_yfw"), cp.frames("shipped_yfw", h, w)
    want_rows, want_total = ch.restate(ch.raw_outputs(pack.convs, x, table))
    got_total, got_rows = calib.host_channel_sums(pack.yfw, x, table, threads=1, want_frames=True)
    ch.same_doubles(got_rows, want_rows, f"{what} at {h}x{w}: per-frame sums")
    ch.same_doubles(got_total, want_total, f"{what} at {h}x{w}: totals")
    many_total, many_rows = calib.host_channel_sums(pack.yfw, x, table, threads=16, want_frames=True)
    ch.same_doubles(many_rows, got_rows, "16 threads against one: per-frame sums")
    ch.same_doubles(many_total, got_total, "16 threads against one: totals")
    if (h, w) == (56, 56):                                               # the general entry at (56, 56) is the 56x56 entry
        ch.same_doubles(calib.host_channel_sums(pack.yfw, x, table, threads=2, general=True), got_total, "general=True at 56x56")
    assert np.isfinite(got_rows).all() and (got_rows != 0).any(axis=0).all()


def test_a_disabled_table_is_the_default_and_enabling_changes_the_sums():
    x, y = cp.frames("shipped_yfw", 16, 24), cs.yfw_bytes(Y)
    none = calib.host_channel_sums(y, x)
    ch.same_doubles(calib.host_channel_sums(y, x, calib.empty_table()), none, "table=None")
    full = calib.host_channel_sums(y, x, ss.shipped_table())
    first, cout = ch.layout()
    assert (full[first[1]:] != none[first[1]:]).any()
    # the value is the one BEFORE the convolution's own entry: quantising conv 0's output alone leaves conv 0's sums and moves conv 1's
    own = calib.host_channel_sums(y, x, ss.shipped_table([ch.conv_outputs()[0]]))
    ch.same_doubles(own[:cout[0]], none[:cout[0]], "conv 0 under its own entry")
    assert (own[first[1]:first[2]] != none[first[1]:first[2]]).any()


def test_layout_is_the_graphs():
    first, cout, pixels = calib.channel_layout()
    want_first, want_cout = ch.layout()
    g = model_file.load_graph()
    want_pixels = [int(np.prod(g["tensors"][t]["shape"][1:3])) for t in ch.conv_outputs()]
    assert list(first) == list(want_first) and list(cout) == list(want_cout) and list(pixels) == want_pixels
    assert int(first[-1] + cout[-1]) == calib.CHANNELS == 544
    assert calib.channel_pixels(160, 160)[0] == 6400 and calib.channel_pixels(56, 56)[-1] == 49


@pytest.mark.parametrize("k", ch.PLANTED)
def test_planted_biases_are_summed_exactly(k):
    y, _ = ch.planted(k)
    first, cout, pixels = calib.channel_layout()
    for h, w in ((56, 56), (16, 24)):
        x = cp.frames("shipped_yfw", h, w)
        n, p = x.shape[0], calib.elements_at(int(pixels[k]), h, w)
        for what, table in _tables():
            total, rows = calib.host_channel_sums(y, x, table, threads=2, want_frames=True)
            sl = slice(int(first[k]), int(first[k] + cout[k]))
            ch.same_doubles(total[sl], ch.planted_want(k, n, p), f"conv {k}, {what}, {h}x{w}: totals")
            for f in range(n):
                ch.same_doubles(rows[f, sl], ch.planted_want(k, 1, p), f"conv {k}, {what}, {h}x{w}: frame {f}")


def test_the_heads_sums_are_those_of_the_logits_the_call_returned():
    y, x = cs.yfw_bytes(Y), np.ascontiguousarray(ss.frames33()[:5])
    first, cout = ch.layout()
    but_head = ss.shipped_table([t for t in ss.ids() if t != 100])
    for what, table in (("all disabled", calib.empty_table()), ("all but the head's entry", but_head)):
        total, rows, logits = calib.host_channel_sums(y, x, table, threads=4, want_frames=True, logits=True)
        want_rows, want_total = ch.restate([np.zeros((5, 1, c), np.float32) for c in cout[:-1]] + [logits.reshape(5, 49, 18)])
        ch.same_doubles(rows[:, first[23]:], want_rows[:, first[23]:], f"{what}: conv 23 per frame")
        ch.same_doubles(total[first[23]:], want_total[first[23]:], f"{what}: conv 23 totals")
        ss.same_bits(logits, calib.host_simulate(y, x, table, threads=4)[0], f"{what}: logits against host_simulate")
    # under its own entry the logits are on the grid and the sums are not theirs
    total, logits = calib.host_channel_sums(y, x, ss.shipped_table(), logits=True)
    ss.same_bits(logits, calib.host_simulate(y, x, ss.shipped_table())[0], "all enabled: logits against host_simulate")


# ---------------------------------------------------------------------------------------------------------------- bias correction
@pytest.fixture(scope="module")
def corrected():
    """the shipped float weights, min/max ranges of the first 8 of frames33() -- the "before" condition holds on them, see the test --, and
    both modes' models"""
    y, x = cs.yfw_bytes(Y), np.ascontiguousarray(ss.frames33()[:8])
    r, _ = calib.host_run(y, x, threads=16)
    out = {mode: calib.correct_biases(y, r, x, mode=mode, channel_sums=ch.host_sums()) for mode in calib.BIAS_MODES}
    return y, x, r, out


def test_sequential_correction_leaves_every_channel_within_the_bias_grid(corrected):
    y, x, r, out = corrected
    before = ptq.quantize_model(y, r)
    bound = ch.bias_bound(before, r)
    gap_before = ch.mean_gap(y, before, x, ch.host_sums())
    print(f"before: {(gap_before > bound).sum()} of 544 channels above the bound, the worst at {(gap_before / bound).max():.1f} x")
    assert (gap_before > bound).any(), "the uncorrected model is within the bound already: the property below would be vacuous"
    image, report = out["sequential"]
    np.testing.assert_array_equal(ch.bias_bound(image, r), bound)        # the bias grid is the weights' and the ranges': the correction leaves it
    gap = ch.mean_gap(y, image, x, ch.host_sums())
    print(f"after:  the worst channel at {(gap / bound).max():.3f} x the bound")
    bad = np.argwhere(gap > bound).reshape(-1)
    assert not bad.size, f"{bad.size} channels above the bound, first {bad[0]}: {gap[bad[0]]!r} against {bound[bad[0]]!r}"
    assert [row["conv"] for row in report] == list(range(24)) and [row["tensor"] for row in report] == list(ch.conv_outputs())
    assert all(0 <= row["rms_err"] <= row["max_err"] and np.isfinite(row["max_err"]) for row in report) and max(row["max_err"] for row in report) > 0
    # the weights and every activation's quantisation are the uncorrected model's: biases alone moved
    a, b = model_file.load_yfm(before), model_file.load_yfm(image)
    moved = [i for i, (s, t) in enumerate(zip(a["tensors"], b["tensors"]))
             if s["zp"] != t["zp"] or not np.array_equal(s["scale"], t["scale"]) or not np.array_equal(s["data"], t["data"])]
    biases = sorted(a["ops"][d["op"]]["ins"][2] for d in model_file.graph_convs())
    assert moved and set(moved) <= set(biases) and all(np.array_equal(a["tensors"][i]["scale"], b["tensors"][i]["scale"]) for i in moved)


def test_once_corrects_the_first_convolution_within_the_bound(corrected):
    y, x, r, out = corrected
    image, report = out["once"]
    first, cout = ch.layout()
    bound, gap = ch.bias_bound(image, r), ch.mean_gap(y, image, x, ch.host_sums())
    assert (gap[:cout[0]] <= bound[:cout[0]]).all(), (gap[:cout[0]], bound[:cout[0]])
    assert len(report) == 24 and report[0] == out["sequential"][1][0]    # nothing earlier changes under conv 0: both modes measure it alike
    assert image != out["sequential"][0]
    with pytest.raises(ValueError, match="mode: 'twice', expected one of"):
        calib.correct_biases(y, r, x, mode="twice", channel_sums=ch.host_sums())


def test_with_biases_round_trip():
    y = cs.yfw_bytes(Y)
    convs = model_file.read_yfw(y)
    assert ptq.with_biases(y, [None] * 24) == y and ptq.with_biases(y, [b for _, b, _ in convs]) == y and ptq.with_biases(y, {}) == y
    new = [np.arange(b.size, dtype=np.float32) - 3 for _, b, _ in convs]
    back = model_file.read_yfw(ptq.with_biases(y, new))
    for c, ((w, b, dw), (w2, b2, dw2)) in enumerate(zip(convs, back)):
        assert np.array_equal(w, w2) and dw == dw2 and b2.dtype == np.float32 and np.array_equal(b2, new[c]), c
    one = model_file.read_yfw(ptq.with_biases(y, {5: new[5]}))
    assert np.array_equal(one[5][1], new[5]) and all(np.array_equal(one[c][1], convs[c][1]) for c in range(24) if c != 5)
    assert ptq.with_biases(ptq.with_biases(y, new), [b for _, b, _ in convs]) == y
    with pytest.raises(ValueError, match="conv 3: 17 values"):
        ptq.with_biases(y, {3: np.zeros(17, np.float32)})
    with pytest.raises(ValueError, match="conv 0: 8 values, not all finite"):
        ptq.with_biases(y, {0: np.full(8, np.nan, np.float32)})
    with pytest.raises(ValueError, match="23 items, expected one per convolution"):
        ptq.with_biases(y, [None] * 23)
    with pytest.raises(ValueError, match=r"convolutions \[24\]"):
        ptq.with_biases(y, {24: np.zeros(1, np.float32)})


def test_quantize_on_device_refuses_a_bad_mode_before_it_touches_a_gpu():
    with pytest.raises(ValueError, match="bias_correction: 'always', expected None or one of"):
        calib.quantize_on_device(cs.yfw_bytes(Y), np.zeros((1, 56, 56, 3), np.int8), bias_correction="always")


def test_refusals_of_the_host_entries():
    y, x = cs.yfw_bytes(Y), np.zeros((2, 8, 8, 3), np.int8)

    def bad(tensor, scale, zp):
        t = ss.shipped_table()
        t[ss.entry_of(tensor)] = (scale, zp)
        return t

    for table, text in ((bad(55, -0.5, 0), r"entry 5 \(tensor 55\): scale is -0.5"), (bad(100, np.nan, 0), r"entry 46 \(tensor 100\): scale is nan"),
                        (bad(58, 0.25, 128), r"entry 8 \(tensor 58\): zero_point is 128, expected -128 to 127"),
                        (bad(53, 1e-39, 0), r"entry 3 \(tensor 53\): scale is 1e-39, whose reciprocal is not a finite float32")):
        with pytest.raises(calib.CalibError, match="yf_calib_host_channel_sums: yf_calib_host_channel_sums: " + text):
            calib.host_channel_sums(y, x, table)
    with pytest.raises(calib.CalibError, match="n is 0, expected at least 1"):
        calib.host_channel_sums(y, x[:0])
    with pytest.raises(calib.CalibError, match=r"yf_calib_host_channel_sums: the frame size is h = 12, w = 8, expected multiples of 8 from 8 to 160"):
        calib.host_channel_sums(y, np.zeros((1, 12, 8, 3), np.int8))
    with pytest.raises(ValueError, match="table: shape"):
        calib.host_channel_sums(y, x, calib.empty_table()[:49])
    import ctypes
    lib, err = calib.load_host(), ctypes.create_string_buffer(400)
    rows, table = np.full((2, 544), 7.5), calib.empty_table()
    args = lambda frames, t, out: (bytes(y), len(y), 8, 8, frames, 2, t, out, None, None, 1, err, 400)
    for a, text in ((args(None, table.ctypes.data, rows.ctypes.data), "yf_calib_host_channel_sums: frames is NULL"),
                    (args(x.ctypes.data, None, rows.ctypes.data), "yf_calib_host_channel_sums: table is NULL"),
                    (args(x.ctypes.data, table.ctypes.data, None), "yf_calib_host_channel_sums: frame_sums is NULL")):
        assert lib.yf_calib_host_channel_sums_hw(*a) <= 0 and err.value.decode().startswith(text), err.value
    assert (rows == 7.5).all()
    assert lib.yf_calib_host_channel_sums_hw(b"YFW1", 4, 8, 8, x.ctypes.data, 2, table.ctypes.data, rows.ctypes.data, None, None, 1, err, 400) <= 0 and err.value
    assert lib.yf_calib_channel_layout(None, None, None) <= 0
