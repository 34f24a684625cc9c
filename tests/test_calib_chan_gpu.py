"""Per-channel sums of every convolution's raw output on the GPU: yfc_channel_sums_kernel (the arena in LDS) and yfc_channel_sums_hw_kernel
(the arena in global memory) against the host build, bit for bit -- per-frame sums, totals, logits --; planted biases, exactly; two streams
on one handle; a second call overwrites; refusals; and the layers on top (calib.correct_biases, quantize_on_device(bias_correction=...))
against the same computed through host_channel_sums."""
import numpy as np
import pytest

import calib_chan_support as ch
import calib_hw_support as hw
import calib_sim_support as ss
import calib_support as cs
from calib_support import calib, ptq

pytestmark = pytest.mark.gpu
REF = 0
Y = "yfw"


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def cal(torch_cuda):
    c = calib.Calibration(cs.yfw_bytes(Y))
    yield c
    c.destroy()


def _against_host(cal, torch, x, table, what, general=False, yfw=None):
    """device == host build for one table on frames x; returns the device's (totals, per-frame sums, logits) as numpy"""
    y = cs.yfw_bytes(Y) if yfw is None else yfw
    want_t, want_r, want_l = calib.host_channel_sums(y, x, table, threads=16, general=general, want_frames=True, logits=True)
    d_x = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    got_t, d_r, d_l = cal.channel_sums(d_x, table, general=general, want_frames=True, logits=True)
    got_r, got_l = d_r.cpu().numpy(), d_l.cpu().numpy()
    ch.same_doubles(got_r, want_r, f"{what}: per-frame sums")
    ch.same_doubles(got_t, want_t, f"{what}: totals")
    ss.same_bits(got_l, want_l, f"{what}: logits")
    ss.same_bits(cal.simulate(d_x, table, general=general)[0].cpu().numpy(), got_l, f"{what}: logits against simulate")
    ch.same_doubles(cal.channel_sums(d_x, table, general=general), got_t, f"{what}: totals alone")
    return got_t, got_r, got_l


def _lds_tables():
    return [("all disabled", calib.empty_table()), ("all enabled", ss.shipped_table()), ("conv slot 51, in front of a LeakyReLU", ss.shipped_table([51]))]


@pytest.mark.parametrize("what,table", _lds_tables(), ids=[t[0] for t in _lds_tables()])
def test_lds_form_equals_the_host_build(cal, torch_cuda, what, table):
    x = ss.frames33()
    totals, rows, logits = _against_host(cal, torch_cuda, x, table, what)
    assert rows.shape == (33, calib.CHANNELS) and np.isfinite(rows).all()
    if what == "all disabled":
        cal.reset()
        cal.observe(torch_cuda.from_numpy(np.ascontiguousarray(x)).cuda())
        ss.same_bits(logits, cal.logits.cpu().numpy(), "all disabled: logits against observe")
        ch.same_doubles(cal.channel_sums(x), totals, "table=None, numpy frames")
        assert cal.frames_observed == 33
        cal.reset()


def _hw_cases():
    return [("8x8 n=5", 8, 8, 5), ("16x24 n=3", 16, 24, 3), ("24x8 n=3", 24, 8, 3), ("56x56 n=33", 56, 56, 33), ("160x160 n=2", 160, 160, 2),
            ("8x8 more frames than workgroups", 8, 8, None)]


@pytest.mark.parametrize("what,h,w,n", _hw_cases(), ids=[c[0] for c in _hw_cases()])
def test_general_form_equals_the_host_build(cal, torch_cuda, what, h, w, n):
    groups = cal.workgroups(h, w)
    if n is None:
        n = groups + 3                                                   # the grid-stride path: three slabs and their LDS scratch are used a second time
        x = np.random.default_rng(groups).integers(-128, 128, (n, h, w, 3), dtype=np.int8)
    else:
        x = ss.frames33() if (h, w) == (56, 56) else hw.frames(h, w, n)
    table = ss.shipped_table()
    totals, rows, logits = _against_host(cal, torch_cuda, x, table, what, general=True)
    assert rows.shape == (n, calib.CHANNELS) and logits.shape == (n, h // 8, w // 8, 18) and np.isfinite(rows).all()
    assert cal.scratch_bytes >= groups * 800 * hw.cells(h, w) * 4
    if (h, w) == (56, 56):                                               # ... and the LDS form gives the general form's bits
        t, d_r, d_l = cal.channel_sums(x, table, want_frames=True, logits=True)
        ch.same_doubles(d_r.cpu().numpy(), rows, "per-frame sums, LDS form against the general form")
        ch.same_doubles(t, totals, "totals, LDS form against the general form")
        ss.same_bits(d_l.cpu().numpy(), logits, "logits, LDS form against the general form")
    if (h, w) == (160, 160):                                             # 6400 pixels are exactly 100 chunks: the scratch's maximum
        assert calib.channel_pixels(h, w)[0] == 6400
        _against_host(cal, torch_cuda, x, calib.empty_table(), what + ", all disabled", general=True)


@pytest.mark.parametrize("k", ch.PLANTED)
def test_planted_biases_are_summed_exactly_on_the_device(torch_cuda, k):
    y, _ = ch.planted(k)
    first, cout, pixels = calib.channel_layout()
    sl = slice(int(first[k]), int(first[k] + cout[k]))
    c = calib.Calibration(y)
    try:
        for h, w, general in ((56, 56, False), (56, 56, True), (16, 24, True)):
            x = hw.frames(h, w, 5)
            p = calib.elements_at(int(pixels[k]), h, w)
            for what, table in (("all disabled", calib.empty_table()), ("all enabled", ss.shipped_table())):
                totals, d_r = c.channel_sums(x, table, general=general, want_frames=True)
                rows = d_r.cpu().numpy()
                ch.same_doubles(totals[sl], ch.planted_want(k, 5, p), f"conv {k}, {what}, {h}x{w}, general={general}: totals")
                for f in range(5):
                    ch.same_doubles(rows[f, sl], ch.planted_want(k, 1, p), f"conv {k}, {what}, {h}x{w}, general={general}: frame {f}")
    finally:
        c.destroy()


def test_two_streams_share_the_slabs_in_order(cal, torch_cuda):
    """Two general launches at 160x160 of two frames each -- both use slabs 0 and 1 -- issued back to back on two streams with no event
    between them from the caller: the handle's own event orders them, and each gives what it gives alone."""
    torch = torch_cuda
    x = hw.frames(160, 160, 4)
    ta, tb = ss.shipped_table(), calib.empty_table()
    d_a, d_b = (torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (x[:2], x[2:]))
    one_a = cal.channel_sums(d_a, ta, want_frames=True, logits=True)
    one_b = cal.channel_sums(d_b, tb, want_frames=True, logits=True)
    rows = [torch.full((2, calib.CHANNELS), -7.5, dtype=torch.float64, device="cuda") for _ in range(2)]
    sums = [torch.full((calib.CHANNELS,), -7.5, dtype=torch.float64, device="cuda") for _ in range(2)]
    out = [torch.full((2, 20, 20, 18), -7.5, dtype=torch.float32, device="cuda") for _ in range(2)]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    lib = cal._lib
    rc1 = lib.yf_calib_channel_sums_hw_device(cal.handle, 160, 160, d_a.data_ptr(), 2, ta.ctypes.data, rows[0].data_ptr(), sums[0].data_ptr(),
                                              out[0].data_ptr(), s1.cuda_stream)
    rc2 = lib.yf_calib_channel_sums_hw_device(cal.handle, 160, 160, d_b.data_ptr(), 2, tb.ctypes.data, rows[1].data_ptr(), sums[1].data_ptr(),
                                              out[1].data_ptr(), s2.cuda_stream)
    assert rc1 == 2 and rc2 == 2, cal._text()
    torch.cuda.synchronize()
    for i, (one, name) in enumerate(((one_a, "first stream"), (one_b, "second stream"))):
        ch.same_doubles(sums[i].cpu().numpy(), one[0], f"{name}: totals")
        ch.same_doubles(rows[i].cpu().numpy(), one[1].cpu().numpy(), f"{name}: per-frame sums")
        ss.same_bits(out[i].cpu().numpy(), one[2].cpu().numpy(), f"{name}: logits")
    assert not np.array_equal(one_a[0], one_b[0])


def test_a_second_call_overwrites(cal, torch_cuda):
    torch = torch_cuda
    x = ss.frames33()
    d_a, d_b = (torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (x[:4], x[4:8]))
    table = ss.shipped_table()
    want = calib.host_channel_sums(cs.yfw_bytes(Y), x[4:8], table, threads=4, want_frames=True)
    rows = torch.full((4, calib.CHANNELS), 1e300, dtype=torch.float64, device="cuda")
    sums = torch.full((calib.CHANNELS,), 1e300, dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    for general in (False, True):
        for d_x in (d_a, d_b):
            tail = (d_x.data_ptr(), 4, table.ctypes.data, rows.data_ptr(), sums.data_ptr(), None, s)
            rc = cal._lib.yf_calib_channel_sums_hw_device(cal.handle, 56, 56, *tail) if general else cal._lib.yf_calib_channel_sums_device(cal.handle, *tail)
            assert rc == 4, cal._text()
        torch.cuda.synchronize()
        ch.same_doubles(rows.cpu().numpy(), want[1], f"general={general}: per-frame sums of the second call")
        ch.same_doubles(sums.cpu().numpy(), want[0], f"general={general}: totals of the second call")


def test_refusals_launch_nothing(cal, torch_cuda):
    torch = torch_cuda
    d_x = torch.zeros((2, 56, 56, 3), dtype=torch.int8, device="cuda")
    d_r = torch.full((2, calib.CHANNELS), -7.5, dtype=torch.float64, device="cuda")
    d_t = torch.full((calib.CHANNELS,), -7.5, dtype=torch.float64, device="cuda")
    d_l = torch.full((2, 882), -7.5, dtype=torch.float32, device="cuda")
    ok = ss.shipped_table()

    def bad(tensor, scale, zp):
        t = ok.copy()
        t[ss.entry_of(tensor)] = (scale, zp)
        return t

    torch.cuda.synchronize()
    cal.reset()
    s, lib, h = torch.cuda.current_stream().cuda_stream, cal._lib, cal.handle
    X, R, T, L = d_x.data_ptr(), d_r.data_ptr(), d_t.data_ptr(), d_l.data_ptr()
    tables = [bad(55, -0.5, 0), bad(100, np.nan, 0), bad(102, np.inf, 0), bad(58, 0.25, 128), bad(58, 0.25, -129), bad(53, 1e-39, 0)]      # (kept alive: the calls take addresses)
    K = ok.ctypes.data
    cases = [
        ((h, X, 2, tables[0].ctypes.data, R, T, L, s), "entry 5 (tensor 55): scale is -0.5"),
        ((h, X, 2, tables[1].ctypes.data, R, T, L, s), "entry 46 (tensor 100): scale is nan"),
        ((h, X, 2, tables[2].ctypes.data, R, T, L, s), "entry 48 (tensor 102): scale is inf"),
        ((h, X, 2, tables[3].ctypes.data, R, T, L, s), "entry 8 (tensor 58): zero_point is 128, expected -128 to 127"),
        ((h, X, 2, tables[4].ctypes.data, R, T, L, s), "entry 8 (tensor 58): zero_point is -129, expected -128 to 127"),
        ((h, X, 2, tables[5].ctypes.data, R, T, L, s), "entry 3 (tensor 53): scale is 1e-39, whose reciprocal is not a finite float32"),
        ((h, X, 0, K, R, T, L, s), "n is 0, expected at least 1"),
        ((h, X, -3, K, R, T, L, s), "n is -3, expected at least 1"),
        ((None, X, 2, K, R, T, L, s), "NULL handle"),
        ((h, None, 2, K, R, T, L, s), "frames is NULL"),
        ((h, X, 2, None, R, T, L, s), "table is NULL"),
        ((h, X, 2, K, None, T, L, s), "frame_sums is NULL"),
    ]
    for args, text in cases:
        assert lib.yf_calib_channel_sums_device(*args) <= 0 and text in cal._text(), (text, cal._text())
        assert cal._text().startswith("yf_calib_channel_sums_device: ")
        assert lib.yf_calib_channel_sums_hw_device(args[0], 56, 56, *args[1:]) <= 0 and text in cal._text(), (text, cal._text())
        assert cal._text().startswith("yf_calib_channel_sums_hw_device: ")
    for hh, ww in ((12, 8), (8, 168), (0, 56)):
        assert lib.yf_calib_channel_sums_hw_device(h, hh, ww, X, 1, K, R, T, L, s) <= 0
        assert f"yf_calib_channel_sums_hw_device: the frame size is h = {hh}, w = {ww}, expected multiples of 8 from 8 to 160" in cal._text()
    torch.cuda.synchronize()
    assert (d_r.cpu().numpy() == -7.5).all() and (d_t.cpu().numpy() == -7.5).all() and (d_l.cpu().numpy() == -7.5).all() and cal.frames_observed == 0
    with pytest.raises(calib.CalibError, match=r"entry 5 \(tensor 55\): scale is -0.5"):
        cal.channel_sums(d_x, bad(55, -0.5, 0))
    with pytest.raises(calib.CalibError, match="no frame has been observed yet"):
        cal.ranges()


@pytest.mark.parametrize("mode", calib.BIAS_MODES)
def test_bias_correction_on_the_device_is_the_host_paths_model(torch_cuda, mode):
    y, x = cs.yfw_bytes(Y), np.ascontiguousarray(ss.frames33()[:8])
    r, _ = calib.host_run(y, x, threads=16)
    want, want_report = calib.correct_biases(y, r, x, mode=mode, channel_sums=ch.host_sums())
    got, report = calib.correct_biases(y, r, torch_cuda.from_numpy(x).cuda(), mode=mode)
    assert got == want and report == want_report
    assert got != ptq.quantize_model(y, r)


def test_quantize_on_device_without_the_argument_is_unchanged(torch_cuda):
    y, x = cs.yfw_bytes(Y), cs.calib_frames()[:9]
    d_x = torch_cuda.from_numpy(np.ascontiguousarray(x)).cuda()
    c = calib.Calibration(y)
    try:
        c.observe(d_x, logits=False)
        by_hand = ptq.quantize_model(y, c.ranges())
    finally:
        c.destroy()
    assert calib.quantize_on_device(y, d_x) == by_hand == calib.quantize_on_device(y, d_x, bias_correction=None)
    with pytest.raises(ValueError, match="bias_correction: 'twice', expected None or one of"):
        calib.quantize_on_device(y, d_x, bias_correction="twice")


def test_quantize_on_device_with_bias_correction_makes_a_model_the_engine_runs(network, torch_cuda):
    """The corrected model is admitted by the engine and is correct_biases' of the min/max ranges; its heads and the head's mean_error on the
    27 calibration frames are finite.  Whether it is better is profiles/bias_correction.txt's to say, not this test's."""
    torch = torch_cuda
    y, x = cs.yfw_bytes(Y), cs.calib_frames()
    d_x = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    image = calib.quantize_on_device(y, d_x, bias_correction="sequential")
    r, _ = calib.host_run(y, x, threads=16)
    plain = ptq.quantize_model(y, r)
    assert image != plain and len(image) == len(plain)
    try:
        network.init_model(image)
        rows = calib.quantisation_report(network, y, image, d_x)
        network.init_model(plain)
        before = calib.quantisation_report(network, y, plain, d_x)
    finally:
        network.set_requant_rounding(REF)
        network.init()
    (head,), (head_before,) = ([row for row in t if row["tensor"] == 100] for t in (rows, before))
    assert head["elements"] == 27 * 882 and len(rows) == len(before)
    print(f"head: mean_error {head_before['mean_error']:+.5f} -> {head['mean_error']:+.5f}, SQNR {head_before['sqnr_db']:.2f} -> {head['sqnr_db']:.2f} dB")
    assert np.isfinite(head["mean_error"]) and np.isfinite(head["sqnr_db"]) and np.isfinite(head["max_abs_error"])
    assert all(np.isfinite(row["mean_error"]) for row in rows)
