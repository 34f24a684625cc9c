"""Simulated quantisation on the GPU: yfc_simulate_kernel (the arena in LDS) and yfc_simulate_hw_kernel (the arena in global memory) against
the host build, bit for bit -- logits, per-frame records, totals --; all disabled against observe; two streams on one handle; refusals; and
the layers on top (calib.sensitivity, quantize_on_device(ranges="head")) against the same computed through host_simulate."""
import numpy as np
import pytest

import calib_support as cs
import calib_hw_support as hw
import calib_sim_support as ss
import quant_support as qs
from calib_support import calib, ptq, model_file

pytestmark = pytest.mark.gpu
REF = 0
Y = "yfw"                             # the shipped .yfw: what the device-equals-host cases run on
PAIR = ss.WEIGHTS                     # the float weights the shipped .yfm came from: the sensitivity table of the shipped pair


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


def _against_host(cal, torch, x, table, what, general=False):
    """device == host build for one table on frames x; returns the device's (logits, records, totals)"""
    y = cs.yfw_bytes(Y)
    want_ref, want_l, want_t, want_s = ss.host_all(y, x, table, general=general)
    d_x = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_ref, none = cal.simulate(d_x, calib.empty_table(), general=general)
    assert none is None
    ss.same_bits(d_ref.cpu().numpy(), want_ref, f"{what}: reference logits")
    d_l, got_t, d_s = cal.simulate(d_x, table, d_ref, general=general, want_stats=True)
    got_l, got_s = d_l.cpu().numpy(), calib.frame_stats_array(d_s).reshape(-1)
    ss.same_bits(got_l, want_l, f"{what}: logits")
    qs.same_records(got_s, want_s, f"{what}: records")
    qs.same_records(got_t, want_t, f"{what}: totals")
    # logits alone, and the record without the logits: the same bits
    ss.same_bits(cal.simulate(d_x, table, general=general)[0].cpu().numpy(), want_l, f"{what}: logits, no reference")
    return got_l, got_s, got_t


def _lds_tables():
    return [("all disabled", calib.empty_table()), ("all enabled", ss.shipped_table()), ("the input alone", ss.shipped_table([0])),
            ("conv slot 51", ss.shipped_table([51])), ("LeakyReLU slot 52", ss.shipped_table([52])), ("ADD slot 68", ss.shipped_table([68])),
            ("pool slot 58", ss.shipped_table([58])), ("QUANTIZE 101", ss.shipped_table([101])), ("QUANTIZE 102", ss.shipped_table([102])),
            ("QUANTIZE 103", ss.shipped_table([103])), ("the head alone, clipped", ss.one_entry(100, np.float32(0.004), 17)),
            ("the input on a coarse grid", ss.one_entry(0, np.float32(0.05), -100))]


@pytest.mark.parametrize("what,table", _lds_tables(), ids=[t[0] for t in _lds_tables()])
def test_lds_form_equals_the_host_build(cal, torch_cuda, what, table):
    x = ss.frames33()
    _, stats, totals = _against_host(cal, torch_cuda, x, table, what)
    if what == "all disabled":
        assert not totals[0]["sum_sq_err"] and not totals[0]["saturated"]
    else:
        assert totals[0]["sum_sq_err"] > 0
    if "clipped" in what or "all enabled" in what:
        assert totals[0]["saturated"] > 0 and stats["saturated"].sum() == totals[0]["saturated"]


def _hw_cases():
    return [("8x8 n=5", 8, 8, 5), ("16x24 n=3", 16, 24, 3), ("24x8 n=3", 24, 8, 3), ("56x56 n=33", 56, 56, 33), ("160x160 n=2", 160, 160, 2),
            ("8x8 more frames than workgroups", 8, 8, None)]


@pytest.mark.parametrize("what,h,w,n", _hw_cases(), ids=[c[0] for c in _hw_cases()])
def test_general_form_equals_the_host_build(cal, torch_cuda, what, h, w, n):
    groups = cal.workgroups(h, w)
    if n is None:
        n = groups + 3                                                   # the grid-stride path: three slabs are used a second time
        x = np.random.default_rng(groups).integers(-128, 128, (n, h, w, 3), dtype=np.int8)
    else:
        x = ss.frames33() if (h, w) == (56, 56) else hw.frames(h, w, n)
    table = ss.shipped_table()
    got_l, got_s, got_t = _against_host(cal, torch_cuda, x, table, what, general=True)
    assert got_l.shape == (n, h // 8, w // 8, 18) and got_t[0]["elements"] == n * hw.cells(h, w) * 18 and got_t[0]["sum_sq_err"] > 0
    assert cal.scratch_bytes >= groups * 800 * hw.cells(h, w) * 4
    if (h, w) == (56, 56):                                               # ... and the LDS form gives the general form's bits
        d_x = torch_cuda.from_numpy(np.ascontiguousarray(x)).cuda()
        d_ref = cal.simulate(d_x, calib.empty_table())[0]
        d_l, t, d_s = cal.simulate(d_x, table, d_ref, want_stats=True)
        ss.same_bits(d_l.cpu().numpy(), got_l, "LDS form against the general form")
        qs.same_records(calib.frame_stats_array(d_s).reshape(-1), got_s, "records, LDS form against the general form")
        qs.same_records(t, got_t, "totals, LDS form against the general form")


def test_all_disabled_equals_observe_and_touches_no_ranges(cal, torch_cuda):
    torch = torch_cuda
    d_x = torch.from_numpy(np.ascontiguousarray(ss.frames33())).cuda()
    cal.reset()
    cal.observe(d_x)
    want, ranges, seen = cal.logits.cpu().numpy(), cal.ranges(), cal.frames_observed
    for general in (False, True):
        ss.same_bits(cal.simulate(d_x, calib.empty_table(), general=general)[0].cpu().numpy(), want, f"all disabled, general={general}")
        cal.simulate(d_x, ss.shipped_table(), torch.from_numpy(want).cuda(), general=general)
    assert cal.frames_observed == seen == 33 and cal.ranges() == ranges
    cal.reset()
    cal.simulate(d_x, ss.shipped_table())
    assert cal.frames_observed == 0
    with pytest.raises(calib.CalibError, match="no frame has been observed yet"):
        cal.ranges()


def test_two_streams_share_the_slabs_in_order(cal, torch_cuda):
    """Two general simulate launches at 160x160 of two frames each -- both use slabs 0 and 1 -- issued back to back on two streams with no
    event between them from the caller: the handle's own event orders them, and each gives what it gives alone."""
    torch = torch_cuda
    x = hw.frames(160, 160, 4)
    a, b = x[:2], x[2:]
    ta, tb = ss.shipped_table(), ss.shipped_table([51, 52, 100])
    d_a, d_b = (torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (a, b))
    ref_a, ref_b = cal.simulate(d_a, calib.empty_table())[0], cal.simulate(d_b, calib.empty_table())[0]
    one_a, tot_a = cal.simulate(d_a, ta, ref_a)
    one_b, tot_b = cal.simulate(d_b, tb, ref_b)
    out = [torch.full((2, 20, 20, 18), -7.5, dtype=torch.float32, device="cuda") for _ in range(2)]
    stats = [torch.zeros((2, 32), dtype=torch.uint8, device="cuda") for _ in range(2)]
    totals = [torch.zeros((1, 48), dtype=torch.uint8, device="cuda") for _ in range(2)]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    lib = cal._lib
    rc1 = lib.yf_calib_simulate_hw_device(cal.handle, 160, 160, d_a.data_ptr(), 2, ta.ctypes.data, ref_a.data_ptr(), out[0].data_ptr(), stats[0].data_ptr(),
                                          totals[0].data_ptr(), s1.cuda_stream)
    rc2 = lib.yf_calib_simulate_hw_device(cal.handle, 160, 160, d_b.data_ptr(), 2, tb.ctypes.data, ref_b.data_ptr(), out[1].data_ptr(), stats[1].data_ptr(),
                                          totals[1].data_ptr(), s2.cuda_stream)
    assert rc1 == 2 and rc2 == 2, cal._text()
    torch.cuda.synchronize()
    ss.same_bits(out[0].cpu().numpy(), one_a.cpu().numpy(), "first stream")
    ss.same_bits(out[1].cpu().numpy(), one_b.cpu().numpy(), "second stream")
    qs.same_records(totals[0].cpu().numpy().view(calib.TOTALS).reshape(1), tot_a, "totals, first stream")
    qs.same_records(totals[1].cpu().numpy().view(calib.TOTALS).reshape(1), tot_b, "totals, second stream")
    assert not np.array_equal(one_a.cpu().numpy(), ref_a.cpu().numpy())


def test_refusals_launch_nothing(cal, torch_cuda):
    torch = torch_cuda
    d_x = torch.zeros((2, 56, 56, 3), dtype=torch.int8, device="cuda")
    d_ref = torch.zeros((2, 882), dtype=torch.float32, device="cuda")
    d_l = torch.full((2, 882), -7.5, dtype=torch.float32, device="cuda")
    d_s = torch.full((2, 32), 0x5A, dtype=torch.uint8, device="cuda")
    d_t = torch.full((48,), 0x5A, dtype=torch.uint8, device="cuda")
    ok = ss.shipped_table()

    def bad(tensor, scale, zp):
        t = ok.copy()
        t[ss.entry_of(tensor)] = (scale, zp)
        return t

    torch.cuda.synchronize()
    cal.reset()
    s, lib, h = torch.cuda.current_stream().cuda_stream, cal._lib, cal.handle
    X, R, L, S, T = d_x.data_ptr(), d_ref.data_ptr(), d_l.data_ptr(), d_s.data_ptr(), d_t.data_ptr()
    tables = [bad(55, -0.5, 0), bad(100, np.nan, 0), bad(102, np.inf, 0), bad(58, 0.25, 128), bad(58, 0.25, -129), bad(53, 1e-39, 0)]      # (kept alive: the calls take addresses)
    K = ok.ctypes.data
    cases = [
        ((h, X, 2, tables[0].ctypes.data, R, L, S, T, s), "entry 5 (tensor 55): scale is -0.5"),
        ((h, X, 2, tables[1].ctypes.data, R, L, S, T, s), "entry 46 (tensor 100): scale is nan"),
        ((h, X, 2, tables[2].ctypes.data, R, L, S, T, s), "entry 48 (tensor 102): scale is inf"),
        ((h, X, 2, tables[3].ctypes.data, R, L, S, T, s), "entry 8 (tensor 58): zero_point is 128, expected -128 to 127"),
        ((h, X, 2, tables[4].ctypes.data, R, L, S, T, s), "entry 8 (tensor 58): zero_point is -129, expected -128 to 127"),
        ((h, X, 0, K, R, L, S, T, s), "n is 0, expected at least 1"),
        ((None, X, 2, K, R, L, S, T, s), "NULL handle"),
        ((h, None, 2, K, R, L, S, T, s), "frames is NULL"),
        ((h, X, 2, None, R, L, S, T, s), "table is NULL"),
        ((h, X, 2, K, None, L, S, None, s), "frame_stats given without ref_logits"),
        ((h, X, 2, K, None, L, None, T, s), "totals given without ref_logits"),
        ((h, X, 2, K, R, L, None, None, s), "ref_logits given without frame_stats"),
        ((h, X, 2, K, R, L, None, T, s), "ref_logits given without frame_stats"),
        ((h, X, 2, tables[5].ctypes.data, R, L, S, T, s), "entry 3 (tensor 53): scale is 1e-39, whose reciprocal is not a finite float32"),
    ]
    for args, text in cases:
        assert lib.yf_calib_simulate_device(*args) <= 0 and text in cal._text(), (text, cal._text())
        assert cal._text().startswith("yf_calib_simulate_device: ")
        assert lib.yf_calib_simulate_hw_device(args[0], 56, 56, *args[1:]) <= 0 and text in cal._text(), (text, cal._text())
        assert cal._text().startswith("yf_calib_simulate_hw_device: ")
    for hh, ww in ((12, 8), (8, 168), (0, 56)):
        assert lib.yf_calib_simulate_hw_device(h, hh, ww, X, 1, K, R, L, S, T, s) <= 0
        assert f"yf_calib_simulate_hw_device: the frame size is h = {hh}, w = {ww}, expected multiples of 8 from 8 to 160" in cal._text()
    torch.cuda.synchronize()
    assert (d_l.cpu().numpy() == -7.5).all() and (d_s.cpu().numpy() == 0x5A).all() and (d_t.cpu().numpy() == 0x5A).all() and cal.frames_observed == 0
    with pytest.raises(calib.CalibError, match=r"entry 5 \(tensor 55\): scale is -0.5"):
        cal.simulate(d_x, bad(55, -0.5, 0))


@pytest.mark.parametrize("what,h,w,n", [("56x56, the 27 frames", 56, 56, 27), ("16x16, 4 frames", 16, 16, 4)], ids=["56x56", "16x16"])
def test_sensitivity_on_the_device_is_the_host_table(torch_cuda, what, h, w, n):
    y, m = cs.yfw_bytes(PAIR), qs.shipped_yfm()
    x = cs.calib_frames() if (h, w) == (56, 56) else hw.frames(h, w, n)
    want = calib.sensitivity(y, m, x, simulate=lambda yy, xx, t, ref: calib.host_simulate(yy, xx, t, ref, threads=16))
    got = calib.sensitivity(y, m, torch_cuda.from_numpy(np.ascontiguousarray(x)).cuda())
    assert len(got) == 77 and [r["name"] for r in got] == [r["name"] for r in want]
    bad = [(a, b) for a, b in zip(got, want) if a != b]
    assert not bad, f"{what}: {len(bad)} rows differ, first {bad[0]}"
    assert got[-2]["sqnr_db"] > got[-1]["sqnr_db"] > 0
    if (h, w) == (16, 16):
        assert calib.sensitivity(y, m, x) == want                        # numpy frames are uploaded


def test_head_ranges_on_the_device_make_the_host_paths_model(network, torch_cuda):
    """quantize_on_device(ranges="head"): the engine admits the model, and it is the model the host path's choices give on the same frames"""
    torch = torch_cuda
    y, x = cs.yfw_bytes(Y), cs.calib_frames()[:9]
    image = calib.quantize_on_device(y, torch.from_numpy(np.ascontiguousarray(x)).cuda(), ranges="head")
    r, _ = calib.host_run(y, x, threads=16)
    counts = calib.host_histogram(y, x, r, 2048, threads=16)
    cands = calib.range_candidates(counts, r, 0.9999, (0,))
    chosen = calib.head_ranges(cands, lambda t, ref: calib.host_simulate(y, x, t, ref, threads=16), (0,))
    assert image == ptq.quantize_model(y, chosen)
    picked = [[c == chosen[t] for c in cands[t]].index(True) for t in sorted(cands)]
    print("candidates chosen (0 minmax, 1 percentile, 2 mse):", picked)
    assert chosen[0] == cands[0][0] and len(picked) == 47
    try:
        network.init_model(image)
    finally:
        network.set_requant_rounding(REF)
        network.init()
    with pytest.raises(ValueError, match="ranges: 'tail', expected one of"):
        calib.quantize_on_device(y, torch.zeros((1, 56, 56, 3), dtype=torch.int8, device="cuda"), ranges="tail")
