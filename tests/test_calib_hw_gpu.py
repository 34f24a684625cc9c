"""Calibration at h x w on the GPU: the general kernels of libyf_calib.so (the arena in global memory) against the LDS kernels at 56x56 and
against the host build at 8x8, 16x24, 24x8 and 160x160, bit for bit -- ranges, logits, histogram counts, comparison records and totals --;
slabs reused by every workgroup, accumulation across sizes, two streams on one handle, and the way from 160x160 device frames to a model
the int8 engine runs at 160x160."""
import numpy as np
import pytest

import calib_support as cs
import calib_hist_support as hs
import calib_hw_support as hw
import model_variants as mv
import quant_support as qs
from calib_support import calib, ptq, model_file

pytestmark = pytest.mark.gpu
REF = 0
YFW = "yfw"


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def cal(torch_cuda):
    c = calib.Calibration(cs.yfw_bytes(YFW))
    yield c
    c.destroy()


def _same(got, want, what):
    ids_g, a = cs.ranges_array(got)
    ids_w, b = cs.ranges_array(want)
    assert ids_g == ids_w and len(ids_g) == 47
    bad = [(t, tuple(x), tuple(y)) for t, x, y in zip(ids_g, a, b) if not np.array_equal(cs.bits(x), cs.bits(y))]
    assert not bad, f"{what}: ranges differ, first {bad[0]} ({len(bad)} tensors)"


def _same_logits(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    d = np.argwhere(cs.bits(got) != cs.bits(want))
    assert not d.shape[0], f"{what}: {d.shape[0]} logits differ, first at {tuple(d[0])}: {got[tuple(d[0])]!r} vs {want[tuple(d[0])]!r}"


def _device_entries(torch, entries):
    """host entries (q: int8 numpy [n, stride]) -> the same entries over device copies"""
    return [e._replace(q=torch.from_numpy(np.ascontiguousarray(e.q)).cuda()) for e in entries]


def _all_entries(h, w, n, seed):
    """an entry for each of the 46 tensors at h x w over random int8 values, each with a scale and zero point of its own"""
    rng = np.random.default_rng(seed)
    return [calib.Entry(t, np.float32(0.01 * (1 + i % 7)), int(i % 5) - 2, rng.integers(-128, 128, (n, e), dtype=np.int8), e)
            for i, (t, e) in enumerate(zip(hs.slots()[1:], hw.elements(h, w)[1:]))]


# ------------------------------------------------------------------------------------------------- the general form against the LDS form
def test_general_form_at_56_equals_the_lds_form(cal, torch_cuda):
    torch = torch_cuda
    x = cs.calib_frames()
    d_x = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    cal.reset()
    cal.observe(d_x)
    lds_r, lds_l = cal.ranges(), cal.logits.cpu().numpy()
    cal.reset()
    assert cal.observe(d_x, general=True) == 27 == cal.frames_observed
    _same(cal.ranges(), lds_r, "general against LDS")
    _same_logits(cal.logits.cpu().numpy(), lds_l, "general against LDS")
    _same(lds_r, cs.host_result(YFW)[0], "LDS against host")
    for bins in (16, 2048):
        a = cal.histogram(d_x, lds_r, bins).cpu().numpy()
        b = cal.histogram(d_x, lds_r, bins, general=True).cpu().numpy()
        hs.assert_same(b, a, f"{bins} bins, general against LDS")
        hs.assert_conserved(b, 27, f"{bins} bins")
    entries = _device_entries(torch, qs.entries_over(qs.oracle_q(*qs.real_run())))
    s1, t1 = cal.compare(d_x, entries)
    s2, t2 = cal.compare(d_x, entries, general=True)
    qs.same_records(calib.frame_stats_array(s2), calib.frame_stats_array(s1), "records, general against LDS")
    qs.same_records(t2, t1, "totals, general against LDS")
    assert cal.scratch_bytes >= cal.workgroups(56, 56) * 39200 * 4


# ------------------------------------------------------------------------------------------------- the device against the host build
def _cases():
    return [("8x8 n=5", 8, 8, 5), ("16x24 n=3", 16, 24, 3), ("24x8 n=3", 24, 8, 3), ("160x160 n=2", 160, 160, 2), ("8x8 every slab twice", 8, 8, None)]


@pytest.mark.parametrize("what,h,w,n", _cases(), ids=[c[0] for c in _cases()])
def test_device_equals_the_host_build(cal, torch_cuda, what, h, w, n):
    torch = torch_cuda
    y = cs.yfw_bytes(YFW)
    groups = cal.workgroups(h, w)
    assert groups >= 1
    if n is None:
        n = 2 * groups + 3                                               # every workgroup takes a second frame into its slab, three a third
        x = np.random.default_rng(groups).integers(-128, 128, (n, h, w, 3), dtype=np.int8)
    else:
        x = hw.frames(h, w, n)
    want_r, want_l = calib.host_run(y, x, threads=16)
    d_x = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    # observe, through the library itself: the logits buffer has one frame more than n, whose sentinel must survive
    cells = hw.cells(h, w)
    d_l = torch.full((n + 1, h // 8, w // 8, 18), -7.5, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    cal.reset()
    rc = cal._lib.yf_calib_observe_hw_device(cal.handle, h, w, d_x.data_ptr(), n, d_l.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == n, cal._text()
    assert cal.frames_observed == n
    _same(cal.ranges(), want_r, what)
    got_l = d_l.cpu().numpy()
    assert got_l[n].size == cells * 18 and (got_l[n] == -7.5).all(), "the frame behind the logits was written"
    _same_logits(got_l[:n], want_l, what)
    # the Python way gives the same, and a smaller size after a larger one allocates nothing
    before = cal.scratch_bytes
    assert before >= groups * 800 * cells * 4
    cal.reset()
    cal.observe(d_x)
    _same(cal.ranges(), want_r, what)
    _same_logits(cal.logits.cpu().numpy(), want_l, what)
    assert cal.scratch_bytes == before
    # histograms
    for bins in (16, 4096):
        want = calib.host_histogram(y, x, want_r, bins, threads=16)
        got = cal.histogram(d_x, want_r, bins).cpu().numpy()
        hs.assert_same(got, want, f"{what}, {bins} bins")
    # comparison of all 46 tensors
    entries = _all_entries(h, w, n, seed=h * w + n)
    want_s, want_t = calib.host_compare(y, x, entries, threads=16)
    got_s, got_t = cal.compare(d_x, _device_entries(torch, entries))
    qs.same_records(calib.frame_stats_array(got_s), want_s, f"{what}: records")
    qs.same_records(got_t, want_t, f"{what}: totals")


def test_refused_sizes_launch_nothing(cal, torch_cuda):
    torch = torch_cuda
    d_x = torch.zeros(160 * 160 * 3, dtype=torch.int8, device="cuda")
    d_l = torch.full((400 * 18,), -7.5, dtype=torch.float32, device="cuda")
    counts = torch.zeros((47, 16), dtype=torch.int64, device="cuda").view(torch.uint64)
    d_stats = torch.zeros(64, dtype=torch.uint8, device="cuda")
    mm = np.ascontiguousarray([cs.host_result(YFW)[0][t] for t in hs.slots()], np.float32)
    entries = calib._qtensors([calib.Entry(100, 1.0, 0, d_x, 7200)])
    torch.cuda.synchronize()
    cal.reset()
    s, lib = torch.cuda.current_stream().cuda_stream, cal._lib
    for h, w in ((0, 56), (4, 8), (60, 56), (56, 60), (168, 160), (160, 168), (-8, 8), (8, -8)):
        rule = f"h = {h}, w = {w}, expected multiples of 8 from 8 to 160"
        assert lib.yf_calib_observe_hw_device(cal.handle, h, w, d_x.data_ptr(), 1, d_l.data_ptr(), s) <= 0 and rule in cal._text(), cal._text()
        assert lib.yf_calib_histogram_hw_device(cal.handle, h, w, d_x.data_ptr(), 1, mm.ctypes.data, 16, counts.data_ptr(), s) <= 0 and rule in cal._text()
        assert lib.yf_calib_compare_hw_device(cal.handle, h, w, d_x.data_ptr(), 1, entries, 1, d_stats.data_ptr(), None, s) <= 0 and rule in cal._text()
        assert lib.yf_calib_workgroups(cal.handle, h, w) <= 0 and rule in cal._text()
    assert lib.yf_calib_observe_hw_device(cal.handle, 8, 8, d_x.data_ptr(), 0, d_l.data_ptr(), s) <= 0 and "n is 0, expected at least 1" in cal._text()
    torch.cuda.synchronize()
    assert cal.frames_observed == 0 and (d_l.cpu().numpy() == -7.5).all() and not counts.cpu().numpy().any() and not d_stats.cpu().numpy().any()
    with pytest.raises(calib.CalibError, match="h = 12, w = 8, expected multiples of 8 from 8 to 160"):
        cal.observe(torch.zeros((1, 12, 8, 3), dtype=torch.int8, device="cuda"))


def test_ranges_accumulate_across_sizes(cal, torch_cuda):
    y = cs.yfw_bytes(YFW)
    x160 = hw.frames(160, 160, 2)
    r56, r160 = cs.host_result(YFW)[0], calib.host_run(y, x160, threads=16)[0]
    cal.reset()
    cal.observe(cs.calib_frames())                                       # the LDS form
    cal.observe(x160)                                                    # the general form, on the same stream
    assert cal.frames_observed == 27 + 2
    _same(cal.ranges(), hw.union(r56, r160), "56x56 then 160x160")
    assert cal.ranges() != r56 and cal.ranges() != r160
    assert cal.logits.shape == (2, 20, 20, 18)


def test_two_streams_share_the_slabs_in_order(cal, torch_cuda):
    """Three general launches at 160x160 of two frames each -- every one uses slabs 0 and 1 -- issued back to back on two streams with no
    event between them from the caller: the handle's own event orders them."""
    torch = torch_cuda
    y = cs.yfw_bytes(YFW)
    x = hw.frames(160, 160, 4)
    a, b = x[:2], x[2:]
    ra, la = calib.host_run(y, a, threads=16)
    want_b = calib.host_histogram(y, b, ra, 64, threads=16)
    want_a = calib.host_histogram(y, a, ra, 64, threads=16)
    d_a, d_b = (torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (a, b))
    counts_a, counts_b = (torch.zeros((47, 64), dtype=torch.int64, device="cuda").view(torch.uint64) for _ in range(2))
    cal.reset()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    cal.observe(d_a, stream=s1.cuda_stream)
    cal.histogram(d_b, ra, 64, counts=counts_b, stream=s2.cuda_stream)
    cal.histogram(d_a, ra, 64, counts=counts_a, stream=s1.cuda_stream)
    logits = cal.logits
    torch.cuda.synchronize()
    _same(cal.ranges(), ra, "observe on the first stream")
    _same_logits(logits.cpu().numpy(), la, "observe on the first stream")
    hs.assert_same(counts_b.cpu().numpy(), want_b, "histogram on the second stream")
    hs.assert_same(counts_a.cpu().numpy(), want_a, "histogram on the first stream again")


# ---------------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def model160(network, torch_cuda, tmp_path_factory):
    """The session's network on the model quantize_on_device makes of the npz weights and the 27 upscaled frames at 160x160; the module leaves
    the network as it found it (the shipped model, reference rounding)."""
    from oracle.oracle import Oracle
    torch = torch_cuda
    x = hw.frames160()
    d_x = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_out = torch.full((28, 20, 20, 18), 77, dtype=torch.int8, device="cuda")
    network.set_requant_rounding(REF)
    network.init()
    network.run_device_hw(160, 160, d_x.data_ptr(), d_out.data_ptr(), 27)
    torch.cuda.synchronize()
    shipped_heads = d_out.cpu().numpy()[:27]
    image = calib.quantize_on_device(cs.yfw_bytes("npz"), d_x)
    path = str(tmp_path_factory.mktemp("calib160") / "calibrated160.yfm")
    open(path, "wb").write(image)
    network.init_model(image)
    try:
        yield dict(image=image, oracle=Oracle(path), x=x, d_x=d_x, shipped_heads=shipped_heads)
    finally:
        network.set_requant_rounding(REF)
        network.init()


def test_160_frames_to_a_model_running_at_160(network, model160, torch_cuda):
    """quantize_on_device of [27, 160, 160, 3] device frames is the host pipeline's model byte for byte (min/max and mse); the engine admits
    it and its 160x160 heads equal the oracle's on the same bytes; against the float logits its error in LSB is at most twice the shipped
    model's on the same frames, median and 99th percentile.  (Upscaled frames, min/max ranges: see test_calib_hw_host.py.)"""
    torch = torch_cuda
    y, x = cs.yfw_bytes("npz"), model160["x"]
    r160, logits = calib.host_run(y, x, threads=16)
    assert model160["image"] == ptq.quantize_model(y, r160)
    counts = calib.host_histogram(y, x, r160, 2048, threads=16)
    assert calib.quantize_on_device(y, model160["d_x"], ranges="mse") == ptq.quantize_model(y, ptq.clip_ranges(counts, r160, "mse", 0.9999, (0,)))
    T = model_file.load_yfm(model160["image"])["tensors"]
    scale, zp = T[100]["scale"][0], T[100]["zp"]
    d_out = torch.full((28, 20, 20, 18), 77, dtype=torch.int8, device="cuda")
    network.run_device_hw(160, 160, model160["d_x"].data_ptr(), d_out.data_ptr(), 27)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert (got[27] == 77).all()
    ref = model160["oracle"].run(x, threads=16)
    d = mv.first_difference(got[:27].reshape(27, -1), ref.reshape(27, -1), (20, 20, 18))
    assert d is None, f"head differs first at (frame, y, x, channel) = {d[:4]}: got {d[4]}, oracle {d[5]}"
    assert not np.array_equal(ref, model160["shipped_heads"])
    S = model_file.load_yfm(cs.SHIPPED_YFM)["tensors"][100]
    shipped = hw.lsb_errors(model160["shipped_heads"], logits, S["scale"][0], S["zp"])
    new = hw.lsb_errors(got[:27], logits, scale, zp)
    fig = {k: (float(np.median(e)), float(np.percentile(e, 99))) for k, e in (("shipped", shipped), ("new", new))}
    for k in fig:
        print(f"{k} model at 160x160: median {fig[k][0]:.3f} LSB, p99 {fig[k][1]:.3f} LSB")
    assert fig["new"][0] <= 2 * fig["shipped"][0] and fig["new"][1] <= 2 * fig["shipped"][1], fig


def test_the_report_at_160_is_the_head_row_of_the_host_comparison(network, model160, torch_cuda):
    """calib.quantisation_report on [n, 160, 160, 3] frames: one row, tensor 100, whose figures are those of the host build's comparison of
    the engine's own heads with the float32 evaluation -- the engine has no per-stage dump at 160x160, so the head is what there is."""
    torch = torch_cuda
    y, n = cs.yfw_bytes("npz"), 3
    x = model160["x"][:n]
    rows = calib.quantisation_report(network, y, model160["image"], x)
    assert [r["tensor"] for r in rows] == [100] and rows[0]["elements"] == n * 7200
    d_out = torch.full((n + 1, 7200), 77, dtype=torch.int8, device="cuda")
    network.run_device_hw(160, 160, model160["d_x"].data_ptr(), d_out.data_ptr(), n)
    torch.cuda.synchronize()
    heads = d_out.cpu().numpy()
    assert (heads[n] == 77).all()
    head = [t for t in calib.report_tensors(network.dump_offset, model160["image"]) if t["offset"] is None]
    _, totals = calib.host_compare(y, x, [calib.Entry(100, head[0]["scale"], head[0]["zero_point"], np.ascontiguousarray(heads[:n]), 7200)], threads=16)
    assert rows == calib.report_rows(head, totals)
    assert calib.quantisation_report(network, y, model160["image"], torch.from_numpy(np.ascontiguousarray(x)).cuda()) == rows
