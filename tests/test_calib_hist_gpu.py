"""Histogram calibration on the GPU: yf_calib_histogram_device against its host build count for count (integer sums are exact, so nothing
is a tolerance), on axes wider and narrower than the data, accumulated across calls and streams; the refusals, with nothing launched; and
quantize_on_device with clipped ranges, byte for byte against the host and bit-exact on the engine against the oracle."""
import functools

import numpy as np
import pytest

import calib_support as cs
import calib_hist_support as hs
import model_variants as mv
from calib_support import calib, ptq

pytestmark = pytest.mark.gpu
YFW = cs.yfw_bytes("yfw")
REF = 0


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def cal(torch_cuda):
    c = calib.Calibration(YFW)
    yield c
    c.destroy()


@functools.lru_cache(maxsize=None)
def _frames():
    x = cs.calib_frames()
    return {"n=1": x[:1], "n=3": x[:3], "27 real frames": x, "structured extremes": mv.structured_extreme_frames(),
            "257 random frames": np.random.default_rng(257).integers(-128, 128, (257, 56, 56, 3), dtype=np.int8)}


_RANGES = {}


def _ranges(name):
    """the host build's ranges of a frame set, once per process"""
    if name not in _RANGES:
        _RANGES[name] = calib.host_run(YFW, _frames()[name], threads=16, want_logits=False)[0]
    return _RANGES[name]


def _cases():
    return [(name, bins) for name in _frames() for bins in (2048, 16)] + [("n=3", 1), ("n=3", 4096)]


@pytest.mark.parametrize("name,bins", _cases(), ids=[f"{n}, {b} bins" for n, b in _cases()])
def test_counts_equal_the_host_build(cal, torch_cuda, name, bins):
    frames, ranges = _frames()[name], _ranges(name)
    want = calib.host_histogram(YFW, frames, ranges, bins, threads=16)
    got = cal.histogram(torch_cuda.from_numpy(np.ascontiguousarray(frames)).cuda(), ranges, bins)
    assert got.dtype == torch_cuda.uint64 and tuple(got.shape) == (47, bins) and got.is_cuda
    got = got.cpu().numpy()
    hs.assert_same(got, want, f"{name}, {bins} bins")
    hs.assert_conserved(got, frames.shape[0], f"{name}, {bins} bins")


def test_axes_narrower_than_the_data(cal, torch_cuda):
    """The axes of frame 0's ranges under all 27 frames: what lies outside is counted in the end bins."""
    x = cs.calib_frames()
    narrow = _ranges("n=1")
    got = cal.histogram(x, narrow, 2048).cpu().numpy()
    hs.assert_same(got, calib.host_histogram(YFW, x, narrow, 2048, threads=16), "narrow axes")
    hs.assert_conserved(got, 27, "narrow axes")
    below = above = 0
    for i, (t, v) in enumerate(zip(hs.slots(), hs.float_tensors(x))):
        lo, hi = np.float32(narrow[t][0]), np.float32(narrow[t][1])
        assert got[i, 0] >= (v < lo).sum() and got[i, -1] >= (v > hi).sum(), t
        below, above = below + int((v < lo).sum()), above + int((v > hi).sum())
    print(f"values of the 27 frames outside frame 0's ranges: {below} below, {above} above")
    assert below > 0 and above > 0


def test_accumulation_streams_and_the_handle_is_untouched(cal, torch_cuda):
    torch = torch_cuda
    ranges, want = cs.host_result("yfw")[0], hs.host_counts(2048)
    d_x = torch.from_numpy(np.ascontiguousarray(cs.calib_frames())).cuda()
    cal.reset()
    cal.observe(d_x[:5])
    before = (cal.ranges(), cal.frames_observed)
    counts = cal.histogram(d_x[:13], ranges, 2048)
    assert cal.histogram(d_x[13:], ranges, 2048, counts=counts) is counts
    hs.assert_same(counts.cpu().numpy(), want, "[0:13] then [13:27]")
    side = torch.cuda.Stream()
    counts = cal.histogram(d_x[:13], ranges, 2048, stream=side.cuda_stream)
    cal.histogram(d_x[13:], ranges, 2048, counts=counts, stream=side.cuda_stream)
    side.synchronize()
    hs.assert_same(counts.cpu().numpy(), want, "[0:13] then [13:27] on a side stream")
    assert (cal.ranges(), cal.frames_observed) == before and cal.frames_observed == 5
    hs.assert_same(cal.histogram(d_x[:5], None, 16).cpu().numpy(), calib.host_histogram(YFW, cs.calib_frames()[:5], before[0], 16), "ranges=None")
    with pytest.raises(ValueError, match="counts"):
        cal.histogram(d_x, ranges, 16, counts=counts)


def test_a_side_stream_waits_for_the_upload_and_the_zeroing(cal, torch_cuda):
    """Frames given as a numpy array are uploaded, and new counts zeroed, on torch's current stream; the launch on a side stream is ordered
    behind both on the device.  So is a second call that takes the counts of a call on the current stream to a side stream."""
    torch = torch_cuda
    ranges, want = cs.host_result("yfw")[0], hs.host_counts(16)
    side = torch.cuda.Stream()
    counts = cal.histogram(cs.calib_frames(), ranges, 16, stream=side.cuda_stream)
    side.synchronize()
    hs.assert_same(counts.cpu().numpy(), want, "numpy frames on a side stream")
    counts = cal.histogram(cs.calib_frames()[:13], ranges, 16)
    cal.histogram(cs.calib_frames()[13:], ranges, 16, counts=counts, stream=side.cuda_stream)
    side.synchronize()
    hs.assert_same(counts.cpu().numpy(), want, "current stream, then a side stream")


def test_refusals_launch_nothing(cal, torch_cuda):
    torch = torch_cuda
    ranges = cs.host_result("yfw")[0]
    d_x = torch.from_numpy(np.ascontiguousarray(cs.calib_frames()[:2])).cuda()
    counts = torch.zeros((47, 16), dtype=torch.int64, device="cuda").view(torch.uint64)
    torch.cuda.synchronize()

    def refused(match, frames=d_x, r=ranges, bins=16, c=counts):
        with pytest.raises(calib.CalibError, match=match):
            cal.histogram(frames, r, bins, counts=c)

    refused(r"bins is 0, expected 1 to 4096", bins=0, c=None)
    refused(r"bins is 4097, expected 1 to 4096", bins=4097, c=None)
    refused(r"n is 0, expected at least 1", frames=d_x[:0])
    refused(r"tensor 57: the range is \{-?nan, ", r={**ranges, 57: (float("nan"), 1.0)})
    refused(r"tensor 100: the range is \{.*, inf\}, expected two finite float32", r={**ranges, 100: (ranges[100][0], float("inf"))})
    refused(r"tensor 68: max -2 is below min 3", r={**ranges, 68: (3.0, -2.0)})
    lib, mm = cal._lib, np.array([ranges[t] for t in hs.slots()], np.float32)
    s = torch.cuda.current_stream().cuda_stream
    for args, text in (((None, d_x.data_ptr(), 2, mm.ctypes.data, 16, counts.data_ptr(), s), "NULL handle"),
                       ((cal.handle, None, 2, mm.ctypes.data, 16, counts.data_ptr(), s), "frames is NULL"),
                       ((cal.handle, d_x.data_ptr(), 2, None, 16, counts.data_ptr(), s), "minmax is NULL"),
                       ((cal.handle, d_x.data_ptr(), 2, mm.ctypes.data, 16, None, s), "counts is NULL")):
        assert lib.yf_calib_histogram_device(*args) <= 0 and text in cal._text(), (text, cal._text())
    torch.cuda.synchronize()
    assert not counts.cpu().numpy().any()


# ---------------------------------------------------------------------------------------------------------------- end to end
def test_minmax_is_still_the_host_model(torch_cuda):
    d_x = torch_cuda.from_numpy(np.ascontiguousarray(cs.calib_frames())).cuda()
    assert calib.quantize_on_device(YFW, d_x, ranges="minmax") == cs.host_model("yfw") == calib.quantize_on_device(YFW, d_x)
    with pytest.raises(ValueError, match="ranges"):
        calib.quantize_on_device(YFW, d_x, ranges="entropy")


@pytest.mark.parametrize("method", ["percentile", "mse"])
def test_clipped_model_end_to_end(network, torch_cuda, tmp_path, method):
    """quantize_on_device(ranges=method) is ptq.quantize_model of ptq.clip_ranges over the HOST build's ranges and histogram, byte for byte;
    the engine initialised from it runs the 27 frames bit-exact against the oracle loaded with the same bytes."""
    from oracle.oracle import Oracle
    torch = torch_cuda
    x = cs.calib_frames()
    d_x = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    image = calib.quantize_on_device(YFW, d_x, ranges=method, percentile=0.9999)
    want = ptq.quantize_model(YFW, ptq.clip_ranges(hs.host_counts(2048), cs.host_result("yfw")[0], method, 0.9999))
    assert image == want and image != cs.host_model("yfw")
    path = str(tmp_path / f"{method}.yfm")
    open(path, "wb").write(image)
    d_out = torch.full((28, 7, 7, 18), 77, dtype=torch.int8, device="cuda")
    network.set_requant_rounding(REF)
    network.init_model(image)
    try:
        network.run_device(d_x.data_ptr(), d_out.data_ptr(), 27)
        torch.cuda.synchronize()
    finally:
        network.init()
    got = d_out.cpu().numpy()
    assert (got[27] == 77).all()
    ref = Oracle(path).run(x, threads=16)
    d = mv.first_difference(got[:27].reshape(27, -1), ref.reshape(27, -1), (7, 7, 18))
    assert d is None, f"{method}: head differs first at (frame, y, x, channel) = {d[:4]}: got {d[4]}, oracle {d[5]}"
