"""Calibration of a float model on the GPU: libyf_calib.so against its host build bit for bit (the same IEEE operations in the same order, and
minimum and maximum are exact), accumulation across calls, and the whole way from float weights to a model the int8 engine runs, on weights
the reference never quantised (the shipped .yfw, the ONNX export)."""
import importlib
import os

import numpy as np
import pytest

from conftest import GOLDEN
import calib_support as cs
import model_variants as mv
from calib_support import calib, ptq, model_file
from images_support import real_images

pytestmark = pytest.mark.gpu
REF = 0


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def cal(torch_cuda):
    c = calib.Calibration(cs.yfw_bytes("yfw"))
    yield c
    c.destroy()


def _same(got, want, what):
    ids_g, a = cs.ranges_array(got)
    ids_w, b = cs.ranges_array(want)
    assert ids_g == ids_w and len(ids_g) == 47
    bad = [(t, tuple(x), tuple(y)) for t, x, y in zip(ids_g, a, b) if not np.array_equal(x, y)]
    assert not bad, f"{what}: ranges differ from the host build's, first {bad[0]} ({len(bad)} tensors)"


def _same_logits(got, want, what):
    d = np.argwhere(cs.bits(got) != cs.bits(want))
    assert not d.shape[0], f"{what}: {d.shape[0]} logits differ, first at {tuple(d[0])}: {got[tuple(d[0])]!r} vs host {want[tuple(d[0])]!r}"


def _cases():
    x = cs.calib_frames()
    return [("n=1", x[:1]), ("n=3", x[:3]), ("27 real frames", x), ("structured extremes", mv.structured_extreme_frames()),
            ("257 random frames", np.random.default_rng(257).integers(-128, 128, (257, 56, 56, 3), dtype=np.int8))]


@pytest.mark.parametrize("what,frames", _cases(), ids=[c[0] for c in _cases()])
def test_ranges_and_logits_equal_the_host_build(cal, torch_cuda, what, frames):
    want_r, want_l = calib.host_run(cs.yfw_bytes("yfw"), frames, threads=16)
    cal.reset()
    d_x = torch_cuda.from_numpy(np.ascontiguousarray(frames)).cuda()
    assert cal.observe(d_x) == frames.shape[0] == cal.frames_observed
    _same(cal.ranges(), want_r, what)
    _same_logits(cal.logits.cpu().numpy(), want_l, what)


def test_the_other_weight_set_equals_the_host_build(torch_cuda):
    c = calib.Calibration(cs.yfw_bytes("npz"))
    try:
        c.observe(cs.calib_frames())
        _same(c.ranges(), cs.host_result("npz")[0], "npz weights")
        _same_logits(c.logits.cpu().numpy(), cs.host_result("npz")[1], "npz weights")
    finally:
        c.destroy()


def test_accumulation_reset_streams_and_no_logits(cal, torch_cuda):
    torch = torch_cuda
    want_r, want_l = cs.host_result("yfw")
    d_x = torch.from_numpy(np.ascontiguousarray(cs.calib_frames())).cuda()
    torch.cuda.synchronize()
    cal.reset()
    with pytest.raises(calib.CalibError, match="no frame has been observed yet"):
        cal.ranges()
    cal.observe(d_x[:13])
    first = cal.ranges()
    cal.observe(d_x[13:])
    _same(cal.ranges(), want_r, "[0:13] then [13:27]")
    _same_logits(cal.logits.cpu().numpy(), want_l[13:], "[13:27]")
    assert first == calib.host_run(cs.yfw_bytes("yfw"), cs.calib_frames()[:13])[0] and first != cal.ranges()
    cal.reset()
    assert cal.frames_observed == 0
    cal.observe(d_x[:1])
    _same(cal.ranges(), calib.host_run(cs.yfw_bytes("yfw"), cs.calib_frames()[:1])[0], "after reset")
    cal.reset()
    side = torch.cuda.Stream()
    cal.observe(d_x, stream=side.cuda_stream)
    _same(cal.ranges(), want_r, "a stream of its own")
    _same_logits(cal.logits.cpu().numpy(), want_l, "a stream of its own")
    cal.reset()
    cal.observe(d_x, logits=False)
    assert cal.logits is None
    _same(cal.ranges(), want_r, "NULL for the logits")
    with pytest.raises(ValueError):
        cal.observe(d_x.reshape(-1)[:100])


def test_refused_float_model_names_the_mismatch(torch_cuda):
    y = bytearray(cs.yfw_bytes("yfw"))
    y[8 + 16] = 1                                                    # conv 0: stride 2 -> 1
    with pytest.raises(calib.CalibError, match="conv 0: stride is 1, expected 2"):
        calib.Calibration(bytes(y))


# ---------------------------------------------------------------------------------------------------------------- end to end
def _lsb_errors(heads, logits, scale, zp):
    """|dequantised head - float logit| / output scale"""
    return np.abs((heads.astype(np.float64) - zp) * float(scale) - logits.astype(np.float64)) / float(scale)


@pytest.fixture(scope="module")
def new_model(network, torch_cuda, tmp_path_factory):
    """The session's network on the model quantize_on_device makes of the shipped .yfw and the 27 calibration frames; the module leaves the
    network as it found it (the shipped model, reference rounding)."""
    from oracle.oracle import Oracle
    torch = torch_cuda
    x = cs.calib_frames()
    d_x = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_out = torch.full((28, 7, 7, 18), 77, dtype=torch.int8, device="cuda")
    network.set_requant_rounding(REF)
    network.init()
    network.run_device(d_x.data_ptr(), d_out.data_ptr(), 27)
    torch.cuda.synchronize()
    shipped_heads = d_out.cpu().numpy()[:27]
    image = calib.quantize_on_device(cs.yfw_bytes("yfw"), d_x)
    path = str(tmp_path_factory.mktemp("calib") / "calibrated.yfm")
    open(path, "wb").write(image)
    network.init_model(image)
    try:
        yield dict(image=image, oracle=Oracle(path), x=x, d_x=d_x, shipped_heads=shipped_heads)
    finally:
        network.set_requant_rounding(REF)
        network.init()


def test_float_weights_to_a_running_int8_model(network, new_model, torch_cuda):
    """quantize_on_device(shipped .yfw, 27 frames) is the host build's model byte for byte; yf_network_init_model admits it; the engine's
    heads equal the oracle's on the same bytes; and its quantisation error against the float logits, in units of the output scale, is at most
    twice the shipped pair's (the shipped .yfm on the engine against the host build on the weights it was quantised from) in median and 99th
    percentile -- the weights and the output scale differ, nothing finer can be derived."""
    torch = torch_cuda
    assert new_model["image"] == cs.host_model("yfw")
    T = model_file.load_yfm(new_model["image"])["tensors"]
    scale, zp = T[100]["scale"][0], T[100]["zp"]
    assert (int(cs.bits(scale)), zp) != (0x3e11987e, -15)
    d_out = torch.full((28, 7, 7, 18), 77, dtype=torch.int8, device="cuda")
    network.run_device(new_model["d_x"].data_ptr(), d_out.data_ptr(), 27)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert (got[27] == 77).all()
    ref = new_model["oracle"].run(new_model["x"], threads=16)
    d = mv.first_difference(got[:27].reshape(27, -1), ref.reshape(27, -1), (7, 7, 18))
    assert d is None, f"head differs first at (frame, y, x, channel) = {d[:4]}: got {d[4]}, oracle {d[5]}"
    assert not np.array_equal(ref, new_model["shipped_heads"])
    S = model_file.load_yfm(cs.SHIPPED_YFM)["tensors"][100]
    shipped = _lsb_errors(new_model["shipped_heads"], cs.host_result("npz")[1], S["scale"][0], S["zp"])
    new = _lsb_errors(got[:27], cs.host_result("yfw")[1], scale, zp)
    fig = {k: (float(np.median(e)), float(np.percentile(e, 99)), float(e.max())) for k, e in (("shipped", shipped), ("new", new))}
    sat = {k: int(((h == -128) | (h == 127)).sum()) for k, h in (("shipped", new_model["shipped_heads"]), ("new", got[:27]))}
    for k in fig:
        print(f"{k} pair: median {fig[k][0]:.3f} LSB, p99 {fig[k][1]:.3f} LSB, max {fig[k][2]:.3f} LSB, saturated head bytes {sat[k]}")
    assert fig["new"][0] <= 2 * fig["shipped"][0] and fig["new"][1] <= 2 * fig["shipped"][1], fig


def test_detect_decodes_with_the_new_output_quantisation(yf, network, new_model, torch_cuda):
    """images.detect on the new model: the records of the oracle on the same bytes under the tables yf_network_decode_tables reports, which are
    the tables of the new output quantisation (interpreter.model_decode_tables, the mirror of csrc/yf_model_file.c's builder)."""
    from test_model_file_gpu import _detect_reference
    images = importlib.import_module("stm32h7-yolo_amd.images")
    interp = importlib.import_module("stm32h7-yolo_amd.interpreter")
    T = model_file.load_yfm(new_model["image"])["tensors"]
    sig, ex, ident = network.decode_tables()
    want_sig, want_ex = interp.model_decode_tables(T[100]["scale"][0], T[100]["zp"])
    assert np.array_equal(cs.bits(sig), cs.bits(want_sig)) and np.array_equal(cs.bits(ex), cs.bits(want_ex))
    shipped = np.fromfile(os.path.join(GOLDEN, "decode_tables_f32.bin"), "<u4").reshape(2, 256)
    assert not np.array_equal(cs.bits(sig), shipped[0])
    orc = new_model["oracle"]
    orc.sig, orc.ex = sig, ex
    imgs = real_images(ptq)[:6]
    got = [b.tolist() for b in images.detect(network, imgs)]
    want = _detect_reference(ptq, orc, imgs, 56)
    assert got == want
    n = sum(len(b) for b in want)
    print(f"detect on the calibrated model: {n} boxes on {len(imgs)} images")
    assert n > 0
