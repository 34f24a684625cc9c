"""Calibration of a float model on the CPU: the host build of the calibration arithmetic (libyf_calib_host.so: csrc/yf_calib_arith.h, the
.yfw parser) against the float64 restatement, ptq.quantize_model against the shipped int8 model, the written .yfm through the library's own
parser and table builder, the refusals, and the parser alone under ASan + UBSan.  No GPU."""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import calib_support as cs
from calib_support import calib, ptq, model_file
from test_model_file_host import hp, parse, prepare_model, ROUNDINGS      # noqa: F401  (hp is a fixture)
from test_ptq import RESIDUAL

PKG = os.path.join(ROOT, "stm32h7-yolo_amd")
CONV, DWCONV, MAXPOOL, PAD, LEAKY, ADD, QUANTIZE, CONCAT = 3, 4, 17, 34, 98, 0, 114, 2

# float32 (the defined order) against float64 (oracle/np_restatement.py, NpModel.run_float) on the 27 calibration frames, measured here:
#   the largest |fp32 - f64| of a range end over the tensor's largest magnitude:  4.87e-7 (npz weights), 6.42e-7 (shipped .yfw)
#     (relative to max(|min|, |max|) of the tensor, not to the range end itself: an end enters ptq.activation_qparams through
#     scale = (max - min) / 255 and zero point = round(-128 - min / scale) of the range widened to hold zero, so what an error in it costs
#     is measured against the width of that range, which is at least the magnitude; the relative error of a minimum near zero beside a wide
#     maximum means nothing to the quantisation)
#   the largest |fp32 - f64| of a logit over the largest |logit|:                  4.89e-7 (npz weights), 7.41e-7 (shipped .yfw)
# The bound is four times the largest of them (other frames excite other sums); profiles/calib_accuracy.txt records the same figures.
MEASURED_REL = 7.42e-7
REL_BOUND = 4 * MEASURED_REL


@pytest.fixture(scope="module")
def restated():
    """name -> (float64 ranges of every op output and the input, float64 logits [27, 7, 7, 18])"""
    from oracle.np_restatement import NpModel
    npm = NpModel(cs.SHIPPED_YFM)
    out = {}
    for name in cs.WEIGHT_SETS:
        convs = [(w, b) for w, b, _ in model_file.read_yfw(cs.yfw_bytes(name))]
        cal = ptq.Calibrator()
        logits = np.stack([npm.run_float(x, float_convs=convs, observe=cal.observe) for x in cs.calib_frames()])
        out[name] = (cal.ranges, logits)
    return out


@pytest.mark.parametrize("name", cs.WEIGHT_SETS)
def test_float32_evaluation_against_the_float64_restatement(restated, name):
    want_r, want_l = restated[name]
    got_r, got_l = cs.host_result(name)
    assert len(got_r) == calib.N_RANGES == 47 and set(got_r) <= set(want_r)
    worst = 0.0
    for t, (lo, hi) in got_r.items():
        a, b = want_r[t]
        mag = max(abs(a), abs(b))
        worst = max(worst, abs(lo - a) / mag, abs(hi - b) / mag)
    worst_l = float(np.abs(got_l - want_l).max() / np.abs(want_l).max())
    print(f"{name}: range ends {worst:.3e}, logits {worst_l:.3e} (bound {REL_BOUND:.3e})")
    assert worst <= REL_BOUND and worst_l <= REL_BOUND
    assert got_r[0] == (0.0, 1.0)                                    # the frames hold black and white pixels


def test_threads_do_not_change_the_host_build():
    r1, l1 = cs.host_result("yfw")
    r4, l4 = calib.host_run(cs.yfw_bytes("yfw"), cs.calib_frames(), threads=4)
    assert r1 == r4 and np.array_equal(cs.bits(l1), cs.bits(l4))


def test_yfw_reader_and_writer_are_inverses():
    for name in cs.WEIGHT_SETS:
        b = cs.yfw_bytes(name)
        assert model_file.write_yfw(model_file.read_yfw(b)) == b
    from oracle.np_fp32 import load_yfw
    mine = model_file.read_yfw(cs.yfw_bytes("yfw"))
    for (w, b, dw), c in zip(mine, load_yfw(os.path.join(PKG, "model", "yoloface_fp32.yfw"))):
        assert dw == c["dw"] and np.array_equal(w.reshape(-1), c["w"].reshape(-1)) and np.array_equal(b, c["b"])
    with pytest.raises(ValueError, match="conv 3"):
        model_file.write_yfw([(w, b, dw) if k != 3 else (w[:-1], b, dw) for k, (w, b, dw) in enumerate(cs.npz_convs())])


def test_quantised_float_model_is_the_shipped_int8_model():
    """quantize_model(the float weights the shipped model came from, float32 ranges of the host build) against oracle/model/yoloface_int8.yfm:
    graph, weights, filter scales and zero points equal; activation scales to 1e-6 except the four residual tensors of tests/test_ptq.py,
    which stay inside that test's bounds; biases are quantize_bias of the scales they were given.  No zero point flips against the float64
    calibration: FLIPPED stays empty."""
    FLIPPED = {}                                                     # tensor -> fractional part of -128 - min / scale that caused it
    got, want = model_file.load_yfm(cs.host_model("npz")), model_file.load_yfm(cs.SHIPPED_YFM)
    assert got["ops"] == want["ops"] and (got["input"], got["output"]) == (want["input"], want["output"])
    assert len(got["tensors"]) == len(want["tensors"]) == 104
    assert len(cs.host_model("npz")) == os.path.getsize(cs.SHIPPED_YFM)
    n_w = n_s = n_zp = n_b = 0
    for i, (a, b) in enumerate(zip(got["tensors"], want["tensors"])):
        assert (a["shape"], a["type"], len(a["scale"]), a["data"] is None) == (b["shape"], b["type"], len(b["scale"]), b["data"] is None), i
        if len(a["scale"]) == 1:
            if i not in FLIPPED:
                assert a["zp"] == b["zp"], (i, a["zp"], b["zp"])
            n_zp += 1
            rel = abs(float(a["scale"][0]) - float(b["scale"][0])) / float(b["scale"][0])
            assert rel < RESIDUAL.get(i, 1e-6), (i, rel)
        elif a["type"] == 0:
            assert a["qdim"] == b["qdim"] and np.array_equal(cs.bits(a["scale"]), cs.bits(b["scale"])) and np.array_equal(a["data"], b["data"]), i
            n_w, n_s = n_w + a["data"].size, n_s + a["scale"].size
    assert (n_w, n_s) == (9126, 544) and len(FLIPPED) <= 2
    assert n_zp == 55                                                # the input and tensors 50..103: 46 with a range of their own, PAD, pool, QUANTIZE outputs
    T = got["tensors"]
    for o in got["ops"]:
        if o["op"] in (CONV, DWCONV):
            s_in, wt, bt = T[o["ins"][0]]["scale"][0], T[o["ins"][1]], T[o["ins"][2]]
            assert np.array_equal(bt["data"], ptq.quantize_bias(_float_bias(o, got), s_in, wt["scale"])), o
            assert np.array_equal(cs.bits(bt["scale"]), cs.bits((np.float64(s_in) * wt["scale"].astype(np.float64)).astype(np.float32)))
            n_b += bt["data"].size
            if o["ins"][0] not in (66, 97):                          # (behind a residual tensor the input scale differs, and the bias with it)
                assert np.array_equal(bt["data"], want["tensors"][o["ins"][2]]["data"]), o
    assert n_b == 544
    assert (cs.bits(T[0]["scale"])[0], T[0]["zp"]) == (0x3B808081, -128)
    for o in got["ops"]:                                             # what csrc/yf_model_file.c demands of PAD, pool and CONCATENATION tensors
        same = lambda x, y: cs.bits(T[x]["scale"])[0] == cs.bits(T[y]["scale"])[0] and T[x]["zp"] == T[y]["zp"]
        if o["op"] in (PAD, MAXPOOL):
            assert same(o["ins"][0], o["out"])
        if o["op"] == CONCAT:
            assert same(o["ins"][0], o["out"]) and same(o["ins"][1], o["out"])


def _float_bias(op, model):
    k = [o for o in model["ops"] if o["op"] in (CONV, DWCONV)].index(op)
    return cs.npz_convs()[k][1]


def test_concatenation_ranges_are_unions_and_pools_are_observed():
    """The rule for tensors 71 and 93, on ranges where it matters: the pool's own minimum decides, not its input's."""
    r = dict(cs.host_result("yfw")[0])
    assert r[58][0] >= r[57][0] and r[58][1] == r[57][1] and r[74][0] >= r[73][0] and r[74][1] == r[73][1]
    r[57], r[58], r[70] = (-9.0, 4.0), (-1.0, 4.0), (-2.0, 3.0)
    T = model_file.load_yfm(ptq.quantize_model(cs.yfw_bytes("yfw"), r))["tensors"]
    s, zp = ptq.activation_qparams(-2.0, 4.0)
    for t in (71, 70, 103):
        assert (T[t]["scale"][0], T[t]["zp"]) == (s, zp), t
    s, zp = ptq.activation_qparams(-9.0, 4.0)
    for t in (57, 58, 59):
        assert (T[t]["scale"][0], T[t]["zp"]) == (s, zp), t
    del r[74]
    with pytest.raises(ValueError, match="tensor 74 is missing"):
        ptq.quantize_model(cs.yfw_bytes("yfw"), r)


@pytest.mark.parametrize("name", cs.WEIGHT_SETS)
def test_written_model_is_admitted_by_the_library(hp, name):
    """write_yfm and load_yfm are inverses on the produced image; csrc/yf_model_file.c parses it and yf_prepare_tables_model builds its tables
    under every rounding tests/test_model_file_host.py covers."""
    image = cs.host_model(name)
    assert model_file.write_yfm(model_file.load_yfm(image)) == image
    rc, text, mf = parse(hp, image)
    assert rc == 0, text
    T = model_file.load_yfm(image)["tensors"]
    assert (mf.out_scale_bits, mf.out_zero_point) == (int(cs.bits(T[100]["scale"])[0]), T[100]["zp"])
    for rounding in ROUNDINGS:
        rc, tab, _ = prepare_model(hp, mf, rounding)
        assert rc == 0 and tab, (name, rounding)
    if name == "yfw":                                                # a model of its own: another output quantisation than the shipped one
        assert (mf.out_scale_bits, mf.out_zero_point) != (0x3e11987e, -15)
        assert abs(float(T[100]["scale"][0]) - 0.11397) < 1e-4 and T[100]["zp"] == -15


# ---------------------------------------------------------------------------------------------------------------- refusals
def _patched(b, at, fmt, value):
    b = bytearray(b)
    struct.pack_into(fmt, b, at, value)
    return bytes(b)


def _record(c):
    """byte offset of conv c's record in a .yfw"""
    at = 8
    for d in model_file.graph_convs()[:c]:
        at += 24 + 4 * (int(np.prod(d["shape"])) + d["cout"])
    return at


def _refusals():
    y = cs.yfw_bytes("yfw")
    r2, r5 = _record(2), _record(5)
    without_last = y[:_record(23)]
    return [
        ("truncated", y[:20000], "conv 18: 320 weights and 8 biases at byte 19904 end past the 20000 bytes of the file"),
        ("cut inside a record", y[:r5 + 10], "conv 5: its record at byte %d ends past the %d bytes of the file" % (r5, r5 + 10)),
        ("wrong magic", b"YFM1" + y[4:], "magic is 59 46 4d 31, expected 'YFW1'"),
        ("23 convs", _patched(without_last, 4, "<I", 23), "23 convs, expected 24"),
        ("swapped cin", _patched(_patched(y, r2 + 4, "<I", 4), r2 + 8, "<I", 8), "conv 2: cin is 4, expected 8"),
        ("n_weights that disagrees", _patched(y, r5 + 20, "<I", 107), "conv 5: n_weights is 107, expected 108"),
        ("a stride", _patched(y, _record(4) + 16, "<I", 1), "conv 4: stride is 1, expected 2"),
        ("NaN weight", _patched(y, r2 + 24 + 4 * 7, "<I", 0x7FC00000), "conv 2: weight 7 has bits 0x7fc00000, expected a finite float32"),
        ("infinite bias", _patched(y, r2 + 24 + 4 * 32 + 4 * 3, "<I", 0xFF800000), "conv 2: bias 3 has bits 0xff800000, expected a finite float32"),
        ("trailing bytes", y + b"\0\0\0\0", "%d bytes, the convs' counts give %d" % (len(y) + 4, len(y))),
    ]


@pytest.mark.parametrize("what,image,text", _refusals(), ids=[r[0] for r in _refusals()])
def test_float_model_is_refused_with_the_first_mismatch(what, image, text):
    with pytest.raises(calib.CalibError) as ei:
        calib.host_run(image, cs.calib_frames()[:1])
    assert text in str(ei.value), (what, str(ei.value))
    with pytest.raises(calib.CalibError):
        cs.HostCalibration(image)


def test_ranges_before_any_frame_and_no_frames_are_refused():
    cal = cs.HostCalibration(cs.yfw_bytes("yfw"))
    with pytest.raises(calib.CalibError, match="no frame has been observed yet"):
        cal.ranges()
    cal.observe(cs.calib_frames()[:13])
    cal.observe(cs.calib_frames()[13:])
    assert cal.ranges() == cs.host_result("yfw")[0] and cal.frames_observed == 27
    cal.reset()
    with pytest.raises(calib.CalibError, match="no frame has been observed yet"):
        cal.ranges()
    with pytest.raises(calib.CalibError, match="n = 0 is below 1"):
        calib.host_run(cs.yfw_bytes("yfw"), np.zeros((0, 56, 56, 3), np.int8))


def test_an_all_zero_filter_channel_is_refused_by_quantize_model():
    convs = [(w.copy(), b, dw) for w, b, dw in cs.npz_convs()]
    convs[6][0][17] = 0                                              # conv2d_13 (op 13, dense OHWI): output channel 17
    with pytest.raises(ValueError, match=r"conv 6 \(op 13\): filter channel 17 is all zero"):
        ptq.quantize_model(model_file.write_yfw(convs), cs.host_result("npz")[0])
    convs = [(w.copy(), b, dw) for w, b, dw in cs.npz_convs()]
    convs[7][0][..., 5] = 0                                          # conv2d_15 (op 15, depthwise 1HWC): channel 5
    with pytest.raises(ValueError, match=r"conv 7 \(op 15\): filter channel 5 is all zero"):
        ptq.quantize_model(model_file.write_yfw(convs), cs.host_result("npz")[0])


def test_yfw_parser_alone_is_clean_under_asan_and_ubsan(tmp_path):
    """tests/csrc/yfw_sanitize_main.c, a program of its own linked with the parser alone: the malformed images above, truncations, every record
    field at extreme values and every weight / bias position special, each image in a heap block of exactly its size."""
    cc = os.environ.get("CC", "cc")                                  # the compiler csrc/Makefile's $(CC) resolves to; a machine without one fails here
    exe, model = str(tmp_path / "yfw_sanitize"), str(tmp_path / "model.yfw")
    open(model, "wb").write(cs.yfw_bytes("yfw"))
    subprocess.check_call([cc, "-O1", "-g", "-std=gnu11", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "csrc", "yfw_sanitize_main.c"),
                           os.path.join(PKG, "csrc", "yf_yfw.c")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, model], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("float model: ok"), r.stdout + r.stderr
