"""Model files on the CPU: the parser (csrc/yf_model_file.c) and the table builder on a model's own numbers (yf_prepare_tables_model), through
libyf_hostprep.so -- no GPU.  The variants are tests/requant_models.py's."""
import ctypes
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT, GOLDEN, REFERENCE, has_reference
from host_libs import host_library
import requant_models as rm
from oracle.np_restatement import quantize_multiplier, mbqm
from test_host_logic import Index, N_LUT, DENSE_OPS, DW_OPS, LEAKY_LUT_IDS, _chan, O as ACC_OFFSET

PKG = os.path.join(ROOT, "stm32h7-yolo_amd")
N_TENSORS, N_CONVS, BLOB = 104, 24, 11304
HDR, TREC, OREC = 24, 44, 52
OPS_AT = HDR + TREC * N_TENSORS
REF, TIES_UP, FP32, GENERIC = 0, 1, 0x10, 0x100
ROUNDINGS = (REF, TIES_UP, 2, 3, FP32, TIES_UP | GENERIC)
SHIFT_RANGE = 3                                     # YF_PREP_ERR_SHIFT_RANGE
model_file = rm.model_file


class WScale(ctypes.Structure):
    _fields_ = [("bits", ctypes.c_void_p), ("count", ctypes.c_int)]


class Model(ctypes.Structure):
    _fields_ = [("scale_bits", ctypes.c_void_p), ("zero_point", ctypes.c_void_p), ("n_tensors", ctypes.c_int), ("wscale", ctypes.c_void_p),
                ("n_convs", ctypes.c_int)]


class ModelFile(ctypes.Structure):                  # yf_model_file, csrc/yf_model_file.h
    _fields_ = [("model", Model), ("scale_bits", ctypes.c_uint32 * N_TENSORS), ("zero_point", ctypes.c_int16 * N_TENSORS),
                ("wscale", WScale * N_CONVS), ("wscale_bits", (ctypes.c_uint32 * 40) * N_CONVS), ("weights", ctypes.c_uint8 * BLOB),
                ("out_scale_bits", ctypes.c_uint32), ("out_zero_point", ctypes.c_int32)]


@pytest.fixture(scope="module")
def hp():
    lib = host_library("libyf_hostprep.so")
    lib.yf_model_file_parse.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ModelFile), ctypes.c_char_p, ctypes.c_size_t]
    lib.yf_prepare_tables_model.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p),
                                            ctypes.POINTER(Index)]
    lib.yf_prepare_tables_rounding.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(Index)]
    lib.yf_model_decode_tables.argtypes = [ctypes.c_uint32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
    lib.free.argtypes = [ctypes.c_void_p]
    return lib


def parse(hp, image):
    """(0, "", ModelFile) or (rc, text, None)"""
    mf, err = ModelFile(), ctypes.create_string_buffer(400)
    rc = hp.yf_model_file_parse(bytes(image), len(image), ctypes.byref(mf), err, 400)
    return (rc, err.value.decode(), mf if rc == 0 else None)


def _tables(hp, call):
    out, ix = ctypes.c_void_p(), Index()
    rc = call(ctypes.byref(out), ctypes.byref(ix))
    if rc != 0:
        assert not out.value
        return rc, None, None
    tab = bytes((ctypes.c_uint8 * ix.total_bytes).from_address(out.value))
    hp.free(out)
    return 0, tab, ix


def prepare_model(hp, mf, rounding):
    return _tables(hp, lambda out, ix: hp.yf_prepare_tables_model(ctypes.byref(mf.model), mf.weights, BLOB, rounding, out, ix))


def prepare_baked(hp, rounding):
    blob = (ctypes.c_uint8 * BLOB).in_dll(hp, "yf_weights_blob")
    return _tables(hp, lambda out, ix: hp.yf_prepare_tables_rounding(blob, BLOB, rounding, out, ix))


def patched(image, at, fmt, value):
    b = bytearray(image)
    struct.pack_into(fmt, b, at, value)
    return bytes(b)


# ---------------------------------------------------------------------------------------------------------------- the shipped model
def test_yfm_writer_and_reader_are_inverses():
    b = rm.shipped_bytes()
    assert model_file.write_yfm(model_file.load_yfm(b)) == b
    for name in ("A", "W", "O"):
        v = rm.build(name)
        assert v != b and len(v) == len(b) and model_file.write_yfm(model_file.load_yfm(v)) == v


@pytest.mark.parametrize("rounding", ROUNDINGS)
def test_shipped_model_file_gives_the_baked_tables(hp, rounding):
    """S through yf_prepare_tables_model: table blob and index byte-equal to yf_prepare_tables_rounding, and the weights rebuilt from the model's
    tensors are the library's blob."""
    rc, text, mf = parse(hp, rm.build("S"))
    assert rc == 0, text
    assert bytes(mf.weights) == bytes((ctypes.c_uint8 * BLOB).in_dll(hp, "yf_weights_blob"))
    assert (mf.out_scale_bits, mf.out_zero_point) == (0x3e11987e, -15)
    rc_m, tab_m, ix_m = prepare_model(hp, mf, rounding)
    rc_b, tab_b, ix_b = prepare_baked(hp, rounding)
    assert (rc_m, rc_b) == (0, 0)
    assert tab_m == tab_b and bytes(ix_m) == bytes(ix_b)


@pytest.mark.skipif(not has_reference(), reason="needs the reference tree's yoloface_int8.tflite")
def test_tflite_to_yfm_reproduces_the_committed_pack():
    tfl = open(os.path.join(REFERENCE, "yoloface", "tflite", "yoloface_int8.tflite"), "rb").read()
    assert model_file.tflite_to_yfm(tfl) == rm.shipped_bytes()


# ---------------------------------------------------------------------------------------------------------------- the variants
@pytest.fixture(scope="module")
def golden_heads_of(tmp_path_factory):
    from oracle.oracle import Oracle
    x = np.fromfile(os.path.join(GOLDEN, "golden_inputs.bin"), np.int8).reshape(-1, 56, 56, 3)
    d = tmp_path_factory.mktemp("requant")
    cache = {}

    def heads(name):
        if name not in cache:
            cache[name] = Oracle(rm.write(name, d)).run(x)
        return cache[name]
    return heads


@pytest.mark.parametrize("name", ["A", "W", "O"])
def test_variants_are_admitted_and_do_not_compute_the_shipped_heads(hp, golden_heads_of, name):
    """(i) the host admits the variant under the reference, ties_up and fp32 roundings; (ii) on the golden frames the oracle's heads for it
    differ from the shipped model's: no GPU case can pass by running the baked constants."""
    rc, text, mf = parse(hp, rm.build(name))
    assert rc == 0, text
    for rounding in (REF, TIES_UP, FP32):
        assert prepare_model(hp, mf, rounding)[0] == 0, (name, rounding)
        assert prepare_model(hp, mf, rounding)[1] != prepare_baked(hp, rounding)[1]
    base = golden_heads_of("S")
    assert np.array_equal(base, np.fromfile(os.path.join(GOLDEN, "golden_heads.bin"), np.int8).reshape(base.shape))
    differ = int((golden_heads_of(name) != base).sum())
    print(f"variant {name}: {differ} of {base.size} golden head bytes differ from the shipped model's")
    assert differ > 0


def _f(x):
    return float(np.float32(x))


def _requant_lut(T, t_in, t_out):
    m, sh = quantize_multiplier(_f(T[t_in]["scale"][0]) / _f(T[t_out]["scale"][0]))
    q = np.arange(-128, 128, dtype=np.int64)
    return np.clip(mbqm(q - T[t_in]["zp"], m, sh) + T[t_out]["zp"], -128, 127).astype(np.int8)


def _leaky_lut(T, t_in, t_out):
    s_in, s_out = np.float32(T[t_in]["scale"][0]), np.float32(T[t_out]["scale"][0])
    ma, sa = quantize_multiplier(_f(s_in * np.float32(0.1) / s_out))
    mi, si = quantize_multiplier(_f(s_in / s_out))
    v = np.arange(-128, 128, dtype=np.int64) - T[t_in]["zp"]
    return np.clip(T[t_out]["zp"] + np.where(v >= 0, mbqm(v, mi, si), mbqm(v, ma, sa)), -128, 127).astype(np.int8)


@pytest.mark.parametrize("name", ["A", "W"])
def test_variant_tables_equal_a_numpy_restatement_on_the_models_scales(hp, name):
    assert_tables_equal_a_numpy_restatement(hp, rm.build(name))


def assert_tables_equal_a_numpy_restatement(hp, image, fp32=True):
    """Every pass's constants, the LUTs and the add tables of a re-quantised model, against oracle/np_restatement.py's quantize_multiplier and
    mbqm on the scales and zero points READ FROM THE FILE: the reference rounding; the dense passes' constants under ties_up and single, in the
    folded sign-free form and in the four-instruction one (YF_ROUND_GENERIC_KERNELS), everything else there as under the reference rounding;
    under fp32 (where the model is admitted) the channels' float32 scale and bias'.  Also used by tests/test_quant_designs_host.py."""
    pack = model_file.load_yfm(image)
    T, ops = pack["tensors"], pack["ops"]
    rc, text, mf = parse(hp, image)
    assert rc == 0, text
    rc, tab, ix = prepare_model(hp, mf, REF)
    assert rc == 0
    rc_f, tab_f, ix_f = prepare_model(hp, mf, FP32)
    assert (rc_f == 0) == bool(fp32)
    others = {r: prepare_model(hp, mf, r) for r in (TIES_UP, 3, TIES_UP | GENERIC, 3 | GENERIC)}
    assert all(v[0] == 0 and len(v[1]) == len(tab) for v in others.values())

    def check_other_forms(c_off, j, mult, rs, bias2, z, dense):
        for r, (_, tab_r, _) in others.items():
            got = _chan(tab_r, c_off, j)
            if not dense:                               # depthwise passes keep the reference rounding under ties_up and single
                assert got == _chan(tab, c_off, j), (hex(r), c_off, j)
                continue
            rounding = (1 << 31) + ((1 << (rs - 1)) << 32) if r & 0xFF == TIES_UP else 1 << (31 + rs)
            if r & GENERIC:
                want, zr = (bias2 - ACC_OFFSET) * 2 * mult + rounding + (1 << 63), ((z << rs) - (1 << 31)) % (1 << 32)
            else:
                want, zr = (bias2 - ACC_OFFSET) * 2 * mult + rounding + ((z << rs) << 32), 0
            assert got == (mult, rs, zr, want % (1 << 64)), (hex(r), c_off, j)

    def t_in_of(op):                                # a convolution's input parameters come from the tensor before an explicit PAD
        t = ops[op]["ins"][0]
        return ops[op - 1]["ins"][0] if ops[op - 1]["op"] == 34 and ops[op - 1]["out"] == t else t

    def check_channel(c_off, c_off_f, j, op, ch, taps, dense):
        o = ops[op]
        t_in, wt, bt, to = t_in_of(op), T[o["ins"][1]], T[o["ins"][2]], T[o["out"]]
        mult, rs, zr, c64 = _chan(tab, c_off, j)
        m, sh = quantize_multiplier(_f(T[t_in]["scale"][0]) * _f(wt["scale"][ch]) / _f(to["scale"][0]))
        assert (mult, -rs) == (m, sh) and 1 <= rs <= 20 and mult > (1 << 30), (op, ch)
        bias2 = int(bt["data"][ch]) - T[t_in]["zp"] * int(taps.sum())
        assert c64 == ((bias2 - ACC_OFFSET) * 2 * mult + (1 << 31) + (((1 << (rs - 1)) - 1) << 32)) % (1 << 64), (op, ch)
        assert zr == (to["zp"] + 128) << rs, (op, ch)
        check_other_forms(c_off, j, mult, rs, bias2, to["zp"] + 128, dense)
        if not fp32:
            return
        fs = np.float32(np.float32(np.float32(T[t_in]["scale"][0]) * np.float32(wt["scale"][ch])) / np.float32(to["scale"][0]))
        base = c_off_f + 80 * (j // 4)
        assert struct.unpack_from("<I", tab_f, base + 4 * (j % 4))[0] == int(fs.view(np.uint32)), (op, ch)
        assert struct.unpack_from("<i", tab_f, base + 16 + 4 * (j % 4))[0] == bias2, (op, ch)

    for s, op in enumerate(DENSE_OPS):
        wt, d = T[ops[op]["ins"][1]], ix.dense[s]
        w = wt["data"].reshape(wt["shape"]).astype(np.int64)
        assert d.cout == wt["shape"][0]
        for ch in range(d.cout):
            check_channel(d.c_off, ix_f.dense[s].c_off if fp32 else 0, ch, op, ch, w[ch].reshape(-1), True)
    for s, op in enumerate(DW_OPS):
        wt, d = T[ops[op]["ins"][1]], ix.dw[s]
        c = wt["shape"][3]
        w = wt["data"].reshape(9, c).astype(np.int64)
        assert ix.halo_zp[s] == T[t_in_of(op)]["zp"]
        for ch in range(c):
            g, j = divmod(ch, 4)
            check_channel(d.g_off + g * 224 + 144, ix_f.dw[s].g_off + g * 224 + 144 if fp32 else 0, j, op, ch, w[:, ch], False)
    assert ix.in_zp == T[0]["zp"] == -128

    lut = np.frombuffer(tab, np.int8, N_LUT * 256, ix.lut_off).reshape(N_LUT, 256)
    for op, lid in LEAKY_LUT_IDS.items():
        assert np.array_equal(lut[lid], _leaky_lut(T, ops[op]["ins"][0], ops[op]["out"])), f"LEAKY_RELU #{op}"
    assert np.array_equal(np.roll(lut[3], 128), _requant_lut(T, 58, 103))         # QUANTIZE #21, raw-indexed
    assert np.array_equal(np.roll(lut[9], 128), _requant_lut(T, 74, 101))         # QUANTIZE #45, raw-indexed
    assert np.array_equal(lut[15], _requant_lut(T, 92, 102)[_leaky_lut(T, 91, 92).astype(int) + 128])   # QUANTIZE #44 o LEAKY_RELU #43

    al = np.frombuffer(tab, "<i4", 3 * 512, ix.lut_off + N_LUT * 256).reshape(3, 2, 256)
    q = np.arange(-128, 128, dtype=np.int64)
    for s, op in enumerate((18, 35, 41)):
        a, o = ix.add[s], ops[op]
        t1, t2, to = T[o["ins"][0]], T[o["ins"][1]], T[o["out"]]
        s1, s2, so = np.float32(t1["scale"][0]), np.float32(t2["scale"][0]), np.float32(to["scale"][0])
        twice = _f(np.float32(2) * max(s1, s2))
        assert (a.m1, a.s1) == quantize_multiplier(_f(s1) / twice) and (a.m2, a.s2) == quantize_multiplier(_f(s2) / twice)
        assert (a.mo, a.so) == quantize_multiplier(twice / _f(np.float32(1 << 20) * so))
        assert (a.zp1, a.zp2, a.zpo) == (t1["zp"], t2["zp"], to["zp"])
        assert np.array_equal(al[s, 0], mbqm((q - a.zp1) << 20, a.m1, a.s1))
        assert np.array_equal(al[s, 1], mbqm((q - a.zp2) << 20, a.m2, a.s2) + ACC_OFFSET)
        assert a.c64o[0] | (a.c64o[1] << 32) == (-ACC_OFFSET * 2 * a.mo + (1 << 31) + (((1 << (a.rso - 1)) - 1) << 32)) % (1 << 64)
        assert a.zro == (a.zpo + 128) << a.rso
    for r, (_, tab_r, ix_r) in others.items():          # LUTs and add tables: the reference rounding's under ties_up and single
        assert tab_r[ix.lut_off:ix.lut_off + N_LUT * 256 + 3 * 2048] == tab[ix.lut_off:ix.lut_off + N_LUT * 256 + 3 * 2048] and bytes(ix_r.add) == bytes(ix.add), hex(r)


# ---------------------------------------------------------------------------------------------------------------- decode tables
def _exact_exp_f32(x):
    """float64 exp rounded once to float32, and the entries whose float64 value lies within 2^-20 of a float32 tie, the distance measured in
    units of the float32 spacing at that value.  (Measured relative to the VALUE, 2^-20 would exclude every argument there is: a float32 tie is
    never further than 2^-24 of the value away.  In spacings, 2^-20 is 2^-43 of the value or wider -- five hundred times the 2^-52 that
    float64 exp can be off by, so an entry outside it rounds the same way whatever the last bit of the float64 exp was.)"""
    y = np.exp(x.astype(np.float64))
    r = y.astype(np.float32)
    r64 = r.astype(np.float64)
    up = np.nextafter(r, np.float32(np.inf)).astype(np.float64)
    dn = np.nextafter(r, np.float32(-np.inf)).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        near = np.minimum(np.abs(y - (r64 + up) / 2) / (up - r64), np.abs(y - (r64 + dn) / 2) / (r64 - dn))
    return r, ~np.isfinite(near) | (near < 2.0 ** -20)


def test_decode_tables_of_another_output_quantisation(hp):
    """O's tables: x = fl32(fl32(q - zp) * s), sigmoid = 1 / (1 + E(-x)), exp = E(x), one float32 operation each, E correctly rounded -- against
    numpy float32 with float64 exp rounded once.  No entry of O may lie near a tie of that rounding (else another O would have been chosen)."""
    scale, zp = rm.output_quantization("O")
    assert (int(scale.view(np.uint32)), zp) != (0x3e11987e, -15)
    sig, ex = np.zeros(256, np.uint32), np.zeros(256, np.uint32)
    hp.yf_model_decode_tables(int(scale.view(np.uint32)), zp, sig.ctypes.data, ex.ctypes.data)
    x = ((np.arange(-128, 128) - zp).astype(np.float32) * scale).astype(np.float32)
    e_neg, tie_neg = _exact_exp_f32(-x)
    e_pos, tie_pos = _exact_exp_f32(x)
    excluded = int((tie_neg | tie_pos).sum())
    assert excluded == 0, f"{excluded} of 256 arguments lie near a float32 tie: choose another O"
    want_sig = (np.float32(1) / (np.float32(1) + e_neg)).astype(np.float32)
    assert np.array_equal(sig, want_sig.view(np.uint32)) and np.array_equal(ex, e_pos.view(np.uint32))
    assert np.all(np.diff(sig.view(np.float32)) >= 0)
    # information: the shipped tables (numpy's float32 exp of the day) against the E-built ones of the shipped quantisation
    hp.yf_model_decode_tables(0x3e11987e, -15, sig.ctypes.data, ex.ctypes.data)
    shipped = np.fromfile(os.path.join(GOLDEN, "decode_tables_f32.bin"), "<u4").reshape(2, 256)
    print(f"shipped decode tables vs E-built: {int((shipped[0] != sig).sum()) + int((shipped[1] != ex).sum())} of 512 entries differ")
    # and the Python mirror builds the same tables
    interp = __import__("importlib").import_module("stm32h7-yolo_amd.interpreter")
    py_sig, py_ex = interp.model_decode_tables(scale, zp)
    assert np.array_equal(py_sig.view(np.uint32), want_sig.view(np.uint32)) and np.array_equal(py_ex.view(np.uint32), e_pos.view(np.uint32))
    assert np.array_equal(interp.model_decode_tables(interp.OUTPUT_SCALE, -15)[0].view(np.uint32), shipped[0])


# ---------------------------------------------------------------------------------------------------------------- refusals
def _tensor(i, field):
    return HDR + TREC * i + {"zp": 20, "ns": 24, "soff": 28, "qdim": 32, "doff": 36, "dbytes": 40}[field]


def _op(i, field):
    return OPS_AT + OREC * i + {"opcode": 0, "in0": 4, "in1": 8, "in2": 12, "out": 16, "padding": 20, "stride_w": 24, "alpha": 48}[field]


def _refusals():
    s = rm.shipped_bytes()
    nd = struct.unpack_from("<I", s, 20)[0]
    zp58 = struct.unpack_from("<i", s, _tensor(58, "zp"))[0]
    return [
        ("bad magic", b"YFM2" + s[4:], "magic is 59 46 4d 32, expected 'YFM1'"),
        ("a doff past the end", patched(s, _tensor(9, "doff"), "<I", nd - 10), "tensor 9: data at doff %d (dbytes 216) ends past the data section of %d bytes" % (nd - 10, nd)),
        ("a soff past the end", patched(s, _tensor(51, "soff"), "<I", nd - 2), "tensor 51: scales at soff %d (1 of them) end past the data section" % (nd - 2)),
        ("ns neither 1 nor the channel count", patched(s, _tensor(9, "ns"), "<I", 3), "tensor 9: n_scales is 3, expected 1 or 8"),
        ("an op's type", patched(s, _op(2, "opcode"), "<I", 114), "op 2: opcode is 114, expected 98"),
        ("an op's stride", patched(s, _op(10, "stride_w"), "<i", 1), "op 10: stride_w is 1, expected 2"),
        ("an op's wiring", patched(s, _op(18, "in1"), "<i", 66), "op 18: inputs[1] is 66, expected 67"),
        ("the LeakyReLU alpha", patched(s, _op(2, "alpha"), "<I", 0x3e4ccccd), "op 2: alpha has bits 0x3e4ccccd, expected 0x3dcccccd"),
        ("an input zero point of -127", patched(s, _tensor(0, "zp"), "<i", -127), "tensor 0 (input): zero point is -127, expected -128"),
        ("a pool output unlike its input", patched(s, _tensor(58, "zp"), "<i", zp58 + 1), "op 8 (MAX_POOL_2D): output tensor 58 has scale bits 0x3d0aa8bd, zero point %d, expected its input's (tensor 57): 0x3d0aa8bd, %d" % (zp58 + 1, zp58)),
        ("a tensor count", patched(s, 4, "<I", 105), "105 tensors, expected 104"),
        ("trailing bytes", s + b"\0\0\0\0", "%d bytes, the header's counts and data size give %d" % (len(s) + 4, len(s))),
    ]


@pytest.mark.parametrize("what,image,text", _refusals(), ids=[r[0] for r in _refusals()])
def test_parser_refuses_with_the_first_mismatch(hp, what, image, text):
    rc, got, _ = parse(hp, image)
    assert rc != 0 and text in got, (what, got)


def test_parser_refuses_every_truncation(hp):
    s = rm.shipped_bytes()
    for n in np.linspace(0, len(s) - 1, 64).astype(int):
        rc, got, _ = parse(hp, s[:n])
        assert rc != 0 and got, n


def test_a_concat_input_unlike_the_output_and_a_bias_scale_are_refused(hp):
    m = model_file.load_yfm(rm.shipped_bytes())
    m["tensors"][70]["zp"] += 1
    rc, got, _ = parse(hp, model_file.write_yfm(m))
    assert rc != 0 and "op 22 (CONCATENATION): input tensor 70" in got, got
    m = model_file.load_yfm(rm.shipped_bytes())
    m["tensors"][26]["scale"][3] *= np.float32(1.001)                 # conv2d_1's bias, channel 3
    rc, got, _ = parse(hp, model_file.write_yfm(m))
    assert rc != 0 and "op 1: bias scale[3]" in got and "(s_in * s_w[3])" in got, got


@pytest.mark.parametrize("rounding", [REF, TIES_UP, FP32])
def test_a_scale_that_drives_a_channel_out_of_the_shift_range_is_refused_by_the_table_builder(hp, rounding):
    """The parser has nothing against the file; the admission checks of ai_network_init apply unchanged (YF_PREP_ERR_SHIFT_RANGE)."""
    m = model_file.load_yfm(rm.shipped_bytes())
    m["tensors"][51]["scale"] = (m["tensors"][51]["scale"] * np.float32(2.0 ** -24)).astype(np.float32)       # conv2d_1's output: multipliers above 1
    rc, text, mf = parse(hp, model_file.write_yfm(m))
    assert rc == 0, text
    assert prepare_model(hp, mf, rounding)[0] == SHIFT_RANGE
    # and every rule of build_chan, build_chan_fp32 and the add block from both sides (tests/quant_designs.py, admission_edges): the model one step inside
    # is admitted and its tables are the restatement's, the one a step outside is refused -- by the roundings the rule belongs to, the others admit both
    import quant_designs as qd
    for rule, inside, outside, refusing, admitting in qd.admission_edges():
        (rc_i, text_i, mf_i), (rc_o, text_o, mf_o) = parse(hp, inside), parse(hp, outside)
        assert (rc_i, rc_o) == (0, 0), (rule, text_i, text_o)
        for r in (rounding, 3) if rounding == TIES_UP else (rounding,):          # the single-rounding form rides with ties_up: the same kernel set
            if r in admitting:
                assert prepare_model(hp, mf_i, r)[0] == 0, rule
                assert prepare_model(hp, mf_o, r)[0] == (SHIFT_RANGE if r in refusing else 0), rule
            else:
                assert prepare_model(hp, mf_i, r)[0] == SHIFT_RANGE, rule
        if rounding == REF:
            assert_tables_equal_a_numpy_restatement(hp, inside, fp32=FP32 in admitting)


def test_table_builder_refuses_a_model_description_of_another_size(hp):
    rc, text, mf = parse(hp, rm.shipped_bytes())
    assert rc == 0
    mf.model.n_tensors = 103
    assert prepare_model(hp, mf, REF)[0] == 1                          # YF_PREP_ERR_ARGS
    mf.model.n_tensors = 104
    mf.wscale[5].count = 5
    assert prepare_model(hp, mf, REF)[0] == 1


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_parser_alone_is_clean_under_asan_and_ubsan(tmp_path):
    """tests/csrc/model_file_sanitize_main.c, linked with the parser alone: the corruptions above, every truncation and every record field set to
    extreme values, each image in a heap block of exactly its size."""
    exe = str(tmp_path / "model_file_sanitize")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu11", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-ffp-contract=off", "-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "csrc", "model_file_sanitize_main.c"),
                           os.path.join(PKG, "csrc", "yf_model_file.c"), "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, rm.SHIPPED], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("model file: ok "), r.stdout + r.stderr


def test_refusals_reach_the_caller_through_the_abi(yf, tmp_path):
    """yf_network_init_model on a created network: a refused image latches AI_ERROR_INIT_FAILED with the parser's text (no GPU is touched before the
    image is accepted); the Interpreter reports a loaded file's quantisation, and the shipped one for a path that does not exist."""
    net = yf.Network()
    try:
        with pytest.raises(yf.NetworkError) as ei:
            net.init_model(patched(rm.build("W"), _op(10, "stride_w"), "<i", 1))
        assert (ei.value.type, ei.value.code) == (0x30, 0x11) and "op 10: stride_w is 1, expected 2" in ei.value.text
        with pytest.raises(yf.NetworkError) as ei:
            net.init_model(rm.build("W")[:1000])
        assert ei.value.type == 0x30 and "1000 bytes" in ei.value.text
        assert net.get_error() == (0, 0)                           # reading the error reset it
        m = model_file.load_yfm(rm.shipped_bytes())                # the parser has nothing against it; the table builder's admission refuses it
        m["tensors"][51]["scale"] = (m["tensors"][51]["scale"] * np.float32(2.0 ** -24)).astype(np.float32)
        for rounding in (REF, TIES_UP, FP32):
            net.set_requant_rounding(rounding)
            with pytest.raises(yf.NetworkError) as ei:
                net.init_model(model_file.write_yfm(m))
            assert (ei.value.type, ei.value.code) == (0x30, 0x12), rounding
            assert "table preparation failed (code 3)" in ei.value.text and "outside what the kernels compute exactly" in ei.value.text
        net.set_requant_rounding(REF)
        with pytest.raises(yf.NetworkError) as ei:
            net.decode_tables()
        assert "not initialised" in ei.value.text
    finally:
        net.destroy()
    interp = __import__("importlib").import_module("stm32h7-yolo_amd.interpreter")
    scale, zp = rm.output_quantization("O")
    it = interp.Interpreter(model_path=rm.write("O", tmp_path))
    assert it.get_output_details()[0]["quantization"] == (float(scale), zp)
    assert it.get_input_details()[0]["quantization"] == (float(np.float32(interp.INPUT_SCALE)), -128)
    it = interp.Interpreter(model_path=str(tmp_path / "no_such_file.tflite"))
    assert it.get_output_details()[0]["quantization"] == (interp.OUTPUT_SCALE, interp.OUTPUT_ZERO_POINT)
    it._net.destroy()
