"""YF_ROUND_FP32 (float32 requantisation of every conv, the XNNPACK delegate's qs8 arithmetic): host side, no GPU.

The table blob keeps the reference blob's layout, weights, byte LUTs, add tables and index; only the yf_pass constants of the 17 dense and 7 depthwise
stages change meaning (yf_tables.h, yf_pass, FP32): mult2 = bits of fs, zr = bias', rshift = K = 0x4B400000 - (zp_out + 128), c64 = 0.  The kernels
compute idx = med3(bits(fl32(fl32(acc) * fs) + 1.5 * 2^23) - K, 0, 255); emulated here in numpy float32 and compared with the oracle's statement
clamp(lrintf((float)acc * fs) + zp_out, -128, 127) + 128 on every accumulator of each channel's non-clamping window, its clamp edges and the ends of
its reachable range."""
import ctypes
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from host_libs import host_library

FP32, GENERIC = 0x10, 0x100
N_DENSE, N_DW, N_ADD, N_CS = 17, 7, 3, 24
DENSE_OPS = [1, 5, 6, 12, 13, 17, 19, 23, 29, 30, 34, 36, 40, 42, 47, 51, 53]
DW_OPS = [3, 10, 15, 27, 32, 38, 49]
CS_DENSE = [0, -1, 1, 2, -1, 3, 4, -1, 5, 6, 7, -1, 8, 9, -1, 10, 11, -1, 12, 13, 14, -1, 15, 16]     # yf_tables.h yf_cs_dense
CS_DW = [-1, 0, -1, -1, 1, -1, -1, 2, -1, -1, -1, 3, -1, -1, 4, -1, -1, 5, -1, -1, -1, 6, -1, -1]     # yf_tables.h yf_cs_dw
MAGIC = np.float32(1.5 * 2.0**23)


class Dense(ctypes.Structure):
    _fields_ = [("w_off", ctypes.c_uint32), ("c_off", ctypes.c_uint32), ("cout", ctypes.c_uint16),
                ("cout_pad4", ctypes.c_uint16), ("k", ctypes.c_uint16), ("krow", ctypes.c_uint16)]


class Dw(ctypes.Structure):
    _fields_ = [("g_off", ctypes.c_uint32), ("c", ctypes.c_uint16), ("ngroups", ctypes.c_uint16)]


class Add(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("zp1", "zp2", "zpo", "m1", "s1", "m2", "s2", "mo", "so", "kco", "rso")] + \
               [("mo2", ctypes.c_uint32), ("zro", ctypes.c_uint32), ("c64o", ctypes.c_uint32 * 2)]


class Index(ctypes.Structure):
    _fields_ = [("dense", Dense * N_DENSE), ("dw", Dw * N_DW), ("add", Add * N_ADD), ("lut_off", ctypes.c_uint32),
                ("total_bytes", ctypes.c_uint32), ("in_zp", ctypes.c_int32), ("halo_zp", ctypes.c_int32 * N_DW),
                ("cs_v_off", ctypes.c_uint32 * N_CS), ("cs_v_bytes", ctypes.c_uint32 * N_CS), ("cs_s_off", ctypes.c_uint32 * N_CS)]


@pytest.fixture(scope="module")
def prep():
    lib = host_library("libyf_hostprep.so")
    lib.yf_prepare_tables_rounding.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(Index)]
    blob = (ctypes.c_uint8 * 11304).in_dll(lib, "yf_weights_blob")

    def make(rounding):
        out, ix = ctypes.c_void_p(), Index()
        rc = lib.yf_prepare_tables_rounding(blob, 11304, rounding, ctypes.byref(out), ctypes.byref(ix))
        return rc, ix, (bytes((ctypes.c_uint8 * ix.total_bytes).from_address(out.value)) if rc == 0 else None)
    return dict(lib=lib, make=make)


@pytest.fixture(scope="module")
def pack():
    from oracle.np_restatement import load_yfm
    return load_yfm(os.path.join(ROOT, "oracle", "model", "yoloface_int8.yfm"))


def _chan(tab, off, j):
    """channel j of the yf_pass at byte `off`: (mult2, zr, c64, rshift)"""
    mult2, = struct.unpack_from("<I", tab, off + 4 * j)
    zr, = struct.unpack_from("<i", tab, off + 16 + 4 * j)
    lo, hi = struct.unpack_from("<II", tab, off + 32 + 8 * j)
    rs, = struct.unpack_from("<i", tab, off + 64 + 4 * j)
    return mult2, zr, lo | (hi << 32), rs


def _channels(pack, ix, tab):
    """every real conv channel: (kind, op, ch, fs bits, bias' stored, K stored, c64, s_in, s_w, s_out, zp_out, bias' of the model, sum |w|)"""
    T, ops = pack["tensors"], pack["ops"]
    out = []
    for s, op in enumerate(DENSE_OPS):
        o, d = ops[op], ix.dense[s]
        t_in = o["ins"][0] if op != 1 else 0
        wt, bt, to = T[o["ins"][1]], T[o["ins"][2]], T[o["out"]]
        w = wt["data"].reshape(wt["shape"]).astype(np.int64)
        for ch in range(wt["shape"][0]):
            wf = w[ch].reshape(-1)
            m2, zr, c64, k = _chan(tab, d.c_off + 80 * (ch // 4), ch % 4)
            bias2 = int(bt["data"][ch]) - T[t_in]["zp"] * int(wf.sum())
            out.append(("dense", op, ch, m2, zr, k, c64, T[t_in]["scale"][0], wt["scale"][ch], to["scale"][0], to["zp"], bias2, int(np.abs(wf).sum())))
    for s, op in enumerate(DW_OPS):
        o, d = ops[op], ix.dw[s]
        t_in = ops[op - 1]["ins"][0] if ops[op - 1]["op"] == 34 else o["ins"][0]
        wt, bt, to = T[o["ins"][1]], T[o["ins"][2]], T[o["out"]]
        c = wt["shape"][3]
        taps = wt["data"].reshape(wt["shape"]).astype(np.int64)[0].reshape(9, c)
        for ch in range(c):
            m2, zr, c64, k = _chan(tab, d.g_off + (ch // 4) * (36 * 4 + 80) + 144, ch % 4)
            bias2 = int(bt["data"][ch]) - T[t_in]["zp"] * int(taps[:, ch].sum())
            out.append(("dw", op, ch, m2, zr, k, c64, T[t_in]["scale"][0], wt["scale"][ch], to["scale"][0], to["zp"], bias2, int(np.abs(taps[:, ch]).sum())))
    return out


def _device(acc, fs, k):
    """the kernels' five instructions (yf_kernels.hip.h, rqf) in numpy float32: v_cvt_f32_i32, v_mul_f32, v_add_f32, v_sub_u32, v_med3_i32"""
    p = acc.astype(np.float32) * np.float32(fs)
    r = (p + MAGIC).view(np.int32).astype(np.int64)
    return np.clip(r - k, 0, 255)


def _want(acc, fs, zp_out):
    """the oracle's statement (oracle/yf_oracle.c conv_requant, FP32): clamp(lrintf((float)acc * fs) + zp_out, -128, 127), as the unsigned byte q + 128"""
    p = acc.astype(np.float32) * np.float32(fs)
    return np.clip(np.rint(p).astype(np.int64) + zp_out, -128, 127) + 128


def test_fp32_blob_is_accepted_and_generic_is_refused(prep):
    rc, ix, tab = prep["make"](FP32)
    assert rc == 0 and len(tab) == ix.total_bytes
    assert prep["make"](FP32 | GENERIC)[0] == 1            # YF_PREP_ERR_ARGS: no integer-epilogue kernel computes this form
    for bad in (4, 7, 99, 0x104, 0x200, 0x11, 0x20):
        assert prep["make"](bad)[0] == 1
    lib = prep["lib"]
    assert [lib.yf_rounding_kernel_set(r) for r in (0, 1, 2, 3, 0x101, 0x103, FP32)] == [0, 1, 1, 1, 0, 0, 2]
    assert lib.yf_rounding_signless_dense(FP32) == 0 and lib.yf_rounding_signless_dense(1) == 1


def test_fp32_blob_differs_from_the_reference_only_in_the_conv_constants(prep):
    """Same layout, same index, same weights, LUTs and add tables: only the yf_pass constants of the conv stages (and their regrouped copies in the
    fused kernel's constant blocks) differ, and the copies agree with the yf_pass arrays."""
    _, ix0, tab0 = prep["make"](0)
    _, ix, tab = prep["make"](FP32)
    assert bytes(ix) == bytes(ix0) and len(tab) == len(tab0)
    may = np.zeros(len(tab), bool)
    for d in ix.dense:
        may[d.c_off:d.c_off + 80 * (d.cout_pad4 // 4)] = True
    for d in ix.dw:
        for g in range(d.ngroups):
            may[d.g_off + g * 224 + 144:d.g_off + g * 224 + 224] = True
    for cs in range(N_CS):
        if CS_DENSE[cs] >= 0:
            d = ix.dense[CS_DENSE[cs]]
            np_, wb = d.cout_pad4 // 4, d.cout_pad4 * d.krow
            may[ix.cs_v_off[cs] + wb:ix.cs_v_off[cs] + wb + 32 * np_] = True
            src = [d.c_off + 80 * p for p in range(np_)]
            vec = [ix.cs_v_off[cs] + wb + 32 * p for p in range(np_)]
        else:
            d = ix.dw[CS_DW[cs]]
            np_ = d.ngroups
            for g in range(np_):
                may[ix.cs_v_off[cs] + 176 * g + 144:ix.cs_v_off[cs] + 176 * g + 176] = True
            src = [d.g_off + 224 * g + 144 for g in range(np_)]
            vec = [ix.cs_v_off[cs] + 176 * g + 144 for g in range(np_)]
        may[ix.cs_s_off[cs]:ix.cs_s_off[cs] + 48 * np_] = True
        for p in range(np_):
            assert tab[vec[p]:vec[p] + 32] == tab[src[p]:src[p] + 32]                                        # mult2, zr
            assert tab[ix.cs_s_off[cs] + 48 * p:ix.cs_s_off[cs] + 48 * p + 48] == tab[src[p] + 32:src[p] + 80]  # c64, rshift
    a, b = np.frombuffer(tab, np.uint8), np.frombuffer(tab0, np.uint8)
    assert np.array_equal(a[~may], b[~may])
    assert (a[may] != b[may]).any()
    lut_end = ix.lut_off + 19 * 256 + 3 * 2048 + 256
    assert tab[ix.lut_off:lut_end] == tab0[ix.lut_off:lut_end]      # byte LUTs, add tables, the debug LUT: the reference rounding's


def test_fp32_constants_are_the_float32_scales_bias_and_zero_points(prep, pack):
    """fs = fl32(fl32(s_in * s_w) / s_out) bit for bit for all 544 conv channels (338 dense, 206 depthwise), computed in float32 (no double
    intermediate, no contraction); zr = bias'; rshift = 0x4B400000 - (zp_out + 128); c64 = 0."""
    _, ix, tab = prep["make"](FP32)
    chans = _channels(pack, ix, tab)
    assert sum(c[0] == "dense" for c in chans) == 338 and sum(c[0] == "dw" for c in chans) == 206
    n_double_differs = 0
    for kind, op, ch, m2, zr, k, c64, s_in, s_w, s_out, zp_out, bias2, _ in chans:
        fs = np.float32(s_in) * np.float32(s_w) / np.float32(s_out)
        assert m2 == int(np.array(fs, np.float32).view(np.uint32)), (kind, op, ch)
        assert zr == bias2 and k == 0x4B400000 - (zp_out + 128) and c64 == 0, (kind, op, ch)
        n_double_differs += np.float32(float(np.float32(s_in)) * float(np.float32(s_w)) / float(np.float32(s_out))) != fs
    assert n_double_differs > 0          # the double-rounded product would be another constant for some channels: the float32 statement is what is pinned


def test_device_formula_equals_lrintf_on_every_accumulator_that_matters(prep, pack):
    """The kernels' float32 epilogue on the stored constants == the oracle's statement, for every accumulator of each channel's non-clamping window
    (with margins: the clamp edges), every exact tie inside it, and the ends of the reachable range |bias'| + 255 * sum|w|."""
    _, ix, tab = prep["make"](FP32)
    n_acc = n_ties = 0
    max_p = 0.0
    for kind, op, ch, m2, zr, k, _, _, _, _, zp_out, bias2, abs_w in _channels(pack, ix, tab):
        fs = np.array([m2], np.uint32).view(np.float32)[0]
        z = zp_out + 128
        lo, hi = int(np.floor((-z - 2) / fs)) - 2, int(np.ceil((257 - z) / fs)) + 2
        acc = np.arange(lo, hi + 1, dtype=np.int64)
        got, want = _device(acc, fs, k), _want(acc, fs, zp_out)
        assert np.array_equal(got, want), (kind, op, ch)
        assert got[0] == 0 and got[-1] == 255, (kind, op, ch)                  # the window reaches both clamps
        p = acc.astype(np.float32) * fs
        n_ties += int(np.count_nonzero(p - np.floor(p) == 0.5))
        n_acc += acc.size
        ends = np.array([bias2 - 255 * abs_w, bias2 + 255 * abs_w, -(abs(bias2) + 255 * abs_w), abs(bias2) + 255 * abs_w], np.int64)
        assert np.array_equal(_device(ends, fs, k), _want(ends, fs, zp_out)), (kind, op, ch)
        max_p = max(max_p, float(np.abs(ends.astype(np.float32) * fs).max()))
    assert n_acc > 5 * 10**7 and n_ties > 100                                  # 7.5e7 accumulators, 444 exact ties (the ties-to-even cases)
    assert max_p < 2.0**21                                                    # the host's bound: far inside the 2^22 the magic-number rounding needs


def test_fp32_is_a_property_of_the_created_network(yf):
    """yf_network_set_requant_rounding(YF_ROUND_FP32) is stored on a created network; 0x110 latches AI_ERROR_INVALID_PARAM and changes nothing;
    $YF_REQUANT_ROUNDING=fp32 is read by ai_network_create; fp32+generic is carried as the invalid 0x110, which ai_network_init refuses (GPU test)."""
    assert yf.YF_ROUND_FP32 == FP32
    net = yf.Network()
    try:
        assert net.set_requant_rounding(yf.YF_ROUND_FP32).requant_rounding == FP32
        for bad in (FP32 | GENERIC, 4, 7, 99, 0x104, 0x200):
            with pytest.raises(yf.NetworkError) as ei:
                net.set_requant_rounding(bad)
            assert ei.value.type == 0x14 and net.requant_rounding == FP32
        assert net.set_requant_rounding(0).requant_rounding == 0
    finally:
        net.destroy()
    code = ("import sys, importlib\nsys.path.insert(0, %r)\nyf = importlib.import_module('stm32h7-yolo_amd')\n"
            "net = yf.Network(); print(net.requant_rounding); net.destroy()\n") % ROOT
    for word, value in (("fp32", FP32), ("fp32+generic", FP32 | GENERIC), ("ties_up", 1)):
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, YF_REQUANT_ROUNDING=word))
        assert r.returncode == 0 and r.stdout.split()[-1] == str(value), r.stdout + r.stderr


def test_which_tflite_names_fp32(tmp_path):
    """tools/which_tflite.py on the fp32 variant's heads names the library mode that computes them."""
    v = np.load(os.path.join(ROOT, "tests", "golden", "golden_heads_variants.npz"))
    p = tmp_path / "X.bin"
    v["X"].tofile(p)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "which_tflite.py"), str(p)], capture_output=True, text=True)
    assert r.returncode == 0 and "computes variant X:" in r.stdout and "YF_ROUND_FP32" in r.stdout and "YF_REQUANT_ROUNDING=fp32" in r.stdout, r.stdout
