"""The designed quantisations (tests/quant_designs.py) on the CPU: that each design's bound stands in the HOST BUILDER's tables under every kernel set that
admits it, that those tables are the numpy restatement's, that the two references agree on every design, and -- from the oracle alone -- that a green
GPU run of a design means something (liveness).  The admission edges themselves are in tests/test_model_file_host.py, beside the shift-range refusal.
No GPU."""
import os
import struct

import numpy as np
import pytest

from conftest import GOLDEN
import model_variants as mv
import quant_designs as qd
from oracle.np_restatement import NpModel
from test_host_logic import N_LUT, DENSE_OPS, DW_OPS, LEAKY_LUT_IDS, _chan
from test_model_file_host import hp, parse, prepare_model, assert_tables_equal_a_numpy_restatement, SHIFT_RANGE      # noqa: F401 (hp is a fixture)

REF, TIES_UP, SINGLE, FP32 = qd.ROUNDINGS
ORACLE_VARIANT = {REF: 0, TIES_UP: 1, SINGLE: 4, FP32: 3}
K_FP32 = 0x4B400000
DESIGNS = qd.DESIGNS
IDS = [d.name for d in DESIGNS]


@pytest.fixture(scope="module")
def oracles(tmp_path_factory):
    from oracle.oracle import Oracle
    d = tmp_path_factory.mktemp("designs")
    cache = {}

    def get(name):
        if name not in cache:
            path = qd.BY_NAME[name].write(d) if name != "S" else qd.rm.SHIPPED
            cache[name] = (Oracle(path), path)
        return cache[name]
    return get


@pytest.fixture(scope="module")
def frames():
    """the 56x56 frames of tests/test_quant_designs_gpu.py (those of tests/test_model_file_gpu.py): the golden six, the real ones and noise"""
    return qd.frames_56()


def _tables(hp, design, rounding):
    rc, text, mf = parse(hp, design.bytes())
    assert rc == 0, text
    return prepare_model(hp, mf, rounding)


def _pass_of(ix, op, ch):
    """(offset of the yf_pass array, channel index in it) of a conv channel in the table blob"""
    if op in DENSE_OPS:
        return ix.dense[DENSE_OPS.index(op)].c_off, ch
    return ix.dw[DW_OPS.index(op)].g_off + (ch // 4) * 224 + 144, ch % 4


def _channels(tab, ix, design, fp32=False):
    """[(op, ch, M, rshift, ZR)] of the design's targeted conv channels as the builder wrote them; under fp32 (op, ch, fs bits, K, bias')"""
    out = []
    for op, chs in design.targets().items():
        if op in DENSE_OPS or op in DW_OPS:
            for ch in chs:
                off, j = _pass_of(ix, op, ch)
                if fp32:
                    base = off + 80 * (j // 4)
                    out.append((op, ch, struct.unpack_from("<I", tab, base + 4 * (j % 4))[0], struct.unpack_from("<i", tab, base + 64 + 4 * (j % 4))[0],
                                struct.unpack_from("<i", tab, base + 16 + 4 * (j % 4))[0]))
                else:
                    mult, rs, zr, _ = _chan(tab, off, j)
                    out.append((op, ch, mult, rs, zr))
    return out


@pytest.mark.parametrize("design", DESIGNS, ids=IDS)
def test_admission_is_what_the_design_states(hp, design):
    """a design is admitted under every rounding but those it names, which refuse it through YF_PREP_ERR_SHIFT_RANGE; every design is admitted by the two
    integer kernel sets, and every bound but the multiplier's (the float32 epilogue has none) by the fp32 one through some design"""
    for r in qd.ROUNDINGS:
        rc = _tables(hp, design, r)[0]
        assert rc == (0 if design.admitted(r) else SHIFT_RANGE), (design, hex(r), rc)
    assert all(design.admitted(r) for r in (REF, TIES_UP, SINGLE))
    assert [d.name for d in DESIGNS if not d.admitted(FP32)] == ["M"] and sum(d.saturation_only for d in DESIGNS) <= 2


@pytest.mark.parametrize("design", DESIGNS, ids=IDS)
def test_the_bound_aimed_at_stands_in_the_builders_tables(hp, design):
    """From yf_prepare_tables_model's output under every admitting rounding -- not from the generator's intentions: the shifts, multipliers, Z, accumulator
    bounds, add shifts, halo zero points and table slopes each design is named for, and the exported table's figures."""
    name, m = design.name, design.model()
    reached = qd.reached(design)
    for r in (x for x in qd.ROUNDINGS if design.admitted(x)):
        rc, tab, ix = _tables(hp, design, r)
        assert rc == 0
        T, ops = m["tensors"], m["ops"]
        if r == FP32:
            for op, ch, fs_bits, k, bias2 in _channels(tab, ix, design, fp32=True):
                assert k == K_FP32 - (T[ops[op]["out"]]["zp"] + 128) and fs_bits == int(qd.fp32_scale(m, op, ch).view(np.uint32)), (op, ch)
            if name in ("Z0", "Z255"):
                assert {k for *_, k, _ in _channels(tab, ix, design, fp32=True)} == {K_FP32 - (0 if name == "Z0" else 255)}
            if name == "SAT":                           # acc_max * fs one accumulator unit under 2^21, behind Z = 0 and Z = 255
                seen = set()
                for op, ch, fs_bits, k, bias2 in _channels(tab, ix, design, fp32=True):
                    fs, acc = float(np.uint32(fs_bits).view(np.float32)), qd.acc_bound(m, op, ch)
                    assert abs(bias2) + 255 * int(np.abs(qd.channel_view(m, op)[ch]).sum()) == acc
                    assert float(acc) * fs < 2097152.0 <= float(acc + 1) * fs, (op, ch)
                    seen.add((K_FP32 - k, np.sign(bias2)))
                assert seen == {(0, 1), (0, -1), (255, 1), (255, -1)}
        else:
            chans = _channels(tab, ix, design)
            hist = {}
            for op, ch, mult, rs, zr in chans:
                assert (mult, rs) == qd.multiplier(m, op, ch)
                hist[rs] = hist.get(rs, 0) + 1
            assert hist == reached["shifts"] and (not chans or (min(c[2] for c in chans), max(c[2] for c in chans)) == reached["mq"])
            if name in ("R1", "R20"):
                want = 1 if name == "R1" else 20
                assert {c[3] for c in chans} == {want} and {c[0] for c in chans} == set(qd.R_CONVS if name == "R1" else qd.R20_CONVS)
            if name == "RMIX":
                assert all(rs == (1, 20, 2, 19)[ch % 4] for _, ch, _, rs, _ in chans) and {c[0] for c in chans} == set(qd.R_CONVS)
                for op in (6, 10, 53):                  # the half-filled last pass of the 18-channel layers: its two live channels at 1 and 20
                    assert sorted(rs for o, ch, _, rs, _ in chans if o == op and ch >= 16) == [1, 20]
            if name == "M":
                for op, ch, mult, rs, zr in chans:
                    assert mult == qd.M_CONVS[op][0] and rs == qd.M_PLAN[ch][0] and qd.acc_bound(m, op, ch) == (1 << 29) - 1, (op, ch)
                assert {c[2] for c in chans} == {(1 << 30) + 1, (1 << 31) - 1} and {c[3] for c in chans} == {2, 20} and reached["acc"] > 0.99
            if name in ("Z0", "Z255"):
                z = 0 if name == "Z0" else 255
                for op, ch, mult, rs, zr in chans:      # ZR = Z << rs in the four-instruction form (folded dense passes carry it inside C64: the restatement test)
                    if r == REF or op in DW_OPS:
                        assert zr == z << rs, (op, ch)
                assert {T[ops[op]["out"]]["zp"] + 128 for op in design.targets()} == {z} == set(reached["Z"])
                assert {18, 35, 41, 53} <= set(design.targets()) and all(ix.add[s].zpo + 128 == z and ix.add[s].zro == z << ix.add[s].rso for s in range(3))
        if name in ("ZIN127", "ZINm128"):
            zp = 127 if name == "ZIN127" else -128
            assert [ix.halo_zp[s] for s in range(7)] == [zp] * 7 == [T[t]["zp"] for t in qd.HALO_TENSORS] and ix.in_zp == -128
            assert T[59]["zp"] == T[75]["zp"] == zp                                           # the outputs of PAD #9 and #26: what the device fills their halo with
        if name == "ADD":
            a, b = ix.add[0], ix.add[1]
            assert (a.rso, a.zpo, b.rso, b.zpo) == (20, 127, qd.ADD_LOW_RSO, -128) and reached["rso"][:2] == [20, qd.ADD_LOW_RSO]
            assert (a.m1, a.s1, a.m2, a.s2) == (1 << 30, -6, 1 << 30, 0) and (b.m1, b.s1, b.m2, b.s2) == (1 << 30, 0, 1 << 30, -6)      # s1/s2 = 1/64 and 64: powers of two
        if name == "SAT":
            assert ix.add[2].rso == 1 and ix.add[2].mo > 1 << 30 and reached["rso"][2] == 1
        if name == "LUT":
            lut = np.frombuffer(tab, np.int8, N_LUT * 256, ix.lut_off).reshape(N_LUT, 256).astype(int)
            for op in qd.LUT_LEAKY_16 + qd.LUT_LEAKY_16TH:
                s_in, s_out, zi = T[ops[op]["ins"][0]]["scale"][0], T[ops[op]["out"]]["scale"][0], T[ops[op]["ins"][0]]["zp"] + 128
                row = lut[LEAKY_LUT_IDS[op]]
                if op in qd.LUT_LEAKY_16:
                    assert s_in == np.float32(16) * s_out and (row[zi + 1] - row[zi] == 16 or row[zi] + 16 > 127), op
                else:
                    assert s_out == np.float32(16) * s_in and row[zi + 16] - row[zi] == 1, op
            for op, ratio in qd.LUT_QUANTIZE.items():
                assert np.float32(T[ops[op]["ins"][0]]["scale"][0]) == np.float32(ratio) * np.float32(T[ops[op]["out"]]["scale"][0]), op


@pytest.mark.parametrize("design", DESIGNS, ids=IDS)
def test_design_tables_equal_the_numpy_restatement(hp, design):
    """the restatement tests/test_model_file_host.py applies to A and W, on every design: REF, ties_up and single in the folded and the four-instruction
    form, and fp32 where the design is admitted"""
    assert_tables_equal_a_numpy_restatement(hp, design.bytes(), fp32=design.admitted(FP32))


@pytest.mark.parametrize("design", DESIGNS, ids=IDS)
def test_the_two_references_agree_on_the_design(oracles, design):
    """the C oracle against oracle/np_restatement.py on the six golden frames, every op's output, in each oracle variant a GPU case of the design uses"""
    orc, path = oracles(design.name)
    x = np.fromfile(os.path.join(GOLDEN, "golden_inputs.bin"), np.int8).reshape(-1, 56, 56, 3)
    npm = NpModel(path)
    sizes, offs, shapes = mv.dump_layout()
    for r in (x_ for x_ in qd.ROUNDINGS if design.admitted(x_)):
        v = ORACLE_VARIANT[r]
        heads, dump = orc.run(x, dump=True, variant=v)
        for f in range(x.shape[0]):
            head, outs = npm.run(x[f], dump=True, variant=v)
            for op, y in enumerate(outs):
                d = mv.first_difference(dump[f:f + 1, offs[op]:offs[op] + sizes[op]], y.reshape(1, -1), shapes[op])
                assert d is None, f"{design}, oracle variant {v}, frame {f}: tflite op {op} differs first at (y, x, channel) = {d[1:4]}: C oracle {d[4]}, numpy {d[5]}"
            assert np.array_equal(head, heads[f])


@pytest.mark.parametrize("design", DESIGNS, ids=IDS)
def test_designs_are_live_on_the_oracle_alone(oracles, frames, design):
    """On the GPU module's 56x56 frames each targeted tensor, restricted to the targeted channels, takes at least 16 distinct byte values, has neither clamp
    end above 90 % of its bytes and, where the design is about a clamp, hits both ends; the heads differ from the shipped model's.  The two
    saturation-only designs must instead hit both ends.  A tensor whose table cannot have 16 levels (design.not_live states the arithmetic) is held to that
    bound instead -- the condition is not loosened for any other."""
    orc = oracles(design.name)[0]
    assert not np.array_equal(orc.run(frames, threads=8), oracles("S")[0].run(frames, threads=8))
    for op, (distinct, lo, hi) in qd.liveness(design, orc, frames).items():
        print(f"{design} op {op}: {distinct} distinct bytes, {100 * lo:.1f} % at -128, {100 * hi:.1f} % at 127")
        if design.saturation_only:
            assert lo > 0 and hi > 0, (design, op)
        elif op in design.not_live:
            assert distinct <= 18 and lo <= 0.9 and hi <= 0.9, (design, op, design.not_live[op])
        else:
            assert distinct >= 16 and lo <= 0.9 and hi <= 0.9 and (not design.clamp or (lo > 0 and hi > 0)), (design, op, distinct, lo, hi)


def test_exported_table_names_every_design_and_what_it_reached():
    table = qd.design_table()
    assert [row["name"] for row in table] == IDS
    for row in table:
        assert row["bound"] and set(row["reached"]) == {"shifts", "mq", "acc", "Z", "rso", "zp_in"}
        assert bool(row["note"]) == (row["saturation_only"] or bool(row["not_live"]))
