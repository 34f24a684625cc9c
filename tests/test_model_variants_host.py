"""CPU tests of the int8 path on weight blobs OTHER than the shipped one (tests/model_variants.py): the host's admission bound from both sides, the fused
epilogue's identities on the tables prepared from blobs that sit on that bound, and -- from the oracle alone -- that the variants the GPU tests run are
informative (a green GPU run must not mean "everything saturated to one answer").  No GPU, no compute calls of the product."""
import ctypes
import os

import numpy as np
import pytest

import model_variants as mv
from conftest import ROOT
from host_libs import host_library
from test_host_logic import Index, O, PKG, _chan, _device_requant, _device_requant3

INT_ROUNDINGS = [0, 1, 2, 3, 0x100, 0x101, 0x102, 0x103]
SENTINEL = 0x5A5A5A5A           # *out_blob before the call


@pytest.fixture(scope="module")
def prepare():
    """prepare(blob, rounding) -> (return code, index, table bytes or None, *out_blob afterwards) of yf_prepare_tables_rounding"""
    lib = host_library("libyf_hostprep.so")
    lib.yf_prepare_tables_rounding.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(Index)]
    libc = ctypes.CDLL(None)
    libc.free.argtypes = [ctypes.c_void_p]

    def run(blob, rounding):
        out, ix = ctypes.c_void_p(SENTINEL), Index()
        rc = lib.yf_prepare_tables_rounding(blob, len(blob), rounding, ctypes.byref(out), ctypes.byref(ix))
        tab = None
        if rc == 0:
            tab = bytes((ctypes.c_uint8 * ix.total_bytes).from_address(out.value))
            libc.free(out)
        return rc, ix, tab, out.value
    return run


@pytest.fixture(scope="module")
def frames():
    return mv.variant_frames()


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("variants")


def test_identity_variant_is_the_shipped_network(prepare, oracle, frames, tmp_path):
    """The helper's byte patch of blob and .yfm, applied with nothing changed, gives the shipped blob, the shipped model file and the shipped oracle output;
    and the blob the LIBRARY ships (yf_weights_blob) is the one the helper patches."""
    blob, path = mv.identity().build(tmp_path)
    assert blob == mv.shipped_blob() and open(path, "rb").read() == open(mv.SHIPPED_YFM, "rb").read()
    lib = ctypes.CDLL(os.path.join(PKG, "lib", "libyf_hostprep.so"))
    assert bytes((ctypes.c_uint8 * mv.BLOB_BYTES).in_dll(lib, "yf_weights_blob")) == blob
    from oracle.oracle import Oracle
    assert np.array_equal(Oracle(path).run(frames, threads=8), oracle.run(frames, threads=8))
    # a real patch reaches both files: no weight or bias byte range of a jitter variant equals the shipped one, and the .yfm holds the blob's tensors
    from oracle.np_restatement import load_yfm
    v = mv.jitter(1)
    jblob, jpath = v.build(tmp_path)
    m, jm = mv.model(), load_yfm(jpath)
    assert len(jblob) == len(blob) and os.path.getsize(jpath) == os.path.getsize(mv.SHIPPED_YFM)
    for op, d in m.convs.items():
        o = jm["ops"][op]
        wt, bt = jm["tensors"][o["ins"][1]], jm["tensors"][o["ins"][2]]
        assert wt["data"].tobytes() == jblob[d["w_off"]:d["w_off"] + wt["dbytes"]] and bt["data"].astype("<i4").tobytes() == jblob[d["b_off"]:d["b_off"] + 4 * d["cout"]]
        assert (wt["data"] != m.w[op].reshape(-1)).all() and (bt["data"] != m.b[op]).all()
        assert np.array_equal(wt["scale"], m.quant[op]["s_w"]) and jm["tensors"][d["t_out"]]["zp"] == m.quant[op]["zp_out"]       # scales and zero points stay


@pytest.mark.parametrize("sign", [1, -1], ids=["pos", "neg"])
@pytest.mark.parametrize("op", sorted(mv.BIAS_EDGE_CHANNELS))
def test_admission_boundary_of_the_integer_roundings(prepare, tmp_path, op, sign):
    """|bias'| + 255 * sum|w| == 2^29 - 1 on one channel is the last bound the host admits, 2^29 the first it refuses (YF_PREP_ERR_SHIFT_RANGE, no table
    blob handed out): a dense conv (conv2d_5, conv2d_47), depthwise ones (conv2d_15, conv2d_27), conv2d_1 (its own packing) and the head (cout 18)."""
    ch = mv.BIAS_EDGE_CHANNELS[op]
    ok, bad = mv.bias_edge(op, ch, sign), mv.bias_edge(op, ch, sign, refused=True)
    assert int(ok.acc_max()[op][ch]) == (1 << 29) - 1 and int(bad.acc_max()[op][ch]) == 1 << 29
    assert int(ok.acc_max()[op].max()) == (1 << 29) - 1 and np.sign(ok.tensors()[1][op][ch] - mv.model().quant[op]["zp_in"] * mv.model().sums(op, mv.model().w[op])[0][ch]) == sign
    blob_ok, blob_bad = ok.build(tmp_path)[0], bad.build(tmp_path)[0]
    assert sum(a != b for a, b in zip(blob_ok, blob_bad)) >= 1 and sum(a != b for a, b in zip(blob_ok, blob_bad)) <= 4      # the twins differ in one bias word
    for r in INT_ROUNDINGS:
        rc, ix, tab, _ = prepare(blob_ok, r)
        assert rc == 0 and tab is not None and ix.total_bytes == len(tab), (ok, hex(r))
        rc, _, tab, out = prepare(blob_bad, r)
        assert rc == mv.YF_PREP_ERR_SHIFT_RANGE and tab is None and out is None, (bad, hex(r), rc)          # *out_blob NULL: no table blob handed out
    rc, _, tab, out = prepare(blob_bad, mv.FP32)
    assert rc == mv.YF_PREP_ERR_SHIFT_RANGE and tab is None and out is None
    # YF_ROUND_FP32 on the 2^29 - 1 twin: admitted exactly where the channel has no tighter bound of its own (acc_max * fs < 2^21 holds up to 2^29 - 1:
    # every channel of conv2d_1 and of the head, fs < 2^-8, and the chosen channels of conv2d_27 and conv2d_47), refused where it has one (conv2d_5, conv2d_15)
    own = mv.model().fp32_acc_bound(op, ch)
    assert (prepare(blob_ok, mv.FP32)[0] == 0) == (own == (1 << 29) - 1) == ok.admitted(mv.FP32), (ok, own)
    if op in (1, 53):
        assert {mv.model().fp32_acc_bound(op, c) for c in range(mv.model().convs[op]["cout"])} == {(1 << 29) - 1} and prepare(blob_ok, mv.FP32)[0] == 0


@pytest.mark.parametrize("sign", [1, -1], ids=["pos", "neg"])
@pytest.mark.parametrize("op,ch", [(5, 2), (38, 9), (3, 1), (12, 0)])
def test_admission_boundary_of_the_fp32_rounding(prepare, tmp_path, op, ch, sign):
    """YF_ROUND_FP32 also asks for acc_max * fs < 2^21, fs = fl32(fl32(s_in * s_w) / s_out): the channel's own bound is found from that statement (float32
    operations, then the product in double as build_chan_fp32 forms it); the largest acc_max below it is admitted, the next one refused -- and every
    integer rounding admits both (these are the blobs 'the integer roundings admit and YF_ROUND_FP32 refuses').  A dense conv (conv2d_5, conv2d_12) and
    depthwise ones (conv2d_3, conv2d_38).  conv2d_1 and the head conv are not in this list because no channel of theirs HAS a bound of its own: their
    fs is below 2^-8, so acc_max * fs < 2^21 holds up to 2^29 - 1 and the accumulator bound is the only one; test_admission_boundary_of_the_integer_roundings
    asserts that, and both sides of the 2^29 bound under YF_ROUND_FP32 for them."""
    m = mv.model()
    a = m.fp32_acc_bound(op, ch)
    fs = float(m.fs(op, ch))
    assert float(a) * fs < mv.FP32_LIMIT <= float(a + 1) * fs and a + 1 < mv.ACC_LIMIT
    ok, bad = mv.fp32_edge(op, ch, sign), mv.fp32_edge(op, ch, sign, refused=True)
    assert int(ok.acc_max()[op][ch]) == a and int(bad.acc_max()[op][ch]) == a + 1
    assert ok.admitted(mv.FP32) and not bad.admitted(mv.FP32) and bad.admitted(0)
    blob_ok, blob_bad = ok.build(tmp_path)[0], bad.build(tmp_path)[0]
    rc, ix, tab, _ = prepare(blob_ok, mv.FP32)
    assert rc == 0 and tab is not None
    rc, _, tab, out = prepare(blob_bad, mv.FP32)
    assert rc == mv.YF_PREP_ERR_SHIFT_RANGE and tab is None and out is None
    for r in INT_ROUNDINGS:
        assert prepare(blob_bad, r)[0] == 0 and prepare(blob_ok, r)[0] == 0


def test_the_helper_states_the_admission_the_host_applies(prepare, workdir):
    """Variant.admitted() is written from the stated bounds (the GPU tests use it to tell an admitted variant from a refused one); the host preparation
    agrees for every variant and rounding.  The integer roundings admit every variant of the list; YF_ROUND_FP32 refuses some bias_edge ones."""
    refused = []
    for v in mv.all_admitted() + mv.bias_edges(refused=True) + [mv.fp32_edge(refused=True), mv.fp32_edge()]:
        blob = v.build(workdir)[0]
        for r in (0, 1, 2, 3, 0x101, 0x103, mv.FP32):
            rc = prepare(blob, r)[0]
            assert rc in (0, mv.YF_PREP_ERR_SHIFT_RANGE) and (rc == 0) == v.admitted(r), (v, hex(r), rc)
            assert (rc == 0) == (not v.refused) or r == mv.FP32, (v, hex(r), rc)
            if rc and not v.refused:
                refused.append(v.name)
    assert refused and all(n.startswith(("bias_edge", "fp32_edge")) for n in refused), refused


# ---- the fused epilogue on the tables of admitted extremes ------------------------------------------------------------------------------
def _channel_constants(ix, tab, op, ch):
    if op in mv.DENSE_OPS:
        return _chan(tab, ix.dense[mv.DENSE_OPS.index(op)].c_off, ch)
    base = ix.dw[mv.DW_OPS.index(op)].g_off + (ch // 4) * (36 * 4 + 80)
    return _chan(tab, base + 144, ch % 4)


def _accumulator_dots(bias2, abs_w, mult, rs, rng):
    """sum w * x_raw values to test a channel on: the two extremes +-255 * sum|w| (accumulators bias' +- 255 * sum|w|), random ones between, and accumulators
    whose first rounding lands on (or next to) a tie of the second shift -- inside the reachable range where it holds any, and around zero"""
    lim = 255 * abs_w
    dots = [lim, -lim, 0, 1, -1] + [int(v) for v in rng.integers(-lim, lim + 1, 24)] + [-bias2, -bias2 - 1, -bias2 + 1]
    half = 1 << (rs - 1)
    k_lo, k_hi = ((bias2 - lim) * mult >> 31) >> rs, ((bias2 + lim) * mult >> 31) >> rs
    ks = {-40, -1, 0, 1} | {k_lo + 1, (k_lo + k_hi) // 2, k_hi - 1}
    for k in sorted(ks):
        a = int(round((k * (1 << rs) + half) * 2.0**31 / mult))
        dots += [s * a - bias2 + d for s in (1, -1) for d in (-2, -1, 0, 1, 2)]
    return [d for d in dots if abs(d + bias2) < (1 << 29) and 0 < O + d < (1 << 32)]


def _check_channel(oracle, consts, bias2, abs_w, zp_out, mode, kind, rng, what):
    """kind 'ref': the four instructions with the carry as TFLite's sign term; 'generic': the same four with a sign-free rounding's constants (the multiply-add
    must never carry out: N inside [2^61, 2^64)); 'folded': the three-instruction form (ZR inside C64, ZR field 0).  Each == the oracle's statement of the
    rounding + zp_out + 128 before the clamp."""
    mult, rs, zr, c64 = consts
    assert 1 <= rs <= 20 and mult > (1 << 30)
    z = zp_out + 128
    assert zr == {"ref": z << rs, "generic": ((z << rs) - (1 << 31)) % (1 << 32), "folded": 0}[kind], what
    dots = _accumulator_dots(bias2, abs_w, mult, rs, rng)
    assert 255 * abs_w in dots and -255 * abs_w in dots, what                     # both extreme accumulators are admitted and checked
    for dot in dots:
        want = oracle.lib.yfo_mbqm_mode(dot + bias2, mult, -rs, mode) + z
        if kind == "folded":
            got = _device_requant3(dot, mult, rs, c64)
        else:
            n = (O + dot) * (2 * mult) + c64
            if kind == "generic":
                assert (1 << 61) <= n < (1 << 64), (what, dot, "the multiply-add carries out")
            got = _device_requant(dot, mult, rs, zr, c64)
        assert got == want, (what, dot, bias2, mult, rs, mode, got, want)


EXTREME_VARIANTS = mv.bias_edges() + [mv.fp32_edge(), mv.fp32_edge(refused=True)] + [mv.uniform(op, v) for op in mv.CONV_OPS for v in (0, 127, -128)] + \
    [mv.amplify(op) for op in mv.CONV_OPS]


@pytest.mark.parametrize("v", EXTREME_VARIANTS, ids=[v.name for v in EXTREME_VARIANTS])
def test_epilogue_identities_on_admitted_extremes(prepare, oracle, workdir, v):
    """build_c64's claim -- the carry-out stands in for TFLite's sign term; the 2^63 keeps acc_p * 2M + C64 inside [2^61, 2^64) for every accumulator the host
    admits -- checked where it is tightest: on the tables prepared from blobs whose accumulator bound is 2^29 - 1, whose weights are all 0 / +127 / -128, or
    amplified, for every channel of the changed conv, every integer rounding and both forms of the dense constants (folded and generic)."""
    m = mv.model()
    op = v.op
    w, b = v.tensors()
    sum_w, abs_w = m.sums(op, w[op])
    q = m.quant[op]
    blob = v.build(workdir)[0]
    rng = np.random.default_rng(op)
    # the distinct forms of the changed conv's constants: dense ref | folded ties-up, single | generic ties-up, single; depthwise ref | ties-up (never folded)
    for r in ([0, 1, 3, 0x101, 0x103] if op in mv.DENSE_OPS else [0, 2]):
        rc, ix, tab, _ = prepare(blob, r)
        assert rc == 0, (v, hex(r))
        _, _, m_dense, m_dw = mv.ROUNDINGS[r & 0xFF]
        if op in mv.DENSE_OPS:
            mode, kind = m_dense, "ref" if m_dense == 0 else "generic" if r & mv.GENERIC else "folded"
        else:
            mode, kind = m_dw, "ref" if m_dw == 0 else "generic"
        for ch in range(m.convs[op]["cout"]):
            bias2 = int(b[op][ch]) - q["zp_in"] * int(sum_w[ch])
            _check_channel(oracle, _channel_constants(ix, tab, op, ch), bias2, int(abs_w[ch]), q["zp_out"], mode, kind, rng, (v.name, hex(r), ch))


# ---- the variants are informative: conditions on the reference alone -------------------------------------------------------------------
@pytest.fixture(scope="module")
def reference_runs(frames, workdir):
    """name -> dict(head, lut=[19 x 256] visited, conv={op: (min, max, distinct, constant per channel)}) from Oracle(yfm_path).run(frames, dump=True)"""
    from oracle.oracle import Oracle
    sizes, offs, shapes = mv.dump_layout()
    producers = mv.lut_input_producers()
    out = {}
    for v in [mv.identity()] + mv.all_admitted():
        head, dump = Oracle(v.build(workdir)[1]).run(frames, dump=True, threads=8)
        lut = np.zeros((19, 256), bool)
        for lid, p in producers.items():
            lut[lid] = np.roll(np.bincount(dump[:, offs[p]:offs[p] + sizes[p]].reshape(-1).view(np.uint8), minlength=256) > 0, 128)      # index = q + 128
        conv = {}
        for op in mv.CONV_OPS:
            y = dump[:, offs[op]:offs[op] + sizes[op]].reshape(-1, shapes[op][2])
            lo, hi = y.min(axis=0), y.max(axis=0)
            conv[op] = (int(lo.min()), int(hi.max()), int((np.bincount(y.reshape(-1).view(np.uint8), minlength=256) > 0).sum()), bool((lo == hi).all()))
        out[v.name] = dict(head=head, lut=lut, conv=conv)
    return out


@pytest.mark.parametrize("seed", [1, 2])
def test_jitter_changes_every_constant_and_stays_informative(reference_runs, seed):
    """jitter: no weight or bias equal to the shipped one (test_identity... checks the bytes), the head differs from the shipped model's on the same frames
    and the frames reach more than half as many distinct heads as there are frames."""
    head, head0 = reference_runs[f"jitter-{seed}"]["head"], reference_runs["identity"]["head"]
    assert not np.array_equal(head, head0) and sum(not np.array_equal(a, b) for a, b in zip(head, head0)) > head.shape[0] // 2
    assert len({h.tobytes() for h in head}) > head.shape[0] // 2


def test_amplify_gains_reach_both_clamps(reference_runs, capsys):
    """amplify(conv, gain), gain from model_variants.AMPLIFY_GAIN: the targeted conv's output contains both -128 and 127, is not constant per channel over the
    batch and takes at least as many distinct values as the shipped model's same tensor on the same frames (strictly more unless that one already takes
    all 256); and the head is not the same for every frame.  Every one of the 24 convs reaches both clamps under the admission bound."""
    lines = ["conv        gain  shipped min/max/distinct   amplified min/max/distinct   distinct heads"]
    bad = []
    for op in mv.CONV_OPS:
        v = mv.amplify(op)
        lo0, hi0, n0, _ = reference_runs["identity"]["conv"][op]
        lo, hi, n, const = reference_runs[v.name]["conv"][op]
        heads = len({h.tobytes() for h in reference_runs[v.name]["head"]})
        lines.append(f"conv2d_{op:<4} {mv.AMPLIFY_GAIN[op]:>4g}  {lo0:>5}/{hi0:>4}/{n0:>4}            {lo:>5}/{hi:>4}/{n:>4}              {heads}")
        if not (lo == -128 and hi == 127 and not const and (n > n0 or n == n0 == 256) and heads > 1 and v.admitted(0)):
            bad.append(v.name)
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert not bad, bad


def test_lut_coverage_of_all_variants_together(reference_runs, capsys):
    """For each of the 19 byte LUTs: the input indices the oracle visits with the shipped model and with the union of all variant families, on the same
    frames.  The union is a superset for every LUT (strict unless the shipped set is already all 256) and includes index 0 and 255 wherever amplify
    reached both clamps of the conv that produces the LUT's input."""
    shipped = reference_runs["identity"]["lut"]
    union = np.zeros_like(shipped)
    for name, r in reference_runs.items():
        union |= r["lut"]
    producers = mv.lut_input_producers()
    lines = ["LUT  input of op  produced by   shipped indices   union of variants"]
    bad = []
    for lid in range(19):
        p = producers[lid]
        n0, n1 = int(shipped[lid].sum()), int(union[lid].sum())
        lines.append(f"{lid:>3}  {mv.LUT_INPUT_OP[lid]:>11}  {'conv2d_' if p in mv.CONV_OPS else 'op '}{p:<6}  {n0:>15}   {n1:>17}" +
                     ("   0 and 255" if union[lid, 0] and union[lid, 255] else ""))
        if not ((union[lid] | ~shipped[lid]).all() and (n1 > n0 or n0 == 256)):
            bad.append(lid)
        if p in mv.CONV_OPS:
            lo, hi = reference_runs[mv.amplify(p).name]["conv"][p][:2]
            if (lo, hi) == (-128, 127) and not (union[lid, 0] and union[lid, 255]):
                bad.append(lid)
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert not bad, bad


def test_the_helpers_tables_are_the_ones_the_other_tests_use():
    """model_variants.py restates a few tables that other test files own; they must stay equal."""
    import test_fp32_requant_gpu
    import test_gpu_parity
    import test_host_logic
    assert mv.STAGES == test_gpu_parity.STAGES == test_fp32_requant_gpu.STAGES
    assert mv.DENSE_OPS == test_host_logic.DENSE_OPS and mv.DW_OPS == test_host_logic.DW_OPS
    assert {r: mv.ROUNDINGS[r][1] for r in (0, 1, 2, 3)} == test_gpu_parity.ROUNDING_TO_VARIANT
    assert {r: mv.ROUNDINGS[r] for r in (1, 2, 3)} == test_host_logic.ROUNDINGS
    assert mv.ROUNDINGS[mv.FP32][1] == test_fp32_requant_gpu.RV_FP32 and mv.FP32 == test_fp32_requant_gpu.FP32 and mv.GENERIC == test_host_logic.GENERIC
    assert {lid: op for op, lid in test_host_logic.LEAKY_LUT_IDS.items()} == {lid: op for lid, op in mv.LUT_INPUT_OP.items() if lid not in (3, 9, 15)}
