"""Simulated quantisation in the float evaluation, host build (csrc/yf_calib_sim.h through libyf_calib_host.so): every step of the stated
arithmetic against a numpy restatement, bit for bit; where in a stage each entry applies; the table of a model; refusals; the Python layers
on top (ptq.dequantized_yfw, ptq.choose_ranges, calib.head_ranges, calib.sensitivity).  No GPU."""
import ctypes

import numpy as np
import pytest

import calib_support as cs
import calib_hw_support as hw
import calib_sim_support as ss
import quant_support as qs
from calib_support import calib, ptq, model_file

Y = ss.WEIGHTS


def _y():
    return cs.yfw_bytes(Y)


# ------------------------------------------------------------------------------------------------- the arithmetic
def test_all_disabled_is_the_float_evaluation():
    x = cs.calib_frames()
    want = calib.host_run(_y(), x)[1]
    lg, totals, stats = calib.host_simulate(_y(), x, calib.empty_table(), want, want_stats=True)
    ss.same_bits(lg, want, "all disabled against host_run")
    want_s, want_t = ss.restate(want, want, [0] * 27)
    qs.same_records(stats, want_s, "records")
    qs.same_records(totals, want_t, "totals")
    for k in ("sum_err", "sum_sq_err", "max_abs_err", "saturated"):
        assert not stats[k].any() and not totals[k].any(), k
    assert (stats["sum_sq_ref"] > 0).all() and totals[0]["elements"] == 27 * 882
    # ... and without reference logits there is no record
    lg2, none = calib.host_simulate(_y(), x, calib.empty_table())
    assert none is None
    ss.same_bits(lg2, want, "no reference")


def _head_alone(scale, zp):
    x, ref = cs.calib_frames(), ss.float_logits(Y, 56, 56, 27)
    lg, totals, stats = calib.host_simulate(_y(), x, ss.one_entry(100, scale, zp), ref, want_stats=True)
    want, clipped = zip(*[ss.sim_q(ref[f], scale, zp) for f in range(27)])
    want = np.stack(want)
    ss.same_bits(lg, want, "the head alone")
    want_s, want_t = ss.restate(want, ref, clipped)
    qs.same_records(stats, want_s, "records")
    qs.same_records(totals, want_t, "totals")
    return int(totals[0]["saturated"]), float(totals[0]["sum_sq_err"])


def test_head_alone_is_sim_q_of_the_logits():
    T = model_file.load_yfm(qs.shipped_yfm())["tensors"][100]
    clipped, err = _head_alone(T["scale"][0], T["zp"])
    assert err > 0


def test_head_with_a_narrow_scale_clips():
    clipped, _ = _head_alone(np.float32(0.004), 17)
    assert clipped > 0


def test_head_on_grids_that_put_logits_on_ties_and_at_the_ends():
    """The head entry at scales that put logits on ties (twice a logit's own value), far inside one step, far outside the grid and near the
    least admitted scale: the host build's rint and clamp against numpy's, bit for bit.  The restatement itself is pinned on a hand-written
    vector; the C functions are called on the same vector by tests/csrc/calib_sim_sanitize_main.c."""
    ref = ss.float_logits(Y, 56, 56, 27)
    x = cs.calib_frames()
    for scale, zp in ((np.float32(2.0) * np.abs(ref[0, 0, 0, 0]), 0), (np.float32(2.0 ** -20), -128), (np.float32(2.0 ** 20), 127), (np.float32(1e-38), 0)):
        lg, _ = calib.host_simulate(_y(), x, ss.one_entry(100, scale, zp), ref)
        ss.same_bits(lg, np.stack([ss.sim_q(r, scale, zp)[0] for r in ref]), f"scale {scale!r}")
    v = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -0.3, 0.3, 8388607.5, 8388608.0, -8388609.0, np.inf, -np.inf, np.nan, 126.5, 127.5, -128.5, -129.5], np.float32)
    out, clipped = ss.sim_q(v, 1.0, 0)
    assert clipped == 7 and np.isnan(out[12]) and list(out[:7]) == [0, 2, 2, -0, -2, -0, 0] and list(out[13:]) == [126, 127, -128, -128]


@pytest.mark.parametrize("tensor", [99, 98])
def test_the_position_of_each_step_inside_a_stage(tensor):
    """tensor 99 (a LeakyReLU output) and tensor 98 (the convolution before it) quantised alone: the head restated from the float tensors"""
    x = cs.calib_frames()[:9]
    n, e = x.shape[0], 49 * 32
    entries = [calib.Entry(t, 1.0, 0, np.zeros((n, e), np.int8), e) for t in (98, 99)]
    _, _, (t98, t99) = calib.host_compare(_y(), x, entries, threads=4, want_tensors=True, elements=[e, e])
    ss.same_bits(ss.leaky(t98), t99, "the float tensors themselves")
    T = model_file.load_yfm(qs.shipped_yfm())["tensors"][tensor]
    scale, zp = T["scale"][0], T["zp"]
    if tensor == 99:
        q, clipped = ss.sim_q(t99, scale, zp)
        want = ss.head_conv(q, _y())
    else:
        q, clipped = ss.sim_q(t98, scale, zp)
        want = ss.head_conv(ss.leaky(q), _y())
    assert not np.array_equal(q, t99 if tensor == 99 else t98)
    ref = ss.float_logits(Y, 56, 56, 27)[:n]
    lg, totals = calib.host_simulate(_y(), x, ss.one_entry(tensor, scale, zp), ref, threads=4)
    ss.same_bits(lg.reshape(n, -1), want, f"tensor {tensor} alone")
    assert int(totals[0]["saturated"]) == clipped


def test_quantize_entries_attach_to_the_stages_the_graph_gives():
    """Entries 47 .. 49 are the graph's QUANTIZE outputs in ascending id; each applies to the value its stage stores, which is where the slot of
    the tensor it copies applies too (a pool's output, a LeakyReLU's with no ADD behind it): with the same parameters the two give the same
    bits, other than the float logits', and both enabled give them again where the grid is idempotent."""
    g = model_file.load_graph()
    quant = sorted((o["out"], o["ins"][0]) for o in g["ops"] if o["op"] == model_file.OPCODE["QUANTIZE"])
    assert ss.ids()[47:] == tuple(t for t, _ in quant) == (101, 102, 103) and len(ss.ids()) == 50
    assert ss.ids()[:47] == tuple(sorted(cs.host_result(Y)[0]))
    x, ref = cs.calib_frames()[:5], ss.float_logits(Y, 56, 56, 27)[:5]
    T = model_file.load_yfm(qs.shipped_yfm())["tensors"]
    seen = []
    for out, src in quant:
        scale, zp = T[out]["scale"][0], T[out]["zp"]
        a, ta = calib.host_simulate(_y(), x, ss.one_entry(out, scale, zp), ref)
        b, tb = calib.host_simulate(_y(), x, ss.one_entry(src, scale, zp), ref)
        ss.same_bits(a, b, f"QUANTIZE output {out} against its input {src}")
        qs.same_records(ta, tb, f"totals, {out} against {src}")
        assert ta[0]["sum_sq_err"] > 0
        seen.append(a)
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2]) and not np.array_equal(seen[0], seen[2])


def test_simulation_table_of_a_quantised_model():
    image = cs.host_model(Y)
    T, g = model_file.load_yfm(image)["tensors"], model_file.load_graph()
    table = calib.simulation_table(image)
    assert table.dtype == calib.SIM_ENTRY and table.shape == (50,) and (table["scale"] > 0).all()
    for i, t in enumerate(ss.ids()):
        assert table[i]["scale"] == T[t]["scale"][0] and table[i]["zero_point"] == T[t]["zp"], t
    quant_out = {o["out"] for o in g["ops"] if o["op"] == model_file.OPCODE["QUANTIZE"]}
    checked = set()
    for o in g["ops"]:
        if o["op"] != model_file.OPCODE["CONCATENATION"]:
            continue
        for t in o["ins"][:2]:                                       # a QUANTIZE output or a tensor wired in directly (70)
            assert tuple(table[ss.entry_of(t)]) == (T[o["out"]]["scale"][0], T[o["out"]]["zp"]), (t, o["out"])
            checked.add(t)
    assert checked == quant_out | {70}
    # tensor 92 reaches its concatenation through QUANTIZE 102 and keeps the parameters of its own range
    assert tuple(table[ss.entry_of(92)]) == tuple(np.array([ptq.activation_qparams(*cs.host_result(Y)[0][92])], calib.SIM_ENTRY)[0])
    one = calib.simulation_table(image, [51, 103])
    assert [ss.ids()[i] for i in np.flatnonzero(one["scale"])] == [51, 103] and tuple(one[1]) == tuple(table[1])
    assert not calib.simulation_table(image, []).view(np.uint8).any()
    with pytest.raises(ValueError, match=r"\[59\] are not among the 50 tensors"):
        calib.simulation_table(image, [51, 59])


# ------------------------------------------------------------------------------------------------- sizes and threads
@pytest.mark.parametrize("h,w,n", [(8, 8, 5), (16, 24, 5), (56, 56, 6)])
def test_threads_and_sizes(h, w, n):
    x = cs.calib_frames()[:n] if (h, w) == (56, 56) else hw.frames(h, w, n)
    table = ss.shipped_table()
    ref1, lg1, t1, s1 = ss.host_all(_y(), x, table, threads=1)
    ref4, lg4, t4, s4 = ss.host_all(_y(), x, table, threads=4)
    assert lg1.shape == (n, h // 8, w // 8, 18)
    ss.same_bits(ref1, calib.host_run(_y(), x)[1], "reference against host_run")
    ss.same_bits(ref4, ref1, "reference, 4 threads")
    ss.same_bits(lg4, lg1, "logits, 4 threads")
    qs.same_records(s4, s1, "records, 4 threads")
    qs.same_records(t4, t1, "totals, 4 threads")
    want_s, want_t = ss.restate(lg1, ref1, s1["saturated"])
    qs.same_records(s1, want_s, "records against the restatement")
    qs.same_records(t1, want_t, "totals against the restatement")
    assert t1[0]["sum_sq_err"] > 0 and t1[0]["elements"] == n * (h // 8) * (w // 8) * 18
    if (h, w) == (56, 56):
        _, lg, t, s = ss.host_all(_y(), x, table, general=True, threads=4)
        ss.same_bits(lg, lg1, "the _hw form at 56x56")
        qs.same_records(s, s1, "records, the _hw form at 56x56")
        qs.same_records(t, t1, "totals, the _hw form at 56x56")


# ------------------------------------------------------------------------------------------------- refusals
def _raw(frames, n, table, ref, logits, stats, totals, h=None, w=None):
    lib, y = calib.load_host(), _y()
    err = ctypes.create_string_buffer(400)
    p = lambda a: None if a is None else a.ctypes.data
    tail = (p(frames), n, p(table), p(ref), p(logits), p(stats), p(totals), 2, err, 400)
    rc = lib.yf_calib_host_simulate(y, len(y), *tail) if h is None else lib.yf_calib_host_simulate_hw(y, len(y), h, w, *tail)
    return rc, err.value.decode()


def test_refusals_name_what_was_refused_and_write_nothing():
    x = np.ascontiguousarray(cs.calib_frames()[:2])
    ref = np.ascontiguousarray(ss.float_logits(Y, 56, 56, 27)[:2])
    logits = np.full((2, 882), -7.5, np.float32)
    stats, totals = np.full(2 * 32, 0x5A, np.uint8), np.full(48, 0x5A, np.uint8)
    ok = ss.shipped_table()

    def bad(tensor, scale, zp):
        t = ok.copy()
        t[ss.entry_of(tensor)] = (scale, zp)
        return t

    cases = [
        ((x, 2, bad(55, -0.5, 0), ref, logits, stats, totals), "entry 5 (tensor 55): scale is -0.5, expected 0 (the tensor stays float) or a finite positive float32"),
        ((x, 2, bad(100, np.nan, 0), ref, logits, stats, totals), "entry 46 (tensor 100): scale is nan"),
        ((x, 2, bad(0, np.inf, 0), ref, logits, stats, totals), "entry 0 (tensor 0): scale is inf"),
        ((x, 2, bad(101, -np.inf, 0), ref, logits, stats, totals), "entry 47 (tensor 101): scale is -inf"),
        ((x, 2, bad(103, 0.25, 128), ref, logits, stats, totals), "entry 49 (tensor 103): zero_point is 128, expected -128 to 127"),
        ((x, 2, bad(51, 0.25, -129), ref, logits, stats, totals), "entry 1 (tensor 51): zero_point is -129, expected -128 to 127"),
        ((x, 0, ok, ref, logits, stats, totals), "n is 0, expected at least 1"),
        ((x, -3, ok, ref, logits, stats, totals), "n is -3, expected at least 1"),
        ((None, 2, ok, ref, logits, stats, totals), "frames is NULL"),
        ((x, 2, None, ref, logits, stats, totals), "table is NULL"),
        ((x, 2, ok, None, logits, stats, None), "frame_stats given without ref_logits"),
        ((x, 2, ok, None, logits, None, totals), "totals given without ref_logits"),
        ((x, 2, ok, ref, logits, None, totals), "ref_logits given without frame_stats, expected room for 2 records"),
        ((x, 2, ok, ref, logits, None, None), "ref_logits given without frame_stats, expected room for 2 records"),
        ((x, 2, bad(53, 1e-39, 0), ref, logits, stats, totals), "entry 3 (tensor 53): scale is 1e-39, whose reciprocal is not a finite float32"),
    ]
    for args, text in cases:
        rc, err = _raw(*args)
        assert rc <= 0 and text in err and err.startswith("yf_calib_host_simulate: "), (text, rc, err)
    for h, w in ((12, 8), (8, 168), (0, 56)):
        rc, err = _raw(x, 1, ok, None, logits, None, None, h, w)
        assert rc <= 0 and f"yf_calib_host_simulate: the frame size is h = {h}, w = {w}, expected multiples of 8 from 8 to 160" in err, err
    assert (logits == -7.5).all() and (stats == 0x5A).all() and (totals == 0x5A).all()
    # a disabled entry's zero point is not read; through Python a refusal is a CalibError with the text
    t = calib.empty_table()
    t[3] = (0.0, 4000)
    ss.same_bits(calib.host_simulate(_y(), x, t)[0], ref, "a disabled entry with a wild zero point")
    with pytest.raises(calib.CalibError, match=r"entry 5 \(tensor 55\): scale is -0.5"):
        calib.host_simulate(_y(), x, bad(55, -0.5, 0))
    with pytest.raises(ValueError, match="table: shape"):
        calib.host_simulate(_y(), x, ok[:49])


# ------------------------------------------------------------------------------------------------- the Python layers
def test_dequantized_yfw():
    y, m = _y(), qs.shipped_yfm()
    assert ptq.dequantized_yfw(y, m, []) == y and ptq.dequantized_yfw(y, m, ()) is not None
    model = model_file.load_yfm(m)
    T, ops, g = model["tensors"], model["ops"], model_file.graph_convs()
    orig, some, every = model_file.read_yfw(y), model_file.read_yfw(ptq.dequantized_yfw(y, m, [1, 23])), model_file.read_yfw(ptq.dequantized_yfw(y, m))
    assert len(every) == 24
    for c, d in enumerate(g):
        wt, bt = T[ops[d["op"]]["ins"][1]], T[ops[d["op"]]["ins"][2]]
        q = wt["data"].reshape(d["shape"]).astype(np.float32)
        s = wt["scale"].astype(np.float32)
        want_w = q * (s.reshape(1, 1, 1, -1) if d["depthwise"] else s.reshape(-1, 1, 1, 1))
        want_b = (bt["data"].astype(np.float64) * bt["scale"].astype(np.float64)).astype(np.float32)
        assert want_w.dtype == np.float32
        ss.same_bits(every[c][0], want_w, f"conv {c} weights")
        ss.same_bits(every[c][1], want_b, f"conv {c} bias")
        assert every[c][2] == d["depthwise"]
        pick = every if c in (1, 23) else orig
        ss.same_bits(some[c][0], pick[c][0], f"conv {c} weights, two listed")
        ss.same_bits(some[c][1], pick[c][1], f"conv {c} bias, two listed")
        # the model's own quantisation of the float weights is within half a step of them
        assert np.abs(every[c][0] - orig[c][0]).max() <= 0.5000001 * s.max()
    assert ptq.dequantized_yfw(ptq.dequantized_yfw(y, m), m) == ptq.dequantized_yfw(y, m)
    with pytest.raises(ValueError, match=r"convs: \[24\]"):
        ptq.dequantized_yfw(y, m, [3, 24])


def test_choose_ranges():
    cands = {5: [(0.0, 1.0), (0.0, 0.9), (0.0, 0.8)], 7: [(-1.0, 1.0), (-0.5, 1.0), (-0.25, 1.0)], 9: [(0.0, 2.0), (0.0, 3.0), (0.0, 4.0)],
             11: [(0.0, 1.0), (0.0, 2.0), (0.0, 3.0)]}
    errors = {5: [3.0, 2.0, 2.5], 7: [1.0, 1.0, 1.0], 9: [2.0, 1.0, 1.0], 11: [float("nan"), 5.0, 4.0]}
    assert ptq.choose_ranges(cands, errors) == {5: (0.0, 0.9), 7: (-1.0, 1.0), 9: (0.0, 3.0), 11: (0.0, 1.0)}
    assert ptq.choose_ranges({5: [(0.0, 1.0)]}, {5: [9.0]}) == {5: (0.0, 1.0)}
    with pytest.raises(ValueError, match="tensor 5: 3 candidates and 2 errors"):
        ptq.choose_ranges({5: cands[5]}, {5: [1.0, 2.0]})
    assert ptq.CLIP_METHODS == ("minmax", "percentile", "mse")


def test_head_ranges_with_identical_candidates_is_minmax():
    """three equal candidates per tensor: one simulation each, every tie goes to the first, and the model is min/max's byte for byte"""
    y, x = _y(), cs.calib_frames()[:5]
    r, _ = calib.host_run(y, x, threads=4)
    calls = []

    def simulate(table, ref):
        calls.append(int(np.count_nonzero(table["scale"])))
        return calib.host_simulate(y, x, table, ref, threads=16)

    chosen = calib.head_ranges({t: [r[t]] * 3 for t in sorted(r)}, simulate, keep=(0,))
    assert chosen == {t: (float(r[t][0]), float(r[t][1])) for t in r}
    assert calls == [0] + [1] * 46
    assert ptq.quantize_model(y, chosen) == ptq.quantize_model(y, r)


def test_head_ranges_takes_the_candidate_with_the_least_head_error():
    y, x = _y(), cs.calib_frames()[:5]
    r, ref = calib.host_run(y, x, threads=4)
    lo, hi = r[51]
    cands = {51: [(lo, hi), (lo / 16, hi / 16), (lo, hi)], 0: [r[0], (0.0, 0.5), (0.0, 0.25)]}
    errs = []
    for c in cands[51]:
        t = ss.one_entry(51, *ptq.activation_qparams(*c))
        errs.append(float(calib.host_simulate(y, x, t, ref)[1][0]["sum_sq_err"]))
    assert errs[1] > errs[0] == errs[2]
    chosen = calib.head_ranges(cands, lambda t, rf: calib.host_simulate(y, x, t, rf), keep=(0,))
    assert chosen == {51: (float(lo), float(hi)), 0: (float(r[0][0]), float(r[0][1]))}
    cands[51] = cands[51][1:]
    assert calib.head_ranges(cands, lambda t, rf: calib.host_simulate(y, x, t, rf), keep=(0,))[51] == (float(lo), float(hi))


def test_sensitivity_rows_on_a_small_size():
    """the table at 16x16 through the host build: 50 + 24 + 3 rows, each the figures of the simulation it names"""
    y, m, x = _y(), qs.shipped_yfm(), hw.frames(16, 16, 4)
    sim = lambda yy, xx, t, ref: calib.host_simulate(yy, xx, t, ref, threads=4)
    rows = calib.sensitivity(y, m, x, simulate=sim)
    assert [r["name"] for r in rows] == [f"tensor {t}" for t in ss.ids()] + [f"conv {c}" for c in range(24)] + ["activations", "weights", "all"]
    assert rows[0]["op"] == "INPUT" and rows[1]["op"] == "CONV_2D" and rows[8]["op"] == "MAX_POOL_2D" and rows[47]["op"] == "QUANTIZE"
    assert rows[50]["op"] == "WEIGHTS" and rows[50]["conv"] == 0 and rows[1]["tensor"] == 51
    ref = calib.host_simulate(y, x, calib.empty_table())[0]
    scale = float(model_file.load_yfm(m)["tensors"][100]["scale"][0])
    _, t = calib.host_simulate(y, x, ss.shipped_table([51]), ref)
    assert rows[1] == calib.sensitivity_row("tensor 51", "CONV_2D", 51, None, t, scale, 4 * 8 * 8 * 8)
    _, t = calib.host_simulate(ptq.dequantized_yfw(y, m, [7]), x, calib.empty_table(), ref)
    assert rows[57] == calib.sensitivity_row("conv 7", "WEIGHTS", None, 7, t, scale, 0)
    _, t = calib.host_simulate(ptq.dequantized_yfw(y, m), x, ss.shipped_table(), ref)
    assert rows[-1]["sqnr_db"] == 10 * np.log10(float(t[0]["sum_sq_ref"]) / float(t[0]["sum_sq_err"])) and rows[-1]["rmse_lsb"] > 0
    assert 0 <= rows[-1]["clipped"] < 0.01
    assert len(calib.format_sensitivity(rows).splitlines()) == 78


def test_coarse_guard_against_a_mis_wired_simulation():
    """On the shipped pair and the 27 calibration frames: quantising the weights alone hurts the head less than quantising everything, and the
    full simulation's rms error against the float logits is within a factor of two of the int8 oracle's own (the simulation predicts the size
    of the loss, not each element).  Host build: ratio 0.97, 34.5 dB against 26.0 dB."""
    y, m, x = _y(), qs.shipped_yfm(), cs.calib_frames()
    ref = ss.float_logits(Y, 56, 56, 27)
    deq = ptq.dequantized_yfw(y, m)
    lw, tw = calib.host_simulate(deq, x, calib.empty_table(), ref, threads=16)
    la, ta = calib.host_simulate(deq, x, ss.shipped_table(), ref, threads=16)
    sqnr = lambda t: 10 * np.log10(float(t[0]["sum_sq_ref"]) / float(t[0]["sum_sq_err"]))
    T = model_file.load_yfm(m)["tensors"][100]
    heads = qs.real_run()[0].reshape(27, -1)
    oracle_rms = hw.rmse(heads, ref.reshape(27, -1), T["scale"][0], T["zp"])
    sim_rms = float(np.sqrt(float(ta[0]["sum_sq_err"]) / int(ta[0]["elements"])))
    print(f"weights {sqnr(tw):.2f} dB, all {sqnr(ta):.2f} dB; rms: simulation {sim_rms / T['scale'][0]:.3f} LSB, oracle {oracle_rms / T['scale'][0]:.3f} LSB, "
          f"ratio {sim_rms / oracle_rms:.3f}")
    assert sqnr(tw) > sqnr(ta)
    assert 0.5 * oracle_rms <= sim_rms <= 2.0 * oracle_rms
