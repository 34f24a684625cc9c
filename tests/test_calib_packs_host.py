"""The host build of the float calibration library against the numpy restatement of the DEFINED arithmetic (calib_packs.evaluate), exactly:
every tensor, range, logit, histogram count, comparison record and simulated logit, on designed weight packs that reach subnormals, -0,
+-inf, NaN and every edge of the simulated quantiser's rounding, and on the two shipped weight sets.  No tolerance anywhere: a value
differs only where both sides are NaN (calib_packs.same_floats).  The certificates keep a pack from testing nothing: they count, in the
restated tensors alone, the value classes each pack names, and show that a contracting or a subnormal-flushing build would be noticed.
Also here: ptq.quantize_model refuses a range that is not finite or is inverted, by name.  Host logic only."""
import numpy as np
import pytest

import calib_packs as cp
import calib_hist_support as hs
import calib_sim_support as ss
import quant_support as qs
from calib_support import calib, ptq

CASES = [(name, h, w) for name in cp.NAMES for h, w in cp.SIZES]
IDS = [f"{name}-{h}x{w}" for name, h, w in CASES]


def test_the_restatement_reads_the_slots_and_entries_the_library_has():
    assert cp.slot_tensors() == tuple(calib.RANGE_TENSORS) == hs.slots() and cp.entry_tensors() == tuple(calib.sim_tensors())
    assert len(cp.slot_tensors()) == 47 and len(cp.entry_tensors()) == 50


def test_same_floats_tells_zeros_apart_and_takes_any_nan_for_any_nan():
    nan = np.array([0x7FC00000, 0xFFC00001], "<u4").view("<f4")
    assert cp.same_floats(nan, nan[::-1]) and cp.same_floats(np.array([0.0, -0.0], np.float32), np.array([0.0, -0.0], np.float32))
    assert not cp.same_floats(np.array([0.0], np.float32), np.array([-0.0], np.float32))
    assert not cp.same_floats(np.array([np.nan], np.float32), np.array([np.inf], np.float32))
    assert not cp.same_floats(np.array([1.0]), np.array([np.nextafter(1.0, 2.0)]))
    with pytest.raises(AssertionError, match="tensor 5 has a NaN end"):
        cp.assert_same_ranges({5: (np.nan, 1.0)}, {5: (np.nan, 1.0)}, "ranges")


# ---------------------------------------------------------------------------------------------------------------- certificates
def _classes(name, h, w, tensor):
    r = cp.restated(name, h, w)
    return cp.count_classes(r.logits if tensor == "logits" else r.tensors[tensor])


def _need(counts, names, what):
    missing = [k for k in names if not counts[k]]
    assert not missing, f"{what}: no value of the classes {missing}; it has {counts}"


@pytest.mark.parametrize("h,w", cp.SIZES)
def test_certificate_subnormal(h, w):
    for t in (55, 56, 57, 58, 94, 95, 96, 97, 98, 99, "logits"):
        _need(_classes("subnormal", h, w, t), ["subnormal"], f"subnormal, tensor {t}")
    _need(_classes("subnormal", h, w, 57), ["-0", "subnormal"], "subnormal, tensor 57")
    planted = cp.restated("subnormal", h, w).tensors[55]
    assert (np.abs(planted) < cp.TINY).any() and (np.abs(planted) >= cp.TINY).any(), "the planted values straddle 2^-126"
    r = cp.restated("subnormal", h, w).tensors[96][0]
    if r.shape[0] > 2 and r.shape[1] > 2:                     # (at 8x8 tensor 96 is one pixel)
        assert (cp._bits(r[1:-1, 1:-1]) == cp._bits(r[1, 1])).all() and (cp._bits(r[0, 0]) != cp._bits(r[1, 1])).any(), "conv 21: border against interior"


@pytest.mark.parametrize("h,w", cp.SIZES)
def test_certificate_overflow(h, w):
    for t in (56, 57):                                          # in front of the LeakyReLU and of the pool
        _need(_classes("overflow", h, w, t), ["finite", "+inf", "-inf", "nan"], f"overflow, tensor {t}")
    r = cp.restated("overflow", h, w)
    _need(_classes("overflow", h, w, 58), ["finite", "+inf", "-inf"], "overflow, tensor 58 (the concatenation's input)")
    nan_channel = np.isnan(r.tensors[57]).all(axis=(0, 1, 2))
    assert nan_channel.any() and (r.tensors[58][..., nan_channel] == -np.inf).all(), "a pool window that is all NaN gives -inf"
    assert np.isnan(r.tensors[62]).all() and cp.ranges_of(r.tensors)[62] == (np.inf, -np.inf), "tensor 62 is NaN at every element"
    assert (r.tensors[74] == -np.inf).all()
    _need(_classes("overflow_add", h, w, 67), ["finite", "+inf", "-inf", "nan"], "overflow_add, tensor 67 (the ADD's operand)")
    _need(_classes("overflow_add", h, w, 68), ["finite", "+inf", "-inf", "nan"], "overflow_add, tensor 68")
    assert np.isfinite(cp.restated("overflow_add", h, w).tensors[62]).all()


@pytest.mark.parametrize("h,w", cp.SIZES)
def test_certificate_overflow_gate(h, w):
    """the pack's frames make tensor 56 NaN at every element; frames with pixels in between do not"""
    r = cp.restated("overflow_gate", h, w)
    _need(cp.count_classes(r.tensors[55]), ["+inf", "-inf", "finite"], "overflow_gate, tensor 55")
    assert np.isnan(r.tensors[56]).all() and cp.ranges_of(r.tensors)[56] == (np.inf, -np.inf)
    grey = cp.evaluate(cp.pack("overflow_gate").convs, np.random.default_rng(5).integers(-64, 64, (1, h, w, 3), dtype=np.int8))
    assert np.isfinite(grey.tensors[56]).all()


SIGNED = ["tie, even below", "tie, odd below", "0.5", "below 0.5", "subnormal", "2^23 - 0.5", "2^23", "2^23 + 1", "2^24", "inf"]
BOUNDS = ["lo", "lo - 0.5", "lo - 1", "hi", "hi + 0.5", "hi + 1"]


def _rint_counts(name, tensor, h, w, scale=cp.RINT_SCALE, zp=cp.RINT_ZP):
    r = cp.restated(name, h, w)
    source = {103: 58}.get(tensor, tensor)                      # the QUANTIZE entry sees the pool's output
    return cp.rint_classes(r.tensors[source], scale, zp)


@pytest.mark.parametrize("h,w", cp.SIZES)
def test_certificate_rint(h, w):
    both = lambda names: [s + k for k in names for s in "+-"]
    head = {k: _rint_counts("rint_a", 100, h, w)[k] + _rint_counts("rint_b", 100, h, w)[k] for k in _rint_counts("rint_a", 100, h, w)}
    _need(head, both(SIGNED) + BOUNDS + ["nan"], "tensor 100 over rint_a and rint_b")
    # in front of a LeakyReLU: the 32 planted values themselves (a planted tensor holds no NaN and 2^23 + 1 is not among the 32) ...
    _need(_rint_counts("rint_a", 98, h, w), both(["tie, even below", "tie, odd below", "0.5", "below 0.5", "subnormal", "2^23 - 0.5", "2^24", "inf"])
          + ["lo", "lo - 0.5", "lo - 1", "hi", "hi + 0.5", "hi + 1", "+2^23", "+2^23 + 1"], "tensor 98 of rint_a")
    # ... and the NaN there comes from the overflow pack's tensor 56
    _need(_rint_counts("overflow", 56, h, w), ["nan", "+inf", "-inf"], "tensor 56 of overflow")
    # the QUANTIZE entry behind the pool, over the two pool sets: every class but the NaN (a pool never gives one) ...
    pool = {k: _rint_counts("rint_pool", 103, h, w)[k] + _rint_counts("rint_pool_b", 103, h, w)[k] for k in head}
    _need(pool, both([k for k in SIGNED if k != "inf"]) + BOUNDS, "tensor 58 over rint_pool and rint_pool_b")
    assert not pool["nan"]
    # ... with the infinite t under the table of scale 2^-100
    _need(_rint_counts("rint_pool", 103, h, w, 2.0 ** -100, 0), ["+inf", "-inf"], "tensor 58 of rint_pool at 2^-100")


def test_certificate_a_contracting_build_changes_the_shipped_tensors():
    for name in ("shipped_npz", "shipped_yfw"):
        a, b = cp.restated(name, 16, 24), cp.restated(name, 16, 24, "contracted")
        changed = [t for t in cp.slot_tensors() if not cp.same_floats(a.tensors[t], b.tensors[t])]
        assert len(changed) >= 40 and not cp.same_floats(a.logits, b.logits), (name, changed)
        assert cp.ranges_of(a.tensors) != cp.ranges_of(b.tensors)


def test_certificate_a_flushing_build_changes_a_logit_and_a_range_end():
    a, b = cp.restated("subnormal", 16, 24), cp.restated("subnormal", 16, 24, "flushed")
    assert not cp.same_floats(a.logits, b.logits)
    ra, rb = cp.ranges_of(a.tensors), cp.ranges_of(b.tensors)
    assert [t for t in ra if ra[t] != rb[t]], "no range end changed"
    assert cp.same_floats(cp.restated("shipped_yfw", 8, 8).logits, cp.restated("shipped_yfw", 8, 8, "flushed").logits)   # (and only there)


@pytest.mark.parametrize("name,h,w", CASES, ids=IDS)
def test_certificate_no_extreme_is_a_zero_of_either_sign(name, h, w):
    """The definition leaves the sign of a zero extreme to the order of the fold (t < v ? t : v keeps whichever zero came first).  Both
    builds report such a zero as +0 (they add +0 to every end) and calib_packs.ranges_of does the same, which alone removes the dependence
    on the fold's order from the comparisons here.  The packs do not lean on it either: no observed tensor that holds both zeros has a
    zero for its minimum or maximum, so every range end compared in these tests is decided by the values alone."""
    r = cp.restated(name, h, w)
    for t, v in r.tensors.items():
        c = cp.count_classes(v)
        if c["+0"] and c["-0"]:
            lo, hi = cp.ranges_of({t: v})[t]
            assert lo != 0 and hi != 0, (name, t, lo, hi)


# ---------------------------------------------------------------------------------------------------------------- the host build
@pytest.mark.parametrize("name,h,w", CASES, ids=IDS)
def test_tensors_and_records(name, h, w):
    p, x, want = cp.pack(name), cp.frames(name, h, w), cp.restated(name, h, w)
    entries, scales, zps, q = cp.compare_entries(name, h, w)
    el = [v.shape[1] for v in q]
    stats, totals, tensors = calib.host_compare(p.yfw, x, entries, threads=1, want_tensors=True, elements=el, general=True)
    xs = cp.flat_tensors(want)[1:]
    for t, got, ref in zip(cp.slot_tensors()[1:], tensors, xs):
        cp.assert_same_floats(got, ref, f"{name} {h}x{w}: tensor {t}")
    with np.errstate(all="ignore"):
        want_stats, want_totals = qs.restate(q, xs, scales, zps)
    cp.assert_same_records(stats, want_stats, f"{name} {h}x{w}: records")
    cp.assert_same_records(totals, want_totals, f"{name} {h}x{w}: totals")
    s2, t2 = calib.host_compare(p.yfw, x, entries, threads=2, general=(h, w) != (56, 56))       # (at 56x56 through the 56x56 entry)
    cp.assert_same_records(s2, want_stats, f"{name} {h}x{w}: records, two threads")
    cp.assert_same_records(t2, want_totals, f"{name} {h}x{w}: totals, two threads")


@pytest.mark.parametrize("name,h,w", CASES, ids=IDS)
def test_ranges_and_logits(name, h, w):
    p, x, want = cp.pack(name), cp.frames(name, h, w), cp.restated(name, h, w)
    for threads, general in ((1, True), (2, (h, w) != (56, 56))):
        ranges, logits = calib.host_run(p.yfw, x, threads=threads, general=general)
        cp.assert_same_ranges(ranges, cp.ranges_of(want.tensors), f"{name} {h}x{w}, {threads} threads")
        cp.assert_same_floats(logits, want.logits, f"{name} {h}x{w}: logits, {threads} threads")


@pytest.mark.parametrize("name,h,w", CASES, ids=IDS)
def test_simulation(name, h, w):
    p, x, ref = cp.pack(name), cp.frames(name, h, w), cp.restated(name, h, w).logits
    got, _ = calib.host_simulate(p.yfw, x, calib.empty_table(), general=True)
    cp.assert_same_floats(got, ref, f"{name} {h}x{w}: every entry disabled")
    for label, table in p.tables.items():
        want = cp.simulated(name, h, w, label)
        with np.errstate(all="ignore"):
            want_stats, want_totals = ss.restate(want.logits, ref, want.clipped)
        for threads in (1, 2):
            logits, totals, stats = calib.host_simulate(p.yfw, x, table, ref, threads=threads, general=True, want_stats=True)
            what = f"{name} {h}x{w}, table {label}, {threads} threads"
            cp.assert_same_floats(logits, want.logits, f"{what}: logits")
            assert stats["saturated"].tolist() == want.clipped.tolist(), f"{what}: clipped counts"
            cp.assert_same_records(stats, want_stats, f"{what}: records")
            cp.assert_same_records(totals, want_totals, f"{what}: totals")


def test_the_simulation_tables_clip_and_change_the_logits():
    """(a table that quantises nothing would make test_simulation a repeat of test_ranges_and_logits)"""
    for name in cp.NAMES:
        for label in cp.pack(name).tables:
            a, b = cp.restated(name, 16, 24), cp.simulated(name, 16, 24, label)
            assert b.clipped.sum() > 0 or not cp.same_floats(a.logits, b.logits), (name, label)
    assert all(cp.simulated(n, 16, 24, k).clipped.sum() > 0 for n, k in (("rint_a", "100"), ("rint_b", "100"), ("rint_a", "98"), ("rint_pool", "103"), ("rint_pool_b", "103"),
                                                                        ("overflow", "56")))
    assert not cp.same_floats(cp.restated("rint_pool", 16, 24).logits, cp.simulated("rint_pool", 16, 24, "103").logits)


@pytest.mark.parametrize("bins", [16, 4096])
@pytest.mark.parametrize("name,h,w", CASES, ids=IDS)
def test_histograms(name, h, w, bins):
    p, x, want = cp.pack(name), cp.frames(name, h, w), cp.restated(name, h, w)
    ranges = cp.inner_ranges(want)
    for threads in (1, 2):
        counts = calib.host_histogram(p.yfw, x, ranges, bins, threads=threads, general=True)
        hs.assert_same(counts, hs.restate(cp.flat_tensors(want), ranges, bins), f"{name} {h}x{w}, {bins} bins, {threads} threads")


def test_the_inner_ranges_leave_infinities_and_nans_to_the_end_bins():
    want = cp.restated("overflow", 16, 24)
    lo, hi = cp.inner_ranges(want)[57]
    v = want.tensors[57].reshape(-1)
    bins = hs.restate_bins(v, lo, hi, 16)
    assert np.isfinite([lo, hi]).all() and lo < hi
    assert (bins[np.isnan(v)] == 0).all() and (bins[v == -np.inf] == 0).all() and (bins[v == np.inf] == 15).all()
    assert np.isnan(v).any() and (v == np.inf).any() and (v == -np.inf).any()


# ---------------------------------------------------------------------------------------------------------------- ptq.quantize_model
def _good_ranges():
    return calib.host_run(cp.pack("shipped_yfw").yfw, cp.frames("shipped_yfw", 56, 56))[0]


@pytest.mark.parametrize("end,text", [((-1.0, np.inf), r"tensor 66: the range is \(-1\.0, inf\)"), ((-np.inf, 2.0), r"tensor 66: the range is \(-inf, 2\.0\)"),
                                      ((-np.inf, np.inf), r"tensor 66: the range is \(-inf, inf\)"), ((np.inf, -np.inf), r"tensor 66: the range is \(inf, -inf\)"),
                                      ((np.nan, 1.0), r"tensor 66: the range is \(nan, 1\.0\)"), ((2.0, 1.0), r"tensor 66: the range is \(2\.0, 1\.0\)")])
def test_quantize_model_refuses_a_range_that_is_not_finite_or_is_inverted(end, text):
    ranges = _good_ranges()
    assert len(ptq.quantize_model(cp.pack("shipped_yfw").yfw, ranges)) > 0
    ranges[66] = end
    with pytest.raises(ValueError, match=text):
        ptq.quantize_model(cp.pack("shipped_yfw").yfw, ranges)


def test_quantize_model_refuses_the_ranges_of_a_network_that_computes_nothing():
    """the host twin of calib.quantize_on_device on the overflow pack: calibration hands over infinite ends and, for the tensors that were NaN
    throughout, the sentinels"""
    p = cp.pack("overflow")
    ranges, _ = calib.host_run(p.yfw, cp.frames("overflow", 56, 56))
    assert ranges[62] == (np.inf, -np.inf) and ranges[57] == (-np.inf, np.inf)
    with pytest.raises(ValueError, match=r"ranges: tensor 56: the range is \(-inf, inf\), expected two finite numbers with min <= max"):
        ptq.quantize_model(p.yfw, ranges)
    for t in ranges:
        if not np.isfinite(ranges[t]).all():
            ranges[t] = (-1.0, 1.0) if t != 62 else ranges[t]
    with pytest.raises(ValueError, match=r"ranges: tensor 62: the range is \(inf, -inf\)"):
        ptq.quantize_model(p.yfw, ranges)
