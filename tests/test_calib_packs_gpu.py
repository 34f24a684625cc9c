"""libyf_calib.so on the designed weight packs of calib_packs.py: the device against the numpy restatement of the defined arithmetic and
against the host build, exactly -- ranges and logits, histograms, comparison records, simulated logits and clipped counts -- where the
tensors hold subnormals, -0, +-inf and NaN and the simulated quantiser meets every edge of its rounding.  This is where a device build that
contracted to fma, flushed float32 subnormals, rounded a tie another way or let a NaN into an extreme would show.  Each pack runs at 56x56
in the LDS form and in the general form, and in the general form at 8x8 and 16x24; three frames, one black and one white.  No tolerance: a
value differs only where both sides are NaN (calib_packs.same_floats)."""
import functools

import numpy as np
import pytest

import calib_packs as cp
import calib_hist_support as hs
import calib_sim_support as ss
import calib_support as cs
import quant_support as qs
from calib_support import calib

pytestmark = pytest.mark.gpu
FORMS = ((56, 56, False), (56, 56, True), (8, 8, True), (16, 24, True))
CASES = [(name,) + f for name in cp.NAMES for f in FORMS]
IDS = [f"{name}-{h}x{w}-{'general' if g else 'lds'}" for name, h, w, g in CASES]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def handles(torch_cuda):
    """one Calibration per pack"""
    made = {}
    try:
        for name in cp.NAMES:
            made[name] = calib.Calibration(cp.pack(name).yfw)
        yield made
    finally:
        for c in made.values():
            c.destroy()


def _device(torch, a):
    return torch.from_numpy(np.array(a)).cuda()


@functools.lru_cache(maxsize=None)
def _host_run(name, h, w):
    return calib.host_run(cp.pack(name).yfw, cp.frames(name, h, w), threads=3, general=True)


@pytest.mark.parametrize("name,h,w,general", CASES, ids=IDS)
def test_observe(handles, torch_cuda, name, h, w, general):
    cal, want = handles[name], cp.restated(name, h, w)
    cal.reset()
    assert cal.observe(_device(torch_cuda, cp.frames(name, h, w)), general=general) == cp.N_FRAMES == cal.frames_observed
    ranges, logits = cal.ranges(), cal.logits.cpu().numpy()
    cp.assert_same_ranges(ranges, cp.ranges_of(want.tensors), f"{name}: ranges against the restatement")
    cp.assert_same_ranges(ranges, _host_run(name, h, w)[0], f"{name}: ranges against the host build")
    cp.assert_same_floats(logits, want.logits, f"{name}: logits against the restatement")
    cp.assert_same_floats(logits, _host_run(name, h, w)[1], f"{name}: logits against the host build")


@pytest.mark.parametrize("name,h,w,general", CASES, ids=IDS)
def test_histogram(handles, torch_cuda, name, h, w, general):
    cal, want = handles[name], cp.restated(name, h, w)
    d_x, ranges = _device(torch_cuda, cp.frames(name, h, w)), cp.inner_ranges(want)
    for bins in (16, 4096):
        got = cal.histogram(d_x, ranges, bins, general=general).cpu().numpy()
        hs.assert_same(got, hs.restate(cp.flat_tensors(want), ranges, bins), f"{name}, {bins} bins: against the restatement")
        hs.assert_same(got, calib.host_histogram(cp.pack(name).yfw, cp.frames(name, h, w), ranges, bins, threads=3, general=True),
                       f"{name}, {bins} bins: against the host build")


@pytest.mark.parametrize("name,h,w,general", CASES, ids=IDS)
def test_compare(handles, torch_cuda, name, h, w, general):
    cal, want = handles[name], cp.restated(name, h, w)
    entries, scales, zps, q = cp.compare_entries(name, h, w)
    d_q = [_device(torch_cuda, v) for v in q]
    d_entries = [calib.Entry(e.tensor, e.scale, e.zero_point, d, d.stride(0)) for e, d in zip(entries, d_q)]
    d_stats, totals = cal.compare(_device(torch_cuda, cp.frames(name, h, w)), d_entries, general=general)
    stats = calib.frame_stats_array(d_stats)
    with np.errstate(all="ignore"):
        want_stats, want_totals = qs.restate(q, cp.flat_tensors(want)[1:], scales, zps)
    cp.assert_same_records(stats, want_stats, f"{name}: records against the restatement")
    cp.assert_same_records(totals, want_totals, f"{name}: totals against the restatement")
    host_stats, host_totals = calib.host_compare(cp.pack(name).yfw, cp.frames(name, h, w), entries, threads=3, general=True)
    cp.assert_same_records(stats, host_stats, f"{name}: records against the host build")
    cp.assert_same_records(totals, host_totals, f"{name}: totals against the host build")


@pytest.mark.parametrize("name,h,w,general", CASES, ids=IDS)
def test_simulate(handles, torch_cuda, name, h, w, general):
    cal, p, x, ref = handles[name], cp.pack(name), cp.frames(name, h, w), cp.restated(name, h, w).logits
    d_x = _device(torch_cuda, x)
    off, _ = cal.simulate(d_x, calib.empty_table(), general=general)
    cp.assert_same_floats(off.cpu().numpy(), ref, f"{name}: every entry disabled")
    for label, table in p.tables.items():
        want, what = cp.simulated(name, h, w, label), f"{name}, table {label}"
        with np.errstate(all="ignore"):
            want_stats, want_totals = ss.restate(want.logits, ref, want.clipped)
        d_logits, totals, d_stats = cal.simulate(d_x, table, ref, general=general, want_stats=True)
        logits, stats = d_logits.cpu().numpy(), calib.frame_stats_array(d_stats)[:, 0]
        cp.assert_same_floats(logits, want.logits, f"{what}: logits against the restatement")
        assert stats["saturated"].tolist() == want.clipped.tolist(), f"{what}: clipped counts"
        cp.assert_same_records(stats, want_stats, f"{what}: records against the restatement")
        cp.assert_same_records(totals, want_totals, f"{what}: totals against the restatement")
        host_logits, host_totals, host_stats = calib.host_simulate(p.yfw, x, table, ref, threads=3, general=True, want_stats=True)
        cp.assert_same_floats(logits, host_logits, f"{what}: logits against the host build")
        cp.assert_same_records(stats, host_stats, f"{what}: records against the host build")
        cp.assert_same_records(totals, host_totals, f"{what}: totals against the host build")


@pytest.mark.parametrize("general", [False, True], ids=["lds", "general"])
def test_a_slot_that_saw_only_nan_takes_the_range_of_later_frames(handles, torch_cuda, general):
    """overflow_gate's frames leave tensor 56 NaN at every element: its slot keeps (+inf, -inf).  Real frames observed after them on the same
    handle give it their range, and every other slot the union.  The pack is overflow_gate and not overflow: overflow's NaN comes from
    planted biases, so its tensors are NaN on any frame and no later frame could fill the slot; overflow_gate's depends on the pixels."""
    cal, p = handles["overflow_gate"], cp.pack("overflow_gate")
    first, real = cp.restated("overflow_gate", 56, 56), cp.evaluate(p.convs, cs.calib_frames()[:3])
    assert np.isnan(real.tensors[56]).any() and np.isfinite(real.tensors[56]).any()
    cal.reset()
    cal.observe(_device(torch_cuda, cp.frames("overflow_gate", 56, 56)), general=general)
    assert cal.ranges()[56] == (np.inf, -np.inf)
    cal.observe(_device(torch_cuda, cs.calib_frames()[:3]), general=general)
    a, b = cp.ranges_of(first.tensors), cp.ranges_of(real.tensors)
    want = {t: (min(a[t][0], b[t][0]), max(a[t][1], b[t][1])) for t in a}
    got = cal.ranges()
    cp.assert_same_ranges(got, want, "the pack's frames, then real frames")
    assert got[56] == b[56] and np.isfinite(got[56]).all() and cal.frames_observed == 6
    cp.assert_same_floats(cal.logits.cpu().numpy(), real.logits, "the real frames' logits")
