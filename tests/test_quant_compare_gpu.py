"""Per-tensor quantisation error on the GPU: yf_calib_compare_device against the host build bit for bit (the same IEEE operations in the defined
order, csrc/yf_calib_compare.h), over the oracle's dump and over the engine's own (yf_network_dump_offset), and the table
calib.quantisation_report makes of the shipped model."""
import numpy as np
import pytest

import calib_support as cs
import model_variants as mv
import quant_support as qs
from calib_support import calib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def cal(torch_cuda):
    c = calib.Calibration(cs.yfw_bytes(qs.WEIGHTS))
    yield c
    c.destroy()


def _cases():
    x = cs.calib_frames()
    return [("n=1", x[:1]), ("n=3", x[:3]), ("27 real frames", x), ("structured extremes", mv.structured_extreme_frames()),
            ("257 random frames", np.random.default_rng(257).integers(-128, 128, (257, 56, 56, 3), dtype=np.int8))]


def _device_entries(torch, q, which=None):
    """the host arrays q[i] uploaded, and the entries over them"""
    d_q = [torch.from_numpy(a).cuda() for a in q]
    idx = range(len(qs.tensors())) if which is None else which
    return d_q, [calib.Entry(qs.tensors()[i]["tensor"], qs.tensors()[i]["scale"], qs.tensors()[i]["zero_point"], d, d.stride(0)) for d, i in zip(d_q, idx)]


def _same_as_host(got, want, what):
    d_stats, totals = got
    qs.same_records(calib.frame_stats_array(d_stats), want[0], what + ": records")
    qs.same_records(totals, want[1], what + ": totals")


@pytest.mark.parametrize("what,frames", _cases(), ids=[c[0] for c in _cases()])
def test_records_and_totals_equal_the_host_build(cal, torch_cuda, what, frames):
    """all 28 entries over the oracle's dump.  257 frames are more than the compute units: a workgroup runs a second frame, with accumulators
    that must have been reset"""
    q = qs.oracle_q(*qs.oracle_run(frames))
    want = calib.host_compare(cs.yfw_bytes(qs.WEIGHTS), frames, qs.entries_over(q), threads=16)
    d_q, entries = _device_entries(torch_cuda, q)
    _same_as_host(cal.compare(frames, entries), want, what)


def test_the_engines_own_dump_at_the_exported_offsets(cal, network, torch_cuda):
    """q read in place out of yf_network_run_device_dump's records: every slice at yf_network_dump_offset is the oracle's dump of that op, and
    the comparison over them equals the host build's over the oracle's"""
    torch = torch_cuda
    x = cs.calib_frames()
    heads, dump = qs.real_run()
    sizes, offs, _ = mv.dump_layout()
    d_x = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_out = torch.zeros((27, calib.LOGITS), dtype=torch.int8, device="cuda")
    d_dump = torch.zeros((27, network.dump_bytes()), dtype=torch.int8, device="cuda")
    network.run_device(d_x.data_ptr(), d_out.data_ptr(), 27, None, d_dump.data_ptr())
    torch.cuda.synchronize()
    got = d_dump.cpu().numpy()
    entries = []
    for t in qs.tensors():
        if t["offset"] is None:
            assert np.array_equal(d_out.cpu().numpy(), heads)
            entries.append(calib.Entry(t["tensor"], t["scale"], t["zero_point"], d_out.data_ptr(), calib.LOGITS))
            continue
        off, op = network.dump_offset(t["op"]), t["op"]
        assert off == t["offset"] and 0 <= off and off + sizes[op] <= network.dump_bytes()
        d = mv.first_difference(got[:, off:off + sizes[op]], dump[:, offs[op]:offs[op] + sizes[op]], mv.dump_layout()[2][op])
        assert d is None, f"tflite op {op} at dump offset {off} differs first at (frame, y, x, channel) = {d[:4]}: got {d[4]}, oracle {d[5]}"
        entries.append(calib.Entry(t["tensor"], t["scale"], t["zero_point"], d_dump.data_ptr() + off, network.dump_bytes()))
    assert len(entries) == 28 and network.dump_offset(53) == -1 and network.dump_offset(-1) == -1 and network.dump_offset(54) == -1
    _same_as_host(cal.compare(d_x, entries), qs.real_host()[:2], "the engine's dump")


def test_a_single_entry_a_stream_of_its_own_and_two_calls_back_to_back(cal, torch_cuda):
    torch = torch_cuda
    x = cs.calib_frames()
    want_s, want_t = qs.real_host()[:2]
    q = qs.oracle_q(*qs.real_run())
    d_x = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    k = [t["tensor"] for t in qs.tensors()].index(78)
    d_one, one = _device_entries(torch, [q[k]], [k])
    _same_as_host(cal.compare(d_x, one), (want_s[:, k:k + 1], want_t[k:k + 1]), "tensor 78 alone")
    d_q, entries = _device_entries(torch, q)
    side = torch.cuda.Stream()
    _same_as_host(cal.compare(d_x, entries, stream=side.cuda_stream), (want_s, want_t), "a stream of its own")
    # two calls on one stream with nothing between them, through the C interface: the first half of the entries, then the second half
    half = len(entries) // 2
    parts = [(entries[:half], slice(0, half)), (entries[half:], slice(half, len(entries)))]
    outs = []
    torch.cuda.synchronize()
    for part, _ in parts:
        d_stats = torch.zeros((27, len(part), 32), dtype=torch.uint8, device="cuda")
        d_totals = torch.zeros((len(part), 48), dtype=torch.uint8, device="cuda")
        outs.append((d_stats, d_totals))
    torch.cuda.synchronize()
    for (part, _), (d_stats, d_totals) in zip(parts, outs):
        rc = cal._lib.yf_calib_compare_device(cal.handle, d_x.data_ptr(), 27, calib._qtensors(part), len(part), d_stats.data_ptr(), d_totals.data_ptr(),
                                              side.cuda_stream)
        assert rc == 27, cal._text()
    side.synchronize()
    for (_, sl), (d_stats, d_totals) in zip(parts, outs):
        got_t = d_totals.cpu().numpy().view(calib.TOTALS).reshape(-1)
        _same_as_host((d_stats, got_t), (np.ascontiguousarray(want_s[:, sl]), want_t[sl]), f"back to back, entries {sl}")
    # d_totals is optional
    d_stats = torch.zeros((27, 1, 32), dtype=torch.uint8, device="cuda")
    assert cal._lib.yf_calib_compare_device(cal.handle, d_x.data_ptr(), 27, calib._qtensors(one), 1, d_stats.data_ptr(), None, None) == 27
    torch.cuda.synchronize()
    qs.same_records(calib.frame_stats_array(d_stats), np.ascontiguousarray(want_s[:, k:k + 1]), "no totals")


def test_a_compare_leaves_ranges_and_frames_observed_alone(cal, torch_cuda):
    x = cs.calib_frames()
    d_q, entries = _device_entries(torch_cuda, qs.oracle_q(*qs.real_run()))
    cal.reset()
    cal.compare(x[:3], [e._replace(q=e.q[:3]) for e in entries])
    with pytest.raises(calib.CalibError, match="no frame has been observed yet"):
        cal.ranges()
    assert cal.frames_observed == 0
    cal.observe(x[:5])
    before = cal.ranges()
    assert before == calib.host_run(cs.yfw_bytes(qs.WEIGHTS), x[:5])[0]
    cal.compare(x, entries)
    assert cal.frames_observed == 5 and cal.ranges() == before
    cal.reset()


def test_a_refusal_carries_the_validations_text(cal, torch_cuda):
    """the one validation function serves both builds (its texts are read one by one in test_quant_compare_host.py)"""
    d_q, entries = _device_entries(torch_cuda, [a[:2] for a in qs.oracle_q(*qs.real_run())])
    x = cs.calib_frames()[:2]
    for bad, text in (([entries[0], entries[0]], r"entry 1: tensor is \d+, which entry 0 lists already"),
                      ([entries[1]._replace(scale=float("inf"))], r"entry 0: scale is inf, expected a finite positive float32"),
                      ([entries[1]._replace(frame_stride=3)], r"entry 0: frame_stride is 3, expected at least the \d+ elements of tensor"),
                      ([entries[1]._replace(q=None)], r"entry 0: q is NULL"), ([], r"compare: count is 0, expected 1 to 46")):
        with pytest.raises(calib.CalibError, match=text):
            cal.compare(x, bad)
    with pytest.raises(calib.CalibError, match=r"compare: n is 0, expected at least 1"):
        cal.compare(np.zeros((0, 56, 56, 3), np.int8), entries)


def test_quantisation_report_of_the_shipped_model(network, torch_cuda):
    """The head's row against an independent numpy computation (Calibration.logits, the engine's heads, the restated order), and its
    maximum error in LSB against the figure profiles/calib_accuracy.txt records for the same weights and frames, to the digits printed there."""
    torch = torch_cuda
    x = cs.calib_frames()
    rows = calib.quantisation_report(network, cs.yfw_bytes(qs.WEIGHTS), qs.shipped_yfm(), x)
    assert [(r["tensor"], r["op"]) for r in rows] == [(t["tensor"], t["op"]) for t in qs.tensors()] and len(rows) == 28
    assert all(r["elements"] == t["elements"] * 27 for r, t in zip(rows, qs.tensors()))
    c = calib.Calibration(cs.yfw_bytes(qs.WEIGHTS))
    try:
        c.observe(x)
        logits = c.logits.cpu().numpy().reshape(27, -1)
    finally:
        c.destroy()
    d_x = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_out = torch.zeros((27, calib.LOGITS), dtype=torch.int8, device="cuda")
    network.run_device(d_x.data_ptr(), d_out.data_ptr(), 27)
    torch.cuda.synchronize()
    head = qs.tensors()[-1]
    _, want = qs.restate([d_out.cpu().numpy()], [logits], [head["scale"]], [head["zero_point"]])
    want_row = calib.report_rows([head], want)[0]
    assert rows[-1] == want_row, (rows[-1], want_row)
    printed, half_digit = qs.printed_head_lsb()
    lsb = rows[-1]["max_abs_error"] / rows[-1]["scale"]
    print(f"head: max_abs_error / scale = {lsb:.6f} LSB, printed {printed}")
    for r in rows:
        print({k: (round(v, 6) if isinstance(v, float) else v) for k, v in r.items()})
    assert abs(lsb - printed) <= half_digit, (lsb, printed)
    assert rows[-1]["saturated"] == 0.0 and all(np.isfinite(r["sqnr_db"]) and r["rmse_over_scale"] > 0 for r in rows)
