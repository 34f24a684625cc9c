"""Per-tensor quantisation error, host build (libyf_calib_host.so): yf_calib_host_compare on the oracle's per-op dump of the 27 calibration
frames.  Its float32 tensors are tied to what yf_calib_host_run gives; its records and totals are required to equal, bit for bit, a numpy
restatement of the defined order (quant_support.restate); designed inputs pin the meaning of every field; every refusal is read."""
import numpy as np
import pytest

import calib_support as cs
import quant_support as qs
from calib_support import calib

N = 27


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_the_covered_tensors_come_from_the_graph_and_the_dump():
    """27 dumped tensors the float evaluation has, and the head: among them one with fewer than 1024 elements and one whose count is no
    multiple of 1024.  QUANTIZE and CONCATENATION records (ops 21, 22, 45, 46) have no tensor in the evaluation."""
    T = qs.tensors()
    assert len(T) == 28 and T[-1]["tensor"] == 100 and T[-1]["offset"] is None and T[-1]["op"] == 53
    assert [t["op"] for t in T] == sorted(t["op"] for t in T)
    assert not {21, 22, 45, 46} & {t["op"] for t in T}
    assert all(qs.dump_offset()(op) >= 0 for op in (21, 22, 45, 46)) and qs.dump_offset()(53) == -1 and qs.dump_offset()(0) == -1
    el = {t["tensor"]: t["elements"] for t in T}
    assert el[78] == 7 * 7 * 8 < 1024 and el[57] == 28 * 28 * 18 and el[57] % 1024 != 0 and el[100] == 882


def test_tensors_out_is_the_evaluation_of_host_run():
    ranges, logits = cs.host_result(qs.WEIGHTS)
    _, _, xs = qs.real_host()
    assert np.array_equal(_bits(xs[-1]).reshape(N, 7, 7, 18), _bits(logits))
    for t, x in zip(qs.tensors(), xs):
        assert x.shape == (N, t["elements"])
        lo, hi = ranges[t["tensor"]]
        assert (float(x.min()), float(x.max())) == (lo, hi), f"tensor {t['tensor']}"


@pytest.mark.parametrize("threads", [1, 16])
def test_records_and_totals_equal_the_restatement(threads):
    q = qs.oracle_q(*qs.real_run())
    _, _, xs = qs.real_host()
    want_s, want_t = qs.restate(q, xs, [t["scale"] for t in qs.tensors()], [t["zero_point"] for t in qs.tensors()])
    got_s, got_t = calib.host_compare(cs.yfw_bytes(qs.WEIGHTS), cs.calib_frames(), qs.entries_over(q), threads=threads)
    qs.same_records(got_s, want_s, f"records, {threads} thread(s)")
    qs.same_records(got_t, want_t, f"totals, {threads} thread(s)")
    assert (got_t["elements"] == np.array(qs.elements()) * N).all() and (got_t["sum_sq_err"] > 0).all()


def test_q_in_a_strided_buffer_equals_q_in_a_packed_one():
    """frame_stride is honoured: the entries read out of the oracle's dump in place (one frame's record after the other)"""
    import model_variants as mv
    heads, dump = qs.real_run()
    _, offs, _ = mv.dump_layout()
    in_place = [calib.Entry(t["tensor"], t["scale"], t["zero_point"], heads if t["offset"] is None else dump[:, offs[t["op"]]:],
                            heads.strides[0] if t["offset"] is None else dump.strides[0]) for t in qs.tensors()]
    got_s, got_t = calib.host_compare(cs.yfw_bytes(qs.WEIGHTS), cs.calib_frames(), in_place, threads=16)
    qs.same_records(got_s, qs.real_host()[0], "records")
    qs.same_records(got_t, qs.real_host()[1], "totals")


def test_designed_inputs():
    _, _, xs = qs.real_host()
    which = list(range(len(qs.tensors())))
    # q = 0 at zero point 0: the error is -x
    zeros = [np.zeros(x.shape, np.int8) for x in xs]
    s, t = calib.host_compare(cs.yfw_bytes(qs.WEIGHTS), cs.calib_frames(), qs.entries_over(zeros, which, zero_point=[0] * len(which)), threads=16)
    assert np.array_equal(s["sum_sq_err"].view(np.uint64), s["sum_sq_ref"].view(np.uint64))
    assert np.array_equal(t["sum_sq_err"].view(np.uint64), t["sum_sq_ref"].view(np.uint64))
    assert np.array_equal(_bits(t["max_abs_err"]), _bits([np.abs(x).max() for x in xs])) and (t["saturated"] == 0).all()
    # the exact nearest quantisation at a scale that clips nothing (a power of two at least max|x| / 126: x / scale, q * scale and the
    # rounding of d - x, which is monotone, are then exact, so the bound holds without an allowance)
    scales = [np.float32(2.0 ** int(np.ceil(np.log2(np.abs(x).max() / 126.0)))) for x in xs]
    near = [np.rint(x.astype(np.float64) / float(sc)).astype(np.int8) for x, sc in zip(xs, scales)]
    assert all(np.abs(q.astype(np.int32)).max() <= 126 for q in near)
    s, t = calib.host_compare(cs.yfw_bytes(qs.WEIGHTS), cs.calib_frames(), qs.entries_over(near, which, scale=scales, zero_point=[0] * len(which)),
                              threads=16)
    assert (t["max_abs_err"] <= np.array(scales) / 2).all() and (t["max_abs_err"] > np.array(scales) / 4).all()
    assert (t["saturated"] == 0).all() and (s["saturated"] == 0).all()
    # a constant 127: every element is saturated
    top = [np.full(x.shape, 127, np.int8) for x in xs]
    s, t = calib.host_compare(cs.yfw_bytes(qs.WEIGHTS), cs.calib_frames(), qs.entries_over(top), threads=16)
    assert (t["saturated"] == np.array(qs.elements()) * N).all() and (s["saturated"] == np.array(qs.elements())[None, :]).all()
    low = [np.full(x.shape, -128, np.int8) for x in xs[:2]]
    assert (calib.host_compare(cs.yfw_bytes(qs.WEIGHTS), cs.calib_frames(), qs.entries_over(low, [0, 1]))[1]["saturated"]
            == np.array(qs.elements()[:2]) * N).all()


def test_a_single_entry_and_another_order():
    q = qs.oracle_q(*qs.real_run())
    want_s, want_t = qs.real_host()[:2]
    k = [t["tensor"] for t in qs.tensors()].index(57)
    s, t = calib.host_compare(cs.yfw_bytes(qs.WEIGHTS), cs.calib_frames(), qs.entries_over([q[k]], [k]))
    qs.same_records(s, want_s[:, k:k + 1], "tensor 57 alone")
    qs.same_records(t, want_t[k:k + 1], "tensor 57 alone, totals")
    order = list(range(len(q)))[::-1]
    s, t, xs = calib.host_compare(cs.yfw_bytes(qs.WEIGHTS), cs.calib_frames()[:3], qs.entries_over([q[i][:3] for i in order], order), threads=2,
                                  want_tensors=True, elements=[qs.elements()[i] for i in order])
    qs.same_records(s, np.ascontiguousarray(want_s[:3, order]), "entries in reverse order")
    for x, i in zip(xs, order):
        assert np.array_equal(_bits(x), _bits(qs.real_host()[2][i][:3]))


def _refused(entries, match, frames=None):
    with pytest.raises(calib.CalibError, match=match):
        calib.host_compare(cs.yfw_bytes(qs.WEIGHTS), cs.calib_frames()[:2] if frames is None else frames, entries)


def test_every_refusal_names_entry_field_found_and_expected():
    q = [a[:2] for a in qs.oracle_q(*qs.real_run())]
    E = qs.entries_over(q)
    k57 = [t["tensor"] for t in qs.tensors()].index(57)
    _refused([E[0], E[1]._replace(tensor=0)], r"entry 1: tensor is 0, expected one of the 46 tensors")
    _refused([E[0]._replace(tensor=59)], r"entry 0: tensor is 59, expected one of the 46 tensors")
    _refused([E[0]._replace(tensor=-1)], r"entry 0: tensor is -1, expected one of the 46 tensors")
    _refused([E[0]._replace(tensor=101)], r"entry 0: tensor is 101, expected one of the 46 tensors")
    _refused([E[0], E[1], E[0]], rf"entry 2: tensor is {E[0].tensor}, which entry 0 lists already")
    for bad, text in ((0.0, "0"), (-0.5, "-0.5"), (float("inf"), "inf"), (float("nan"), "-?nan")):
        _refused([E[0], E[1], E[2]._replace(scale=bad)], rf"entry 2: scale is {text}, expected a finite positive float32")
    _refused([E[0]._replace(zero_point=128)], r"entry 0: zero_point is 128, expected -128 to 127")
    _refused([E[0], E[1]._replace(zero_point=-129)], r"entry 1: zero_point is -129, expected -128 to 127")
    _refused([E[3]._replace(q=None)], rf"entry 0: q is NULL, expected the int8 values of tensor {E[3].tensor}")
    _refused([E[k57]._replace(frame_stride=28 * 28 * 18 - 1)], r"entry 0: frame_stride is 14111, expected at least the 14112 elements of tensor 57")
    _refused([], r"compare: count is 0, expected 1 to 46")
    _refused([E[0]] * 47, r"compare: count is 47, expected 1 to 46")
    _refused(E[:1], r"compare: n is 0, expected at least 1", frames=np.zeros((0, 56, 56, 3), np.int8))
    bad = bytearray(cs.yfw_bytes(qs.WEIGHTS))
    bad[8 + 16] = 1
    with pytest.raises(calib.CalibError, match="conv 0: stride is 1, expected 2"):
        calib.host_compare(bytes(bad), cs.calib_frames()[:1], [e._replace(q=e.q[:1]) for e in E[:1]])
