"""The tracker on the CPU: the host build of csrc/yf_images_track.h (yf_images_track_host, libyf_images_host.so) against the plain-Python
statement `ptq.track_step`, exactly -- records, infos, counts, status and the whole state buffer, every array between guard bytes and
every place that must not be written a sentinel -- on the designed sequences of tests/track_support.py and on the seeded random ones;
both layouts; one call of F steps against F calls of one step; the argument checks.  No GPU."""
import numpy as np
import pytest

import track_support as ts
from images_support import ptq          # noqa: F401 (fixture)


@pytest.mark.parametrize("case", ts.designed(), ids=lambda c: c.name)
def test_host_build_equals_the_statement_on_the_designed_sequences(case):
    for layout in ts.LAYOUTS:
        dets, counts, streams, steps, state0 = ts.laid_out(case, layout)
        want = ts.expected(dets, counts, streams, steps, layout, case.cap, case.params, state0, case.out_cap)
        got = ts.host_run(dets, counts, streams, steps, layout, case.cap, case.params, state0, case.out_cap)
        assert got.rc == streams * steps and ts.same(got, want), (case.name, layout)
        # without a status array the rest is the same
        bare = ts.host_run(dets, counts, streams, steps, layout, case.cap, case.params, state0, case.out_cap, with_status=False)
        assert (bare.status == ts.SENTINEL32).all() and ts.same(bare._replace(status=want.status), want), (case.name, layout)


def test_the_designed_sequences_show_what_they_were_designed_for():
    """the statement itself, on the cases whose outcome can be said in a line"""
    by = {c.name: c for c in ts.designed()}

    def run(name, layout=ts.TIME):
        c = by[name]
        dets, counts, streams, steps, state0 = ts.laid_out(c, layout)
        return ts.expected(dets, counts, streams, steps, layout, c.cap, c.params, state0, c.out_cap)

    r = run("lifecycle")
    assert r.out_counts.tolist() == [0, 0, 2, 2, 2, 1, 1, 2, 2]                      # confirmed at the third hit; A held twice, then gone
    assert r.info[3, 0].tolist() == (1, 3, 1, 4) and r.info[4, 0].tolist() == (1, 3, 2, 5) and r.out[4, 0]["x1"] == 10
    assert r.info[5, 0]["id"] == 2 and r.info[7].tolist()[:2] == [(2, 8, 0, 8), (3, 3, 0, 3)]
    assert r.state["slot"]["id"][0, :3].tolist() == [3, 2, 0] and r.state["issued"][0] == 3           # C in A's slot, id 1 not reissued
    r = run("tie")
    assert [(int(d["x1"]), int(d["y1"])) for d in r.out[1, :2]] == [(6, 2), (6, -2)] and r.info[1, :2]["hits"].tolist() == [2, 2]
    assert [(int(d["x1"]), int(d["y1"])) for d in r.out[2, :2]] == [(10, 0), (2, 0)]                   # detection 0 to slot 0 again
    r = run("global_greedy")
    assert [int(d["x1"]) for d in r.out[1, :2]] == [2, 10] and r.out_counts[1] == 2
    r = run("full")
    assert r.status.tolist() == [0, 2, 0] and r.out_counts.tolist() == [64, 64, 64] and r.state["issued"][0] == 64
    r = run("counts", ts.STREAM)
    assert r.status.tolist() == [1, 0, 0, 0, 0, 1, 0, 0] and r.out_counts[0] == 10
    r = run("counts64")
    assert r.status.tolist() == [1, 1, 3] and r.out_counts[0] == 64                             # six new ones in the reversed row find no slot
    r = run("out_cap")
    assert r.out_counts.tolist() == [5, 5] and (r.out[:, 2:].view(np.uint8) == 0xA5).all() and r.info[1, 0]["misses"] == 1
    r = run("extremes")
    assert r.out_counts.tolist() == [10, 14, 14, 10, 0] and r.state["issued"][0] == 18               # the four improper boxes: born anew each time
    r = run("iou0")
    assert r.info[1]["id"][:3].tolist() == [1, 3] + [ts.SENTINEL32 & 0xFFFFFFFF] and r.out_counts[1] == 2
    r = run("iou1")
    assert r.info[1]["id"][:2].tolist() == [1, 3]
    r = run("wrap")
    assert r.info[0]["id"][:3].tolist() == [1, 2, 0xFFFFFFFF] and r.state["issued"][0] == 2 and r.state["reserved"][0] == 0xDEADBEEF
    assert run("wrap_at_max").info[0]["id"][:3].tolist() == [1, 2, 9]
    r = run("saturate")
    assert r.info[1, 0].tolist() == (4, ts.I32MAX, 0, ts.I32MAX) and r.info[1, 1].tolist() == (5, ts.I32MAX, 0, ts.I32MAX) and r.out_counts[0] == 2
    assert run("saturate_kept").info[0, 2].tolist() == (6, 3, ts.I32MAX, ts.I32MAX)
    r = run("misses")
    assert [i.tolist() for i in r.info[0, :2]] == [(4, 2, -4, 10), (5, 3, 0, 10)] and r.out_counts.tolist() == [2, 2, 2]
    assert r.state["slot"]["id"][0, :4].tolist() == [4, 5, 0, 0] and r.state["slot"]["misses"][0, 0] == -2
    r = run("dirty")
    assert r.info[0]["id"][:2].tolist() == [9, 9] and [int(d["x1"]) for d in r.out[0, :2]] == [100, 60]
    assert r.state["slot"][0, 0].tolist()[:4] == (21, 1, 0, 1) and r.state["slot"][0, 4].tolist()[:4] == (0, -1, -1, -1)


def test_host_build_equals_the_statement_on_the_random_sequences():
    for layout in ts.LAYOUTS:
        dets, counts, want = ts.random_call(layout)
        got = ts.host_run(dets, counts, ts.R_STREAMS, ts.R_STEPS, layout, ts.R_CAP, ts.R_PARAMS, ts.empty_state(ts.R_STREAMS), ts.R_OUT_CAP)
        assert got.rc == ts.R_STREAMS * ts.R_STEPS and ts.same(got, want), layout


def test_both_layouts_give_the_same_frames():
    a = ts.host_run(*ts.random_call(ts.TIME)[:2], ts.R_STREAMS, ts.R_STEPS, ts.TIME, ts.R_CAP, ts.R_PARAMS, ts.empty_state(ts.R_STREAMS), ts.R_OUT_CAP)
    b = ts.host_run(*ts.random_call(ts.STREAM)[:2], ts.R_STREAMS, ts.R_STEPS, ts.STREAM, ts.R_CAP, ts.R_PARAMS, ts.empty_state(ts.R_STREAMS),
                    ts.R_OUT_CAP)
    assert ts.by_frame(a, ts.R_STREAMS, ts.R_STEPS, ts.TIME) == ts.by_frame(b, ts.R_STREAMS, ts.R_STEPS, ts.STREAM)
    assert a.out.tobytes() != b.out.tobytes()


def test_one_call_of_many_steps_equals_many_calls_of_one():
    dets, counts, want = ts.random_call(ts.TIME)
    got = ts.split_calls(ts.host_run, dets, counts, ts.R_STREAMS, ts.R_STEPS, ts.R_CAP, ts.R_PARAMS, ts.empty_state(ts.R_STREAMS), ts.R_OUT_CAP)
    assert ts.same(got, want)


def test_the_argument_check_rejects_every_fault():
    assert ts.host_check() == "" and ts.host_check(streams=0) == "" and ts.host_check(steps=0, status=8) == ""
    assert ts.host_check(params=(float("inf"), 1, 0)) == "" and ts.host_check(params=(-2.0, ts.I32MAX, ts.I32MAX), cap=1200, out_cap=ts.I32MAX) == ""
    assert ts.host_check(streams=2 ** 31 - 2, steps=1) == "" and ts.host_check(streams=46340, steps=46340) == ""
    for kw, text in ts.FAULTS:
        assert text in ts.host_check(**kw), (kw, ts.host_check(**kw))
    # the entry refuses what the check refuses and writes nothing; an empty batch is taken after the checks and writes nothing either
    case = ts.designed()[0]
    dets, counts, streams, steps, state0 = ts.laid_out(case, ts.TIME)
    for params, cap, out_cap in (((float("nan"), 1, 1), case.cap, 4), ((0.3, 0, 1), case.cap, 4), ((0.3, 1, 1), 0, 4), ((0.3, 1, 1), case.cap, 0)):
        r = ts.host_run(dets, counts, streams, steps, ts.TIME, cap, params, state0, out_cap)
        assert r.rc == -1 and r.state.tobytes() == state0.tobytes() and (r.out_counts == ts.SENTINEL32).all(), (params, cap, out_cap)
        assert (r.out.view(np.uint8) == 0xA5).all() and (r.status == ts.SENTINEL32).all(), (params, cap, out_cap)
    for streams0, steps0 in ((0, 5), (1, 0), (0, 0)):
        r = ts.host_run(dets, counts, streams0, steps0, ts.TIME, case.cap, case.params, state0, 4)
        assert r.rc == 0 and r.state.tobytes() == state0.tobytes() and (r.out_counts == ts.SENTINEL32).all()
        assert (r.out.view(np.uint8) == 0xA5).all()
    assert ts.track_host().yf_images_track_state_bytes_host(3) == 3 * 2824 and ts.track_host().yf_images_track_state_bytes_host(-1) == 0
