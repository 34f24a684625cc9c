"""The score of tracks against labelled identities on the CPU: the host build of csrc/yf_images_score.h (libyf_images_host.so) against
`ptq.track_score_step`, the plain-Python statement, exactly -- the whole state, the matches and the status, every array between guard
bytes and every place that must not be written a sentinel -- on the designed scenes (the hand-counted exchange of two ids, continuity
against the optimum, two rows with the same last hypothesis, an object that returns, void rows and records, counts above the caps, empty
rows, score_iou 0 and 1), on every number of rows against every number of columns, the 64 x 64 table of equal weights and the staircase,
1, 3 and 5 streams by 1 and 7 steps in both layouts, states of random bytes and counters at their extremes; the summary against
`ptq.track_score_summary`, the two doubles bit for bit; one case per argument check; and the tracker's host build scored on the pan
stream, where the greedy match switches identities and the optimal assignment does not.  No GPU."""
import numpy as np
import pytest

import assign_support as asg
import score_support as sc
import track_support as ts
from images_support import ptq      # noqa: F401 (fixture)


def same_as_statement(call, streams, steps, layout, gt_cap, out_cap, score_iou, state0, what, stats=None):
    want = sc.expected(call, streams, steps, layout, gt_cap, out_cap, score_iou, state0, stats)
    got = sc.host_run(call, streams, steps, layout, gt_cap, out_cap, score_iou, state0)
    assert got.rc == streams * steps and sc.same(got, want), what
    return got


def run_case(name, layout=ts.TIME):
    case = next(c for c in sc.designed() if c.name == name)
    call, streams, steps, state0 = sc.laid_out(case, layout)
    return same_as_statement(call, streams, steps, layout, case.gt_cap, case.out_cap, case.score_iou, state0, (name, layout)), streams, steps


def counters(state, s=0):
    return {name: int(state[name][s]) for name in sc.COUNTERS}


@pytest.mark.parametrize("name", [c.name for c in sc.designed()])
def test_host_build_equals_the_statement_on_the_designed_scenes(name):
    for layout in ts.LAYOUTS:
        run_case(name, layout)


def test_two_ids_exchanged_are_two_switches_on_that_frame_and_none_after():
    case = next(c for c in sc.designed() if c.name == "swap")
    call, streams, steps, state0 = sc.laid_out(case, ts.TIME)
    seen = []
    for t in range(1, 6):                                        # the first t frames: time-major, one stream
        r = sc.host_run(tuple(a[:t] for a in call), 1, t, ts.TIME, 2, 2, 0.5, state0)
        seen.append(int(r.state["switches"][0]))
    assert seen == [0, 0, 0, 2, 2]
    assert counters(r.state) == dict(frames=5, gt=10, hyp=10, matches=10, misses=0, false_positives=0, switches=2, overlap=10 * sc.TOP)
    assert r.match.tolist() == [[0, 1]] * 5 and r.status.tolist() == [0] * 5
    assert r.state["last"][0, :3].tolist() == [9, 7, 0] and r.state["present"][0, :3].tolist() == [5, 5, 0]
    assert r.state["tracked"][0, :3].tolist() == [5, 5, 0]
    assert sc.host_summary(r.state)["mota"] == 1.0 - 2.0 / 10.0 and sc.host_summary(r.state)["motp"] == (float(10 * sc.TOP) / 10.0) / 2.0 ** 30


def test_a_kept_pair_stays_where_exchanging_partners_would_weigh_more():
    kept, _, _ = run_case("continuity")
    alone, _, _ = run_case("optimum")
    w_kept, w_swap = 1 + int(67 / 133 * 2 ** 30), 1 + int(93 / 107 * 2 ** 30)
    assert 67 / 133 >= 0.5 and w_swap > w_kept
    assert kept.match.tolist() == [[0, 1], [0, 1]] and counters(kept.state)["switches"] == 0
    assert counters(kept.state)["overlap"] == 2 * sc.TOP + 2 * w_kept
    assert alone.match.tolist() == [[1, 0]] and counters(alone.state)["overlap"] == 2 * w_swap      # the optimum, where nothing is kept


def test_two_rows_with_the_same_last_hypothesis_an_object_that_returns_and_empty_rows():
    r, _, _ = run_case("same_last")
    assert r.match[0, :2].tolist() == [1, 0] and r.match[0, 2] == ts.SENTINEL32
    assert counters(r.state)["switches"] == 1 and r.state["last"][0, :2].tolist() == [5, 6]
    r, _, _ = run_case("returns")
    assert r.state["switches"].tolist() == [1, 0] and r.state["matches"].tolist() == [3, 3] and r.state["frames"].tolist() == [5, 5]
    assert r.state["last"][:, 0].tolist() == [4, 3] and r.state["present"][:, 0].tolist() == [3, 3]
    r, _, _ = run_case("empty")
    assert counters(r.state) == dict(frames=5, gt=3, hyp=3, matches=0, misses=3, false_positives=3, switches=0, overlap=0)
    assert r.match.tolist() == [[-1, -1]] + [[ts.SENTINEL32] * 2] * 3 + [[-1, ts.SENTINEL32]]


def test_void_rows_void_records_and_counts_above_the_caps_set_exactly_their_bits():
    r, _, _ = run_case("voids")
    assert r.status.tolist() == [sc.GT_VOID, sc.HYP_VOID, sc.GT_CLIPPED, sc.HYP_CLIPPED, 15, 0, 0]
    # of the six rows only (5, B) and (6, A) count: hypotheses 12 and 11
    assert r.match[0].tolist() == [-1, -1, -1, 1, -1, 0] and r.match[1].tolist()[:2] == [1, -1]
    assert r.match[4].tolist() == [-1, -1, -1, 2, -1, 1] and (r.match[5] == ts.SENTINEL32).all()
    c = counters(r.state)
    assert c["frames"] == 7 and c["gt"] == 2 + 2 + 6 + 2 + 2 + 0 + 2 and c["hyp"] == 2 + 1 + 2 + 3 + 2 + 0 + 2
    assert c["switches"] == 0 and c["misses"] == 1 + 4 and c["false_positives"] == 1
    for name, want in (("iou0", [0, -1]), ("iou1", [0, -1])):
        r, _, _ = run_case(name)
        assert r.match.tolist() == [want], name


def test_every_number_of_rows_against_every_number_of_columns():
    frames = sc.sweep_frames()
    stats = {}
    for score_iou in (0.05, 0.5):
        for layout in ts.LAYOUTS:
            call = sc.lay_out(frames, 64, 64, layout)
            r = same_as_statement(call, 15, 2, layout, 64, 64, score_iou, sc.empty_state(15), (score_iou, layout), stats)
    assert stats["kept"] > 0 and stats["new"] > 0 and stats["switches"] > 0
    assert (r.state["matches"] > 0).any() and (r.state["misses"] > 0).any() and (r.state["false_positives"] > 0).any()


def test_the_table_of_equal_weights_and_the_staircase(ptq):
    for layout in ts.LAYOUTS:
        stats = {}
        r = same_as_statement(sc.lay_out(sc.equal_frames(), 64, 64, layout), 1, 2, layout, 64, 64, 0.3, sc.empty_state(1), ("equal", layout), stats)
        first, second = ts.frame_of(0, 0, 1, 2, layout), ts.frame_of(0, 1, 1, 2, layout)
        assert r.match[first].tolist() == list(range(64)) and r.match[second].tolist() == list(range(63, -1, -1))
        assert stats == dict(kept=64, new=64, switches=0, void_rows=0, void_columns=0) and counters(r.state)["matches"] == 128
        r = same_as_statement(sc.lay_out(sc.staircase_frames(), 64, 64, layout), 1, 2, layout, 64, 64, asg.STAIR_IOU, sc.empty_state(1),
                              ("stair", layout))
        # row i (the strip over 64 - i tiles) ends on column 63 - i
        assert r.match[first].tolist() == list(range(63, -1, -1)) and counters(r.state)["matches"] > 64
    # the searches these tables force, by the statement: 2080 rounds, an augmenting path through all 64 columns
    truths, hyps = sc.staircase_frames()[0][0][:2]
    rec = lambda t: (0,) * 6 + tuple(t[1:])
    search = {}
    ptq.track_assign_solve(ptq.track_assign_weights({j: rec(t) for j, t in enumerate(hyps)}, [rec(t) for t in truths], asg.STAIR_IOU), search)
    assert search["rounds"] == 2080 and search["path"] == 64


@pytest.mark.parametrize("streams", [1, 3, 5])
def test_streams_by_steps_in_both_layouts_and_one_call_against_many(streams):
    for steps in (1, 7):
        frames = sc.drift_frames(streams, steps)
        results = {}
        for layout in ts.LAYOUTS:
            call = sc.lay_out(frames, sc.D_GT_CAP, sc.D_OUT_CAP, layout)
            results[layout] = same_as_statement(call, streams, steps, layout, sc.D_GT_CAP, sc.D_OUT_CAP, 0.5, sc.junk_state(streams), (streams, steps, layout))
        assert results[ts.TIME].state.tobytes() == results[ts.STREAM].state.tobytes()
        call = sc.lay_out(frames, sc.D_GT_CAP, sc.D_OUT_CAP, ts.TIME)
        split = sc.split_calls(sc.host_run, call, streams, steps, sc.D_GT_CAP, sc.D_OUT_CAP, 0.5, sc.junk_state(streams))
        assert sc.same(split, results[ts.TIME]), (streams, steps)


def test_one_streams_input_changes_no_other_streams_bytes():
    streams, steps = 5, 7
    frames = sc.drift_frames(streams, steps)
    other = [list(clip) for clip in frames]
    other[2] = [([(3, 7, 7, 30 + t, 30), (4, 200, 100, 240, 150 - t)], [(8, 9, 8, 33 + t, 31)], None, None) for t in range(steps)]
    for layout in ts.LAYOUTS:
        a = sc.host_run(sc.lay_out(frames, sc.D_GT_CAP, sc.D_OUT_CAP, layout), streams, steps, layout, sc.D_GT_CAP, sc.D_OUT_CAP, 0.5, sc.empty_state(streams))
        b = sc.host_run(sc.lay_out(other, sc.D_GT_CAP, sc.D_OUT_CAP, layout), streams, steps, layout, sc.D_GT_CAP, sc.D_OUT_CAP, 0.5, sc.empty_state(streams))
        for s in range(streams):
            rows = [ts.frame_of(s, t, streams, steps, layout) for t in range(steps)]
            equal = a.state[s].tobytes() == b.state[s].tobytes() and a.match[rows].tobytes() == b.match[rows].tobytes() and \
                a.status[rows].tobytes() == b.status[rows].tobytes()
            assert equal == (s != 2), (layout, s)


def test_random_states_wrap_and_saturate_as_the_statement_does_and_the_random_scenes_count_everything():
    streams, steps = 3, 40
    frames = sc.drift_frames(streams, steps)
    stats = {}
    for layout in ts.LAYOUTS:
        call = sc.lay_out(frames, sc.D_GT_CAP, sc.D_OUT_CAP, layout)
        state0 = sc.junk_state(streams)
        r = same_as_statement(call, streams, steps, layout, sc.D_GT_CAP, sc.D_OUT_CAP, 0.5, state0, layout, stats)
        assert int(r.state["frames"][0]) == steps - 1 and int(r.state["gt"][0]) < 8 * steps               # from UINT64_MAX: wrapped
        touched = r.state["present"][0] != state0["present"][0]
        assert (r.state["present"][0, ::2] == ts.I32MAX).all() and touched[1::2].any() and not touched[::2].any()
        without = sc.host_run(call, streams, steps, layout, sc.D_GT_CAP, sc.D_OUT_CAP, 0.5, state0, with_match=False, with_status=False)
        assert (without.match == ts.SENTINEL32).all() and (without.status == ts.SENTINEL32).all() and without.state.tobytes() == r.state.tobytes()
    for name in ("kept", "new", "switches", "void_rows"):
        assert stats.get(name, 0) >= 1, (name, stats)


def test_the_summary_equals_the_statements_bit_for_bit(ptq):
    frames = sc.drift_frames(3, 40)
    call = sc.lay_out(frames, sc.D_GT_CAP, sc.D_OUT_CAP, ts.TIME)
    scored = sc.host_run(call, 3, 40, ts.TIME, sc.D_GT_CAP, sc.D_OUT_CAP, 0.5, sc.empty_state(3)).state
    no_match = sc.crafted(present={1: 4, 2: 5, 3: 5, 4: 1, 5: 0, 6: -3}, tracked={1: 4, 2: 4, 3: 3, 4: 0, 5: 9, 6: -3}, frames=5, gt=7, hyp=2, misses=7,
                          false_positives=2)
    wrapped = sc.crafted(gt=3, misses=sc.U64MAX, false_positives=5, switches=9, matches=sc.U64MAX, overlap=sc.U64MAX - 7)
    for states in (scored, scored[:1], sc.empty_state(1), sc.empty_state(2)[:0], no_match, wrapped, sc.junk_state(4), sc.junk_state(2, 8400, False),
                   np.concatenate([scored, no_match, wrapped])):
        want = sc.py_summary(states)
        assert sc.same_summary(sc.host_summary(states), want), want
    s = sc.host_summary(no_match)
    assert (s["objects"], s["mostly_tracked"], s["mostly_lost"]) == (4, 2, 1) and s["motp"] == 0.0 and s["mota"] == 1.0 - 9.0 / 7.0
    empty = sc.host_summary(sc.empty_state(1))
    assert empty["mota"] == 0.0 and empty["motp"] == 0.0 and empty["objects"] == 0
    total = sc.host_summary(scored)
    assert total["gt"] > 0 and total["matches"] > 0 and 0.0 < total["motp"] <= 1.0 + 2.0 ** -30
    assert total["frames"] == 120 and total["matches"] + total["misses"] == total["gt"] and total["matches"] + total["false_positives"] == total["hyp"]
    assert sc.score_host().yf_images_score_summary_host(None, 1, np.zeros(1, sc.SUMMARY).ctypes.data) == -1
    assert sc.score_host().yf_images_score_summary_host(scored.ctypes.data, -1, np.zeros(1, sc.SUMMARY).ctypes.data) == -1
    assert sc.score_host().yf_images_score_summary_host(scored.ctypes.data, 1, None) == -1


def test_every_argument_check_with_its_text():
    assert sc.host_check() == "" and sc.host_check(match=0, status=0) == "" and sc.host_check(streams=0, steps=0) == ""
    assert sc.host_check(gt_cap=64, out_cap=2 ** 31 - 1, score_iou=float("inf")) == ""
    for kw, text in sc.FAULTS:
        assert text in sc.host_check(**kw), kw
    assert sc.score_host().yf_images_score_state_bytes_host(3) == 3 * 3136 and sc.score_host().yf_images_score_state_bytes_host(0) == 0
    assert sc.score_host().yf_images_score_state_bytes_host(-2) == 0
    # a refused call writes nothing; neither does an empty batch, which is taken after the checks
    case = next(c for c in sc.designed() if c.name == "swap")
    call, streams, steps, _ = sc.laid_out(case, ts.TIME)
    state0 = sc.junk_state(1)
    def refused(**kw):
        def fn(*p):
            a = dict(zip(sc.NAMES, p), **kw)
            return sc.score_host().yf_images_score_tracks_host(*(a[k] for k in sc.NAMES), None)
        return sc.run_with(fn, call, 1, steps, ts.TIME, 2, 2, 0.5, state0)
    for kw in (dict(gt_cap=65), dict(out_cap=0), dict(score_iou=float("nan")), dict(layout=2), dict(steps=-1), dict(gt=None), dict(match=2)):
        r = refused(**kw)
        assert r.rc == -1 and r.state.tobytes() == state0.tobytes() and (r.match == ts.SENTINEL32).all() and (r.status == ts.SENTINEL32).all(), kw
    for streams0, steps0 in ((0, 5), (1, 0), (0, 0)):
        r = sc.host_run(call, streams0, steps0, ts.TIME, 2, 2, 0.5, state0)
        assert r.rc == 0 and r.state.tobytes() == state0.tobytes() and (r.match == ts.SENTINEL32).all() and (r.status == ts.SENTINEL32).all()


def scored_tracker(gains, assign, stream, layout=ts.TIME):
    """the tracker's host build on one stream of `asg.crossing_frames`, then the score's on what it reported -> (Result, tracker Result)"""
    frames, truth = [asg.crossing_frames()[stream]], [sc.clip_truth()[stream]]
    tracked = sc.tracked_on_host(frames, asg.C_CAP, gains, assign)
    gt, gt_counts = sc.truth_arrays(truth, 2, ts.TIME)
    call = (tracked.out, tracked.info, tracked.out_counts, gt, gt_counts)
    return same_as_statement(call, 1, asg.C_STEPS, ts.TIME, 2, 8, sc.SCORE_IOU, sc.empty_state(1), (gains, assign, stream)), tracked


def test_on_the_pan_the_greedy_match_switches_identities_and_the_optimal_assignment_does_not():
    greedy, _ = scored_tracker(asg.BASE_GAINS, asg.GREEDY, 1)
    optimal, _ = scored_tracker(asg.BASE_GAINS, asg.OPTIMAL, 1)
    g, o = sc.host_summary(greedy.state), sc.host_summary(optimal.state)
    assert g["switches"] > 0 and g["false_positives"] > 0 and g["mota"] < 1.0
    assert o["switches"] == 0 and o["false_positives"] == 0 and o["misses"] == 0 and o["mota"] == 1.0
    assert o["gt"] == g["gt"] == 2 * asg.C_STEPS and o["matches"] == 2 * asg.C_STEPS and o["mostly_tracked"] == 2
    assert sc.same_summary(g, sc.py_summary(greedy.state)) and sc.same_summary(o, sc.py_summary(optimal.state))
    # the motion model at the suggested gains: the optimal assignment still keeps both identities
    assert sc.host_summary(scored_tracker(asg.SUGGESTED, asg.OPTIMAL, 1)[0].state)["mota"] == 1.0
