"""The optimal assignment on the CPU: the host build of csrc/yf_images_assign.h (yf_images_track_motion_assign_host, libyf_images_host.so)
against the plain-Python statement `ptq.track_assign_match` / `ptq.track_motion_step(assign="optimal")`, exactly -- the minimal scene on
which the greedy match strands a detection and the optimal one keeps both identities; optimality itself, independently of the procedure,
against a brute force over all injections and against scipy.optimize.linear_sum_assignment; the tie rules, pinned by recorded
assignments; sequences of two faces passing each other, random sequences, a state of random bytes and a full table in both layouts,
every byte of records, infos, counts, status and state; assign = greedy is the motion entry's host function, and optimal equals greedy
where no detection and no slot has two eligible partners; the argument checks.  No GPU."""
import itertools

import numpy as np
import pytest

import assign_support as asg
import motion_support as ms
import track_support as ts
from images_support import ptq          # noqa: F401 (fixture)


def both(dets, counts, streams, steps, layout, cap, params, assign, state0, out_cap, what):
    """the host build equals the statement -> the result"""
    want = asg.expected(dets, counts, streams, steps, layout, cap, params, assign, state0, out_cap)
    got = asg.host_run(dets, counts, streams, steps, layout, cap, params, assign, state0, out_cap)
    assert got.rc == streams * steps and ts.same(got, want), what
    return got


def test_the_minimal_scene_greedy_strands_a_detection_and_optimal_keeps_both_ids(ptq):
    a, b, d0, d1 = (asg.rec(box) for box in (asg.A, asg.B, asg.D0, asg.D1))
    iou = {name: ptq.track_iou(x, y)[1] for name, x, y in (("A0", a, d0), ("B0", b, d0), ("A1", a, d1), ("B1", b, d1))}
    assert iou["A0"] == 0.6 and iou["B0"] == iou["A1"] == 6700.0 / 13300.0 and iou["B1"] == 900.0 / 19100.0
    assert [v >= 0.3 for v in iou.values()] == [True, True, True, False]
    assert ptq._track_match({0: a, 1: b}, [d0, d1], 0.3)[:2] == ({0: 0}, {0: 0})
    slot_det, det_slot, total = ptq.track_assign_match({0: a, 1: b}, [d0, d1], 0.3)
    assert (slot_det, det_slot) == ({0: 1, 1: 0}, {0: 1, 1: 0}) and total == 2 * (1 + int(6700.0 / 13300.0 * 2 ** 30)) > 1 + int(0.6 * 2 ** 30)
    assert asg.host_match({0: asg.A, 1: asg.B}, [asg.D0, asg.D1], 0.3)[:3] == (slot_det, det_slot, total)
    # ... and as two steps of the tracker: greedy gives d0 to track 1 (A), bears d1 as track 3 and holds track 2 (B) over; optimal
    # gives d0 to track 2 and d1 to track 1, and no id is issued
    for gains in (asg.BASE_GAINS, asg.SUGGESTED):
        for layout in ts.LAYOUTS:
            dets, counts = ts.lay_out(asg.minimal_frames(), 2, layout)
            params = asg.M_PARAMS + gains
            g = both(dets, counts, 1, 2, layout, 2, params, asg.GREEDY, ms.empty_state(1), 4, ("greedy", gains, layout))
            o = both(dets, counts, 1, 2, layout, 2, params, asg.OPTIMAL, ms.empty_state(1), 4, ("optimal", gains, layout))
        assert ms.boxes_of(g, 1) == [(1, *asg.D0, 0), (2, *asg.B, 1), (3, *asg.D1, 0)] and int(g.state["issued"][0]) == 3
        assert ms.boxes_of(o, 1) == [(1, *asg.D1, 0), (2, *asg.D0, 0)] and int(o.state["issued"][0]) == 2


def random_scene(rng, m, occupied):
    """m detections and `occupied` tracks in random slots, boxes of side 20 .. 80 thrown into a square of 150: most pairs overlap"""
    def box():
        x, y, w, h = (int(v) for v in (rng.integers(0, 150), rng.integers(0, 150), rng.integers(20, 81), rng.integers(20, 81)))
        return (x, y, x + w - 1, y + h - 1)
    slots = sorted(int(k) for k in rng.choice(64, occupied, replace=False))
    return {k: box() for k in slots}, [box() for _ in range(m)]


def brute_force(w, slots):
    """the largest total weight over all injections of a subset of the rows into the given columns"""
    best = 0
    rows = range(len(w))
    for k in range(min(len(w), len(slots)) + 1):
        for chosen in itertools.combinations(rows, k):
            for cols in itertools.permutations(slots, k):
                if all(w[i][j] > 0 for i, j in zip(chosen, cols)):
                    best = max(best, sum(w[i][j] for i, j in zip(chosen, cols)))
    return best


@pytest.mark.parametrize("occupied", [0, 1, 5, 64])
@pytest.mark.parametrize("m", [0, 1, 2, 3, 7, 8, 63, 64])
def test_the_match_is_optimal_whatever_the_procedure(ptq, m, occupied):
    rng = np.random.default_rng(7000 + 100 * m + occupied)
    beat = 0
    for trial in range(3):
        match_iou = (0.05, 0.2, 0.4)[trial]
        boxes, dets = random_scene(rng, m, occupied)
        records = {k: asg.rec(b) for k, b in boxes.items()}
        w = ptq.track_assign_weights(records, [asg.rec(d) for d in dets], match_iou)
        slot_det, det_slot, total = ptq.track_assign_match(records, [asg.rec(d) for d in dets], match_iou)
        assert asg.host_match(boxes, dets, match_iou) == (slot_det, det_slot, total, w), (m, occupied, trial)
        assert asg.host_solve(w) == (slot_det, det_slot, total)
        # a matching: injective both ways, of eligible pairs of occupied slots only
        assert {j: i for i, j in det_slot.items()} == slot_det and len(set(det_slot.values())) == len(det_slot)
        assert all(w[i][j] > 0 and j in boxes and 0 <= i < m for i, j in det_slot.items())
        assert all(w[i][j] == 0 for i in range(m) for j in range(64) if j not in boxes)
        for i, j in det_slot.items():
            iou = ptq.track_iou(records[j], asg.rec(dets[i]))[1]
            assert iou is not None and iou >= match_iou and w[i][j] == 1 + int(iou * 2 ** 30) and 1 <= w[i][j] <= asg.TOP
        assert total == sum(w[i][j] for i, j in det_slot.items())
        greedy = asg.greedy_total(w)
        g_slot_det = ptq._track_match(records, [asg.rec(d) for d in dets], match_iou)[0]
        assert greedy == sum(w[i][j] for j, i in g_slot_det.items())                    # the helper is the tracker's greedy match
        assert total >= greedy
        beat += total > greedy
        if m <= 6 and occupied <= 6:
            assert total == brute_force(w, sorted(boxes)), (m, occupied, trial)
    if m >= 63 and occupied == 64:
        assert beat >= 1                                                                # the scenes are ones on which greedy loses


@pytest.mark.parametrize("occupied", [0, 1, 5, 64])
@pytest.mark.parametrize("m", [1, 2, 3, 7, 8, 63, 64])
def test_the_larger_scenes_total_is_scipys(ptq, m, occupied):
    """the same scenes (the same seeds) against scipy.optimize.linear_sum_assignment on the table of weights"""
    optimize = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(7000 + 100 * m + occupied)
    for trial in range(3):
        match_iou = (0.05, 0.2, 0.4)[trial]
        boxes, dets = random_scene(rng, m, occupied)
        w = ptq.track_assign_weights({k: asg.rec(b) for k, b in boxes.items()}, [asg.rec(d) for d in dets], match_iou)
        a = np.array(w, np.int64).reshape(m, 64)
        r, c = optimize.linear_sum_assignment(a, maximize=True)
        assert ptq.track_assign_solve(w)[2] == asg.host_solve(w)[2] == int(a[r, c].sum()), (m, occupied, trial)


def test_the_procedure_on_tables_of_weights_against_brute_force_and_its_bound(ptq):
    """small tables with few levels of weight (many ties), at the extremes of the range: the total is the brute-force optimum, the host
    build gives the same pairs, and no potential leaves [0, 2^30 + 1]"""
    rng = np.random.default_rng(7050)
    stats = {}
    for trial in range(60):
        m, cols = int(rng.integers(0, 6)), sorted(int(k) for k in rng.choice(64, int(rng.integers(1, 6)), replace=False))
        levels = [(0, 1), (0, 1, 2, 3), (0, asg.TOP), (0, 1, asg.TOP - 1, asg.TOP)][trial % 4]
        w = [[0] * 64 for _ in range(m)]
        for i in range(m):
            for j in cols:
                w[i][j] = int(rng.choice(levels))
        got = ptq.track_assign_solve(w, stats)
        assert got[2] == brute_force(w, cols) and asg.host_solve(w) == got, (trial, w)
    assert 0 < stats["potential"] <= asg.TOP and stats["path"] >= 2


def test_the_tie_rules_are_pinned(ptq):
    # all weights equal at 64 x 64: every permutation is optimal; the procedure gives detection i slot i, in 2080 rounds
    boxes, dets = asg.all_equal_scene()
    records, recs = {k: asg.rec(b) for k, b in boxes.items()}, [asg.rec(d) for d in dets]
    w = ptq.track_assign_weights(records, recs, 0.3)
    assert len({x for row in w for x in row}) == 1 and w[0][0] > 1
    stats = {}
    slot_det, det_slot, total = ptq.track_assign_solve(w, stats)
    assert det_slot == {i: i for i in range(64)} and total == 64 * w[0][0] and stats["rounds"] == 2080 and stats["potential"] <= asg.TOP
    assert asg.host_match(boxes, dets, 0.3) == (slot_det, det_slot, total, w)
    # the staircase: 2080 rounds too, the last row's augmenting path runs through all 64 columns; detection i (the strip over 64 - i
    # tiles) ends on slot 63 - i
    boxes, dets = asg.staircase_scene()
    records, recs = {k: asg.rec(b) for k, b in boxes.items()}, [asg.rec(d) for d in dets]
    w = ptq.track_assign_weights(records, recs, asg.STAIR_IOU)
    assert all(w[i][j] == (1 + 2 ** 30 // (64 - i) if j < 64 - i else 0) for i in range(64) for j in range(64))
    stats = {}
    slot_det, det_slot, total = ptq.track_assign_solve(w, stats)
    assert det_slot == {i: 63 - i for i in range(64)} and stats["rounds"] == 2080 and stats["path"] == 64 and stats["potential"] <= asg.TOP
    assert asg.host_match(boxes, dets, asg.STAIR_IOU) == (slot_det, det_slot, total, w)
    # two identical detections and one track (slot 9): the lower detection gets it; with two tracks at the same box (slots 9 and 30)
    # detection 0 gets the lower slot; two identical tracks and one detection: the lower slot
    t, d = (0, 0, 19, 19), (2, 0, 21, 19)
    cases = [({9: t}, [d, d], {0: 9}), ({9: t, 30: t}, [d, d], {0: 9, 1: 30}), ({30: t, 9: t}, [d], {0: 9}),
             ({9: t, 30: t, 31: (100, 100, 119, 119)}, [d, (101, 100, 120, 119), d], {0: 9, 1: 31, 2: 30})]
    for boxes, dets, want in cases:
        got = ptq.track_assign_match({k: asg.rec(b) for k, b in boxes.items()}, [asg.rec(x) for x in dets], 0.3)
        assert got[1] == want and asg.host_match(boxes, dets, 0.3)[:3] == got, (boxes, dets, got)


def test_the_crossing_sequences_differ_between_the_matches_and_the_host_build_equals_the_statement():
    frames = asg.crossing_frames()
    for gains in (asg.BASE_GAINS, asg.SUGGESTED):
        params = asg.M_PARAMS + gains
        for layout in ts.LAYOUTS:
            dets, counts = ts.lay_out(frames, asg.C_CAP, layout)
            o = both(dets, counts, 2, asg.C_STEPS, layout, asg.C_CAP, params, asg.OPTIMAL, ms.empty_state(2), 8, ("optimal", gains, layout))
            g = both(dets, counts, 2, asg.C_STEPS, layout, asg.C_CAP, params, asg.GREEDY, ms.empty_state(2), 8, ("greedy", gains, layout))
        if gains == asg.BASE_GAINS:
            # without a motion model the two matches part on both streams; on the pan greedy strands a detection step after step
            assert ts.by_frame(o, 2, asg.C_STEPS, layout)[0] != ts.by_frame(g, 2, asg.C_STEPS, layout)[0]
            assert o.state[0].tobytes() != g.state[0].tobytes()
            assert int(o.state["issued"][1]) == 2 and int(g.state["issued"][1]) > 2
        assert int(o.state["issued"][0]) == 2


@pytest.mark.parametrize("gains", [asg.SUGGESTED, ms.SUGGESTED + (1,), asg.BASE_GAINS, (128, 64, 200, 1)], ids=str)
def test_host_build_equals_the_statement_on_the_random_sequences(gains):
    results = {}
    for layout in ts.LAYOUTS:
        dets, counts = ts.lay_out(ms.random_frames(), ms.R_CAP, layout)
        results[layout] = both(dets, counts, ms.R_STREAMS, ms.R_STEPS, layout, ms.R_CAP, ms.R_BASE + gains, asg.OPTIMAL, ms.empty_state(ms.R_STREAMS),
                               ms.R_OUT_CAP, (gains, layout))
    assert ts.by_frame(results[ts.TIME], ms.R_STREAMS, ms.R_STEPS, ts.TIME) == ts.by_frame(results[ts.STREAM], ms.R_STREAMS, ms.R_STEPS, ts.STREAM)
    assert (results[ts.TIME].status & 1).any() and (results[ts.TIME].out_counts > 0).any()


def test_host_build_equals_the_statement_on_the_crowded_random_sequences_of_the_base_tracker():
    """tests/track_support.py's sequences: up to 70 records a frame, a table that fills up, ties, drops"""
    for layout in ts.LAYOUTS:
        dets, counts = ts.lay_out(ts.random_frames(), ts.R_CAP, layout)
        r = both(dets[:], counts, ts.R_STREAMS, ts.R_STEPS, layout, ts.R_CAP, ts.R_PARAMS + asg.SUGGESTED, asg.OPTIMAL, ms.empty_state(ts.R_STREAMS),
                 ts.R_OUT_CAP, layout)
    assert (r.status == 3).any() and (r.out_counts > ts.R_OUT_CAP).any()


def test_a_state_of_random_bytes_a_full_table_and_the_dense_scenes():
    for layout in ts.LAYOUTS:
        dets, counts, junk = asg.junk_call(layout)
        for gains in (ms.SUGGESTED + (1,), ms.DIFFERENCE + (0,)):
            both(dets, counts, 2, 3, layout, 6, (0.3, 2, 1) + gains, asg.OPTIMAL, junk, 64, ("junk", gains, layout))
        near = [(10, 10, 40, 40), (100, 100, 140, 140), (12, 9, 41, 42)]
        d2, c2 = ts.lay_out([[(near, None), (near[::-1], None), ([], None), (near, None)]], 3, layout)
        both(d2, c2, 1, 4, layout, 3, (0.1, 1, 3) + ms.DIFFERENCE + (1,), asg.OPTIMAL, ms.extreme_state(), 64, ("extreme", layout))
        # the full tables: 64 tracks and 64 detections all mutually eligible; then the staircase; every lane matches
        state0, frames = asg.all_equal_state()
        d3, c3 = ts.lay_out(frames, 64, layout)
        r = both(d3, c3, 1, 2, layout, 64, (0.3, 1, 2) + asg.SUGGESTED, asg.OPTIMAL, state0, 64, ("equal", layout))
        assert (r.out_counts == 64).all() and not r.status.any() and (r.info["misses"] == 0).all() and int(r.state["issued"][0]) == 64
        boxes, stair = asg.staircase_scene()
        d4, c4 = ts.lay_out([[(stair, None), (stair[:40] + [(900, 900, 950, 950)] * 3, None)]], 64, layout)
        r = both(d4, c4, 1, 2, layout, 64, (asg.STAIR_IOU, 1, 2) + asg.BASE_GAINS, asg.OPTIMAL, asg.scene_state(boxes), 64, ("stair", layout))
        first = ts.frame_of(0, 0, 1, 2, layout)
        assert (r.info["misses"][first] == 0).all() and r.status.tolist() == [0, 2]       # all 64 matched; then a full table drops births


def test_assign_greedy_is_the_motion_entrys_host_function():
    calls = []
    for layout in ts.LAYOUTS:
        calls.append((*ts.lay_out(ms.random_frames(), ms.R_CAP, layout), ms.R_STREAMS, ms.R_STEPS, layout, ms.R_CAP, ms.R_BASE + asg.SUGGESTED,
                      ms.empty_state(ms.R_STREAMS), ms.R_OUT_CAP))
        calls.append((*ts.lay_out(asg.crossing_frames(), asg.C_CAP, layout), 2, asg.C_STEPS, layout, asg.C_CAP, asg.M_PARAMS + asg.BASE_GAINS,
                      ms.empty_state(2), 8))
        dets, counts, junk = asg.junk_call(layout)
        calls.append((dets, counts, 2, 3, layout, 6, (0.3, 2, 1) + ms.SUGGESTED + (1,), junk, 64))
        state0, frames = asg.all_equal_state()
        calls.append((*ts.lay_out(frames, 64, layout), 1, 2, layout, 64, (0.3, 1, 2) + asg.SUGGESTED, state0, 64))
    for dets, counts, streams, steps, layout, cap, params, state0, out_cap in calls:
        want = ms.host_run(dets, counts, streams, steps, layout, cap, params, state0, out_cap)
        got = asg.host_run(dets, counts, streams, steps, layout, cap, params, asg.GREEDY, state0, out_cap)
        assert want.rc == streams * steps and ts.same(got, want), (layout, cap)
        assert ts.same(got, asg.expected(dets, counts, streams, steps, layout, cap, params, asg.GREEDY, state0, out_cap))


def test_optimal_equals_greedy_where_no_detection_and_no_slot_has_two_eligible_partners():
    frames = asg.sparse_frames()
    streams, steps, cap = len(frames), len(frames[0]), 8
    for gains in (asg.SUGGESTED, asg.BASE_GAINS):
        params = (0.3, 1, 2) + gains
        for layout in ts.LAYOUTS:
            dets, counts = ts.lay_out(frames, cap, layout)
            assert asg.max_degree(dets, counts, streams, steps, layout, cap, params, ms.empty_state(streams)) == 1      # the precondition
            g = asg.host_run(dets, counts, streams, steps, layout, cap, params, asg.GREEDY, ms.empty_state(streams), 8)
            o = asg.host_run(dets, counts, streams, steps, layout, cap, params, asg.OPTIMAL, ms.empty_state(streams), 8)
            assert g.rc == streams * steps and ts.same(g, o), (gains, layout)
            assert (g.info["misses"][g.info["id"] != 0xA5A5A5A5] > 0).any() and (g.out_counts > 1).any()    # tracks held over, several at once
    # ... and the scenario of a moving box with a gap, and the lifecycle of the designed sequences
    dets, counts = ts.lay_out(ms.scenario(), ms.S_CAP, ts.TIME)
    params = ms.S_BASE + asg.SUGGESTED
    assert asg.max_degree(dets, counts, 1, ms.S_STEPS, ts.TIME, ms.S_CAP, params, ms.empty_state(1)) == 1
    assert ts.same(asg.host_run(dets, counts, 1, ms.S_STEPS, ts.TIME, ms.S_CAP, params, asg.GREEDY, ms.empty_state(1), 4),
                   asg.host_run(dets, counts, 1, ms.S_STEPS, ts.TIME, ms.S_CAP, params, asg.OPTIMAL, ms.empty_state(1), 4))


def test_one_call_of_many_steps_equals_many_calls_of_one():
    params = ms.R_BASE + asg.SUGGESTED
    dets, counts = ts.lay_out(ms.random_frames(), ms.R_CAP, ts.TIME)
    want = asg.expected(dets, counts, ms.R_STREAMS, ms.R_STEPS, ts.TIME, ms.R_CAP, params, asg.OPTIMAL, ms.empty_state(ms.R_STREAMS), ms.R_OUT_CAP)
    run = lambda d, c, streams, steps, layout, cap, p, state0, out_cap: asg.host_run(d, c, streams, steps, layout, cap, p, asg.OPTIMAL, state0, out_cap)
    got = ts.split_calls(run, dets, counts, ms.R_STREAMS, ms.R_STEPS, ms.R_CAP, params, ms.empty_state(ms.R_STREAMS), ms.R_OUT_CAP)
    assert ts.same(got, want)


def test_the_argument_check_rejects_every_fault_in_the_motion_entrys_order_then_assign(ptq):
    assert asg.host_check() == "" and asg.host_check(asg.GREEDY) == "" and asg.host_check(streams=0) == ""
    for bad in asg.BAD_ASSIGNS:
        assert "assign must be" in asg.host_check(bad)
    for kw, text in ms.FAULTS:
        for assign in (asg.OPTIMAL, 7):                                               # every other fault comes before a bad assign
            assert text in asg.host_check(assign, **kw) and asg.host_check(assign, **kw) == ms.host_check(**kw), (kw, assign)
    # the entry refuses what the check refuses and writes nothing; an empty batch is taken after the checks and writes nothing either
    dets, counts = ts.lay_out(ms.scenario(), ms.S_CAP, ts.TIME)
    state0 = ms.junk_state(1)
    good = ms.S_BASE + asg.SUGGESTED
    for params, assign, cap in ((good, 2, ms.S_CAP), (good, -1, ms.S_CAP), (ms.S_BASE + (257, 0, 0, 0), asg.OPTIMAL, ms.S_CAP), (good, asg.OPTIMAL, 0),
                                (ms.S_BASE + ms.SUGGESTED + (2,), asg.GREEDY, ms.S_CAP)):
        r = asg.host_run(dets, counts, 1, ms.S_STEPS, ts.TIME, cap, params, assign, state0, 4)
        assert r.rc == -1 and r.state.tobytes() == state0.tobytes() and (r.out_counts == ts.SENTINEL32).all(), (params, assign, cap)
        assert (r.out.view(np.uint8) == 0xA5).all() and (r.status == ts.SENTINEL32).all()
    for streams0, steps0 in ((0, 5), (1, 0), (0, 0)):
        r = asg.host_run(dets, counts, streams0, steps0, ts.TIME, ms.S_CAP, good, asg.OPTIMAL, state0, 4)
        assert r.rc == 0 and r.state.tobytes() == state0.tobytes() and (r.out_counts == ts.SENTINEL32).all()
    assert asg.host_run(dets, counts, 0, 0, ts.TIME, ms.S_CAP, good, 5, state0, 4).rc == -1       # ... after the checks
    with pytest.raises(ValueError, match="assign"):
        ptq.track_motion_step(ptq.track_motion_empty_state(), [], good, assign="hungarian")
