"""The tracker with a motion model on the CPU: the host build of csrc/yf_images_motion.h (yf_images_track_motion_host,
libyf_images_host.so) against the plain-Python statement `ptq.track_motion_step`, exactly -- records, infos, counts, status and the whole
state buffer, every array between guard bytes and every place that must not be written a sentinel -- on the scenario of a moving box whose
detections have a gap (with its expected ids and held-over boxes, literally), the designed sequences of tests/track_support.py and seeded
random ones; both layouts; the equivalence with the base tracker at (alpha, beta) = (256, 0); the rounding of the two helpers; states of
random bytes and at the int64 extremes, records at the int32 extremes; one call of F steps against F calls of one; the argument checks.
No GPU."""
import numpy as np
import pytest

import motion_support as ms
import track_support as ts
from images_support import ptq          # noqa: F401 (fixture)


def both(dets, counts, streams, steps, layout, cap, params, state0, out_cap, what):
    """the host build equals the statement -> the result"""
    want = ms.expected(dets, counts, streams, steps, layout, cap, params, state0, out_cap)
    got = ms.host_run(dets, counts, streams, steps, layout, cap, params, state0, out_cap)
    assert got.rc == streams * steps and ts.same(got, want), what
    return got


@pytest.mark.parametrize("gains", ms.GAIN_SETS, ids=str)
@pytest.mark.parametrize("smooth", [0, 1])
def test_the_scenario_of_a_moving_box_with_a_gap(gains, smooth):
    """the ids and the held-over boxes the definition gives: without a velocity the box stays behind and the face comes back as track 2;
    with one the box follows and the id stays"""
    for layout in ts.LAYOUTS:
        dets, counts = ts.lay_out(ms.scenario(), ms.S_CAP, layout)
        r = both(dets, counts, 1, ms.S_STEPS, layout, ms.S_CAP, ms.S_BASE + gains + (smooth,), ms.empty_state(1), 4, (gains, smooth, layout))
    ids, held = ms.S_EXPECTED[gains]
    for t in range(ms.S_STEPS):
        rows = ms.boxes_of(r, t)
        if t in ms.S_GAP:
            assert rows == [(1, *held[t - 6], t - 5)], (t, rows)                       # one track, held over, where the table says
        else:
            carrier = [row for row in rows if row[5] == 0]
            assert len(carrier) == 1 and carrier[0][0] == ids[t], (t, rows)
            if not smooth:
                assert carrier[0][1:5] == ms.s_box(t), (t, rows)                         # the detection verbatim
    if gains == ms.BASE_LIKE:
        # the face came back as track 2 while track 1 is still held where it was last seen: misses 4 and 5 at steps 9 and 10; at step 11 its
        # misses would be 6 > max_misses 5 and it is removed
        assert [ms.boxes_of(r, t)[0] for t in (9, 10)] == [(1, 70, 40, 109, 89, 4), (1, 70, 40, 109, 89, 5)]
        assert [len(ms.boxes_of(r, t)) for t in (9, 10, 11)] == [2, 2, 1] and int(r.state["issued"][0]) == 2
    else:
        assert all(len(ms.boxes_of(r, t)) == 1 for t in range(ms.S_STEPS)) and int(r.state["issued"][0]) == 1
    if gains == ms.DIFFERENCE:
        assert held == [ms.s_box(t) for t in ms.S_GAP]                                  # the true boxes
        assert r.state["slot"]["vel"][0, 0].tolist() == [256 * 12, 256 * 4, 256 * 12, 256 * 4]


def test_the_statement_reproduces_the_scenarios_table_at_the_base_trackers_own_call(ptq):
    """the left column of the table: `ptq.track_step`, the tracker without the model, on the scenario"""
    st, ids = ptq.track_empty_state(), []
    for t, (boxes, _) in enumerate(ms.scenario()[0]):
        st, emitted, _ = ptq.track_step(st, [(0, 0, 0, 0, 0, 0, *b) for b in boxes], ms.S_BASE, frame=t)
        ids.append([(i[0], rec[6:10]) for rec, i in emitted])
    assert [ids[t] for t in ms.S_GAP] == [[(1, (70, 40, 109, 89))]] * 3 and ids[9][1] == (2, ms.s_box(9))


@pytest.mark.parametrize("case", ts.designed(), ids=lambda c: c.name)
def test_host_build_equals_the_statement_on_the_designed_sequences(case):
    for layout in ts.LAYOUTS:
        dets, counts, streams, steps, base0 = ts.laid_out(case, layout)
        state0 = ms.lift(base0)
        for gains in (ms.SUGGESTED + (0,), (200, 100, 128, 1)):
            params = tuple(case.params) + gains
            want = both(dets, counts, streams, steps, layout, case.cap, params, state0, case.out_cap, (case.name, layout, gains))
        bare = ms.host_run(dets, counts, streams, steps, layout, case.cap, params, state0, case.out_cap, with_status=False)
        assert (bare.status == ts.SENTINEL32).all() and ts.same(bare._replace(status=want.status), want), (case.name, layout)


@pytest.mark.parametrize("gains", ms.R_GAINS, ids=str)
def test_host_build_equals_the_statement_on_the_random_sequences(gains):
    results = {}
    for layout in ts.LAYOUTS:
        dets, counts, want = ms.random_call(layout, gains)
        got = ms.host_run(dets, counts, ms.R_STREAMS, ms.R_STEPS, layout, ms.R_CAP, ms.R_BASE + gains, ms.empty_state(ms.R_STREAMS), ms.R_OUT_CAP)
        assert got.rc == ms.R_STREAMS * ms.R_STEPS and ts.same(got, want), layout
        results[layout] = got
    assert ts.by_frame(results[ts.TIME], ms.R_STREAMS, ms.R_STEPS, ts.TIME) == ts.by_frame(results[ts.STREAM], ms.R_STREAMS, ms.R_STEPS, ts.STREAM)
    assert results[ts.TIME].out.tobytes() != results[ts.STREAM].out.tobytes()


def test_the_random_sequences_exercise_the_filter():
    """matches, births, removals, held-over tracks and a clipped count all occur; with a velocity the held-over boxes move"""
    stats = {}
    dets, counts = ts.lay_out(ms.random_frames(), ms.R_CAP, ts.TIME)
    r = ms.expected(dets, counts, ms.R_STREAMS, ms.R_STEPS, ts.TIME, ms.R_CAP, ms.R_BASE + ms.SUGGESTED + (0,), ms.empty_state(ms.R_STREAMS),
                    ms.R_OUT_CAP, stats)
    assert all(stats.get(name, 0) >= 1 for name in ("matches", "births", "removals", "held")), stats
    assert (r.status & 1).any() and (r.state["slot"]["vel"] != 0).any() and (r.out_counts > ms.R_OUT_CAP).any()
    base = ms.expected(dets, counts, ms.R_STREAMS, ms.R_STEPS, ts.TIME, ms.R_CAP, ms.R_BASE + ms.BASE_LIKE + (0,), ms.empty_state(ms.R_STREAMS),
                       ms.R_OUT_CAP)
    assert r.out.tobytes() != base.out.tobytes()


def _base_part(state):
    out = ts.empty_state(len(state))
    out["issued"], out["reserved"], out["slot"] = state["issued"], state["reserved"], state["slot"]["base"]
    return out


@pytest.mark.parametrize("damp", [0, 200, 256])
@pytest.mark.parametrize("smooth", [0, 1])
def test_alpha_256_beta_0_is_the_base_tracker(damp, smooth):
    """from the empty state: the records, infos, counts and status of `ptq.track_step` and of yf_images_track_host, and the base tracker's
    slot in every slot's `base`"""
    gains = (256, 0, damp, smooth)
    calls = [(*ts.laid_out(c, layout)[:4], layout, c.cap, tuple(c.params), c.out_cap) for c in ts.designed() if c.state0 is None
             for layout in ts.LAYOUTS]
    for layout in ts.LAYOUTS:
        calls.append((*ts.lay_out(ms.random_frames(), ms.R_CAP, layout), ms.R_STREAMS, ms.R_STEPS, layout, ms.R_CAP, ms.R_BASE, ms.R_OUT_CAP))
    for dets, counts, streams, steps, layout, cap, base_params, out_cap in calls:
        want = ts.expected(dets, counts, streams, steps, layout, cap, base_params, ts.empty_state(streams), out_cap)
        assert ts.same(want, ts.host_run(dets, counts, streams, steps, layout, cap, base_params, ts.empty_state(streams), out_cap))
        for run in (ms.expected, ms.host_run):
            got = run(dets, counts, streams, steps, layout, cap, base_params + gains, ms.empty_state(streams), out_cap)
            assert got.rc == want.rc and all(getattr(got, name).tobytes() == getattr(want, name).tobytes()
                                             for name in ("out", "info", "out_counts", "status")), (layout, cap, run.__name__)
            assert _base_part(got.state).tobytes() == want.state.tobytes()
            assert not got.state["slot"]["vel"].any() and not got.state["slot"]["pad"].any()
            occupied = got.state["slot"]["base"]["id"] != 0
            for e, name in enumerate(("x1", "y1", "x2", "y2")):
                assert (got.state["slot"]["pos"][..., e] == 256 * got.state["slot"]["base"]["det"][name].astype(np.int64))[occupied].all()


def test_the_helpers_round_toward_zero_and_to_the_nearest_pixel(ptq):
    lib = ms.motion_host()
    values = [0, 1, 127, 128, 129, 255, 256, 257, 383, 384, 385, 1000003, 2 ** 40, 2 ** 42 - 1]
    for g in (0, 1, 13, 128, 192, 255, 256):
        for v in values:
            m = ptq.motion_mul(g, v)
            assert m == (g * v) // 256 and ptq.motion_mul(g, -v) == -m                 # symmetric: toward zero on both sides
            assert lib.yfi_motion_mul_host(g, v) == m and lib.yfi_motion_mul_host(g, -v) == -m
    assert ptq.motion_mul(128, -3) == -1 and (128 * -3) >> 8 == -2                      # not the floor a plain shift would give
    # the pixel of a position: halves go up, on both sides of zero
    for p, want in ((127, 0), (128, 1), (129, 1), (-127, 0), (-128, 0), (-129, -1), (-384, -1), (-385, -2), (383, 1), (384, 2), (0, 0),
                    (256 * ts.I32MAX, ts.I32MAX), (256 * ts.I32MAX + 128, ts.I32MAX), (256 * ts.I32MIN - 129, ts.I32MIN), (2 ** 41, ts.I32MAX),
                    (-2 ** 41, ts.I32MIN), (256 * ts.I32MIN - 128, ts.I32MIN), (256 * ts.I32MIN + 128, ts.I32MIN + 1)):
        assert ptq.motion_box(p) == want and lib.yfi_motion_box_host(p) == want, p
    for v in (ms.I64MIN, ms.I64MAX, ms.LIMIT + 1, -ms.LIMIT - 1, ms.LIMIT, -ms.LIMIT, 5, -5):
        assert ptq.motion_sat(v) == lib.yfi_motion_sat_host(v) == max(-ms.LIMIT, min(ms.LIMIT, v))


def test_untrusted_states_and_extreme_records():
    """states of random bytes, pos and vel at the int64 extremes, records with int32-extreme edges: the host build and the statement agree,
    and whatever was read, what is written lies within the clamp"""
    odd = [(ts.I32MIN, ts.I32MIN, ts.I32MAX, ts.I32MAX), (ts.I32MAX, ts.I32MAX, ts.I32MIN, ts.I32MIN), (ts.I32MAX - 1, 0, ts.I32MAX, ts.I32MAX),
           (ts.I32MIN, ts.I32MIN, ts.I32MIN + 1, ts.I32MIN + 1), (5, 5, 4, 9), (0, 0, 0, 0)]
    near = [(10, 10, 40, 40), (100, 100, 140, 140), (12, 9, 41, 42)]
    for gains in (ms.SUGGESTED + (1,), ms.DIFFERENCE + (0,), (256, 256, 0, 1), (1, 255, 255, 0)):
        for layout in ts.LAYOUTS:
            # random bytes: two streams, the second with a full table
            junk = ms.junk_state(2, full=(1,))
            boxes = [ms.predicted_box(junk, s, k) for s in (0, 1) for k in (3, 17)]
            frames = [[(boxes + near[:1], None), (boxes[:2], None), (near[:1], None)], [(near[1:2] + boxes, None), (odd[:4], None), ([], None)]]
            dets, counts = ts.lay_out(frames, 6, layout)
            both(dets, counts, 2, 3, layout, 6, (0.3, 2, 1) + gains, junk, 64, ("junk", gains, layout))
            # the int64 extremes
            frames = [[(near, None), (near[::-1], None), (odd, None), ([], None), (near, None)]]
            dets, counts = ts.lay_out(frames, 6, layout)
            r = both(dets, counts, 1, 5, layout, 6, (0.1, 1, 3) + gains, ms.extreme_state(), 64, ("extreme", gains, layout))
            occupied = r.state["slot"]["base"]["id"][0] != 0
            assert occupied.any() and (np.abs(r.state["slot"]["pos"][0][occupied]) <= ms.LIMIT).all()
            assert (np.abs(r.state["slot"]["vel"][0][occupied]) <= ms.LIMIT).all()
            # records at the int32 extremes from the empty state: tracks of them are born, matched where proper, and age out
            frames = [[(odd, None), (odd, None), (odd[::-1], None), ([], None), (odd[:2], None)]]
            dets, counts = ts.lay_out(frames, 6, layout)
            both(dets, counts, 1, 5, layout, 6, (0.3, 1, 1) + gains, ms.empty_state(1), 64, ("odd", gains, layout))


def test_one_call_of_many_steps_equals_many_calls_of_one():
    for gains in (ms.SUGGESTED + (0,), (128, 64, 200, 1)):
        dets, counts, want = ms.random_call(ts.TIME, gains)
        got = ts.split_calls(ms.host_run, dets, counts, ms.R_STREAMS, ms.R_STEPS, ms.R_CAP, ms.R_BASE + gains, ms.empty_state(ms.R_STREAMS),
                             ms.R_OUT_CAP)
        assert ts.same(got, want), gains


def test_the_argument_check_rejects_every_fault():
    assert ms.host_check() == "" and ms.host_check(streams=0) == "" and ms.host_check(steps=0, status=8) == ""
    for gains in ((0, 0, 0, 0), (256, 256, 256, 1), (256, 0, 13, 1)):
        assert ms.host_check(params=ts.DEFAULT + gains) == ""
    for kw, text in ms.FAULTS:
        assert text in ms.host_check(**kw), (kw, ms.host_check(**kw))
    # the entry refuses what the check refuses and writes nothing; an empty batch is taken after the checks and writes nothing either
    dets, counts = ts.lay_out(ms.scenario(), ms.S_CAP, ts.TIME)
    state0 = ms.junk_state(1)
    good = ms.S_BASE + ms.SUGGESTED + (0,)
    for params, cap, out_cap in ((ms.S_BASE + (257, 0, 0, 0), ms.S_CAP, 4), (ms.S_BASE + (0, -1, 0, 0), ms.S_CAP, 4), (ms.S_BASE + (0, 0, 300, 0), ms.S_CAP, 4),
                                 (ms.S_BASE + ms.SUGGESTED + (2,), ms.S_CAP, 4), ((float("nan"), 1, 1) + ms.SUGGESTED + (0,), ms.S_CAP, 4),
                                 (good, 0, 4), (good, ms.S_CAP, 0)):
        r = ms.host_run(dets, counts, 1, ms.S_STEPS, ts.TIME, cap, params, state0, out_cap)
        assert r.rc == -1 and r.state.tobytes() == state0.tobytes() and (r.out_counts == ts.SENTINEL32).all(), (params, cap, out_cap)
        assert (r.out.view(np.uint8) == 0xA5).all() and (r.status == ts.SENTINEL32).all(), (params, cap, out_cap)
    for streams0, steps0 in ((0, 5), (1, 0), (0, 0)):
        r = ms.host_run(dets, counts, streams0, steps0, ts.TIME, ms.S_CAP, good, state0, 4)
        assert r.rc == 0 and r.state.tobytes() == state0.tobytes() and (r.out_counts == ts.SENTINEL32).all()
        assert (r.out.view(np.uint8) == 0xA5).all()


def test_the_state_size():
    lib = ms.motion_host()
    assert lib.yf_images_track_motion_state_bytes_host(3) == 3 * 7176 == 3 * ms.MSTATE.itemsize
    assert lib.yf_images_track_motion_state_bytes_host(0) == 0 and lib.yf_images_track_motion_state_bytes_host(-1) == 0
