"""The optimal assignment on the MI355X (yf_images_track_motion_assign_device): the device against the host build of
csrc/yf_images_assign.h, exactly -- records, infos, counts, status and the whole state buffer, every array between guard bytes and every
place that must not be written a sentinel -- on the minimal scene and the sequences of two faces passing each other (once against the
plain-Python statement too, so that this file stands alone); 0, 1, 2, 63 and 64 detections against 0, 1 and 64 occupied slots; the
64 x 64 scene of equal weights (2080 rounds of the search) and the staircase whose last augmenting path runs through all 64 columns;
counts above cap and a full table that drops a detection; 1, 3 and 130 streams by 1 and 7 steps in both layouts; one call of many steps
against many calls of one; one stream's records changed, every other stream's bytes the same; assign = greedy against the motion entry on
the device, and optimal against greedy where no detection and no slot has two eligible partners; an empty batch and the argument
checks; `Tracker(assign="optimal")` with and without `motion=`; and `detect_redacted` with such a tracker on a clip of the real images."""
import ctypes

import numpy as np
import pytest

import assign_support as asg
import motion_support as ms
import track_support as ts
from images_support import Batch, images_after_network, last_error, ptq, real_images, to_host, torch_cuda      # noqa: F401 (fixtures; `images` is images_after_network)

pytestmark = pytest.mark.gpu


def device_run(torch, images, dets, counts, streams, steps, layout, cap, params, assign, state0, out_cap, with_status=True):
    """the device entry on uploaded copies -> ts.Result, as `asg.host_run` gives it"""
    lib = images.load()

    def call(d, c, streams, steps, layout, cap, params, state, out, info, oc, out_cap, status):
        p = ms.c_params(params)
        rc = lib.yf_images_track_motion_assign_device(d, c, streams, steps, layout, cap, ctypes.byref(p), assign, state, out, info, oc, out_cap,
                                                      status, None)
        torch.cuda.synchronize()
        return rc
    return ts.run_with(call, dets, counts, streams, steps, layout, cap, params, state0, out_cap, with_status,
                       upload=lambda a: torch.from_numpy(a.copy()).cuda(), download=lambda b: b.cpu().numpy())


def motion_device_run(torch, images, dets, counts, streams, steps, layout, cap, params, state0, out_cap):
    lib = images.load()

    def call(d, c, streams, steps, layout, cap, params, state, out, info, oc, out_cap, status):
        p = ms.c_params(params)
        rc = lib.yf_images_track_motion_device(d, c, streams, steps, layout, cap, ctypes.byref(p), state, out, info, oc, out_cap, status, None)
        torch.cuda.synchronize()
        return rc
    return ts.run_with(call, dets, counts, streams, steps, layout, cap, params, state0, out_cap,
                       upload=lambda a: torch.from_numpy(a.copy()).cuda(), download=lambda b: b.cpu().numpy())


def same_as_host(torch, images, dets, counts, streams, steps, layout, cap, params, state0, out_cap, what, assign=asg.OPTIMAL):
    want = asg.host_run(dets, counts, streams, steps, layout, cap, params, assign, state0, out_cap)
    got = device_run(torch, images, dets, counts, streams, steps, layout, cap, params, assign, state0, out_cap)
    assert want.rc == streams * steps and ts.same(got, want), what
    return got


def test_device_equals_the_host_build_on_the_minimal_scene_and_the_crossing_sequences(torch_cuda, images):
    for gains in (asg.BASE_GAINS, asg.SUGGESTED):
        params = asg.M_PARAMS + gains
        for layout in ts.LAYOUTS:
            dets, counts = ts.lay_out(asg.minimal_frames(), 2, layout)
            o = same_as_host(torch_cuda, images, dets, counts, 1, 2, layout, 2, params, ms.empty_state(1), 4, ("minimal", gains, layout))
            g = same_as_host(torch_cuda, images, dets, counts, 1, 2, layout, 2, params, ms.empty_state(1), 4, ("minimal", gains, layout), asg.GREEDY)
        # greedy strands d1 (a third id, track 2 held over); optimal keeps both ids
        assert ms.boxes_of(g, 1) == [(1, *asg.D0, 0), (2, *asg.B, 1), (3, *asg.D1, 0)] and int(g.state["issued"][0]) == 3
        assert ms.boxes_of(o, 1) == [(1, *asg.D1, 0), (2, *asg.D0, 0)] and int(o.state["issued"][0]) == 2
        for layout in ts.LAYOUTS:
            dets, counts = ts.lay_out(asg.crossing_frames(), asg.C_CAP, layout)
            got = same_as_host(torch_cuda, images, dets, counts, 2, asg.C_STEPS, layout, asg.C_CAP, params, ms.empty_state(2), 8, ("crossing", gains, layout))
        # ... and the host build is the statement (tests/test_track_assign_host.py); here too, so that this file stands alone
        assert ts.same(got, asg.expected(dets, counts, 2, asg.C_STEPS, layout, asg.C_CAP, params, asg.OPTIMAL, ms.empty_state(2), 8)), gains
        assert got.state["issued"].tolist() == [2, 2]


def sweep_scene():
    """15 streams of two steps at cap 64: stream 3 a + b has (0, 1, 2, 63, 64)[a] detections against (0, 1, 64)[b] occupied slots, boxes
    of side 20 .. 80 thrown into a square of 150 so that most pairs overlap; the second step meets what the first left"""
    rng = np.random.default_rng(7300)

    def box():
        x, y, w, h = (int(v) for v in (rng.integers(0, 150), rng.integers(0, 150), rng.integers(20, 81), rng.integers(20, 81)))
        return (x, y, x + w - 1, y + h - 1)
    states, frames = [], []
    for m in (0, 1, 2, 63, 64):
        for occupied in (0, 1, 64):
            slots = sorted(int(k) for k in rng.choice(64, occupied, replace=False))
            states.append(asg.scene_state({k: box() for k in slots}, issued=64))
            frames.append([([box() for _ in range(m)], None), ([box() for _ in range(m)], None)])
    return np.concatenate(states), frames


def test_every_number_of_detections_against_every_number_of_occupied_slots(torch_cuda, images):
    state0, frames = sweep_scene()
    for match_iou in (0.05, 0.3):
        for layout in ts.LAYOUTS:
            dets, counts = ts.lay_out(frames, 64, layout)
            got = same_as_host(torch_cuda, images, dets, counts, 15, 2, layout, 64, (match_iou, 1, 1) + asg.SUGGESTED, state0, 64, (match_iou, layout))
        greedy = asg.host_run(dets, counts, 15, 2, layout, 64, (match_iou, 1, 1) + asg.SUGGESTED, asg.GREEDY, state0, 64)
        assert not ts.same(got, greedy)                                                # scenes on which the two matches part
    assert (got.status & 2).any() and (got.out_counts == 64).any() and (got.out_counts == 0).any()


def test_the_dense_scenes_all_weights_equal_and_the_staircase(torch_cuda, images):
    for layout in ts.LAYOUTS:
        state0, frames = asg.all_equal_state()
        dets, counts = ts.lay_out(frames, 64, layout)
        r = same_as_host(torch_cuda, images, dets, counts, 1, 2, layout, 64, (0.3, 1, 2) + asg.SUGGESTED, state0, 64, ("equal", layout))
        assert (r.out_counts == 64).all() and not r.status.any() and (r.info["misses"] == 0).all() and int(r.state["issued"][0]) == 64
        # the recorded assignment of the tie rule: detection i to slot i -- every track's record carries its own slot's `col` field (j % 7)
        first = ts.frame_of(0, 0, 1, 2, layout)
        assert r.info["id"][first].tolist() == list(range(1, 65)) and r.out["col"][first].tolist() == [k % 7 for k in range(64)]
        boxes, stair = asg.staircase_scene()
        dets, counts = ts.lay_out([[(stair, None), (stair[:40] + [(900, 900, 950, 950)] * 3, None)]], 64, layout)
        r = same_as_host(torch_cuda, images, dets, counts, 1, 2, layout, 64, (asg.STAIR_IOU, 1, 2) + asg.BASE_GAINS, asg.scene_state(boxes), 64,
                         ("stair", layout))
        first = ts.frame_of(0, 0, 1, 2, layout)
        # detection i (the strip over 64 - i tiles) ends on slot 63 - i: track k + 1 reports the strip over k + 1 tiles
        assert (r.info["misses"][first] == 0).all() and r.out["x2"][first].tolist() == [10 * k + 9 for k in range(64)]
        assert r.status.tolist() == [0, 2]                                            # then a full table drops births (bit 1)


def test_counts_above_cap_a_full_table_random_bytes_and_the_random_sequences(torch_cuda, images):
    for layout in ts.LAYOUTS:
        # tests/track_support.py's crowded sequences: up to 70 records a frame (bit 0), a table that fills up and drops (bit 1), ties
        dets, counts = ts.lay_out(ts.random_frames(), ts.R_CAP, layout)
        r = same_as_host(torch_cuda, images, dets, counts, ts.R_STREAMS, ts.R_STEPS, layout, ts.R_CAP, ts.R_PARAMS + asg.SUGGESTED,
                         ms.empty_state(ts.R_STREAMS), ts.R_OUT_CAP, ("crowded", layout))
        assert (r.status == 3).any() and (counts > 64).any() and (r.out_counts > ts.R_OUT_CAP).any()
        case = next(c for c in ts.designed() if c.name == "counts")
        d2, c2, streams, steps, base0 = ts.laid_out(case, layout)
        r = same_as_host(torch_cuda, images, d2, c2, streams, steps, layout, case.cap, tuple(case.params) + asg.SUGGESTED, ms.lift(base0), case.out_cap,
                         ("counts", layout))
        assert (r.status & 1).any()
        bare = device_run(torch_cuda, images, d2, c2, streams, steps, layout, case.cap, tuple(case.params) + asg.SUGGESTED, asg.OPTIMAL, ms.lift(base0),
                          case.out_cap, with_status=False)
        assert (bare.status == ts.SENTINEL32).all() and ts.same(bare._replace(status=r.status), r)
        for gains in (ms.SUGGESTED + (1,), (128, 64, 200, 1)):
            d3, c3 = ts.lay_out(ms.random_frames(), ms.R_CAP, layout)
            same_as_host(torch_cuda, images, d3, c3, ms.R_STREAMS, ms.R_STEPS, layout, ms.R_CAP, ms.R_BASE + gains, ms.empty_state(ms.R_STREAMS),
                         ms.R_OUT_CAP, ("random", gains, layout))
        d4, c4, junk = asg.junk_call(layout)
        same_as_host(torch_cuda, images, d4, c4, 2, 3, layout, 6, (0.3, 2, 1) + ms.SUGGESTED + (1,), junk, 64, ("junk", layout))
        near = [(10, 10, 40, 40), (100, 100, 140, 140), (12, 9, 41, 42)]
        d5, c5 = ts.lay_out([[(near, None), (near[::-1], None), ([], None), (near, None)]], 3, layout)
        same_as_host(torch_cuda, images, d5, c5, 1, 4, layout, 3, (0.1, 1, 3) + ms.DIFFERENCE + (1,), ms.extreme_state(), 64, ("extreme", layout))


def crowd_frames(streams, steps):
    """`ts.drift_frames` with a second copy of every box a few pixels beside it: every frame has detections with two eligible tracks"""
    frames = []
    for clip in ts.drift_frames(streams, steps):
        frames.append([(boxes + [(x1 + 4, y1 + 3, x2 + 4, y2 + 3) for x1, y1, x2, y2 in boxes][:3], None) for boxes, _ in clip])
    return frames


@pytest.mark.parametrize("streams", [1, 3, 130])
def test_streams_by_steps_in_both_layouts(torch_cuda, images, streams):
    cap, out_cap, params = 10, 6, (0.3, 2, 1) + asg.SUGGESTED
    for steps in (1, 7):
        frames = crowd_frames(streams, steps)
        results = {}
        for layout in ts.LAYOUTS:
            dets, counts = ts.lay_out(frames, cap, layout)
            results[layout] = same_as_host(torch_cuda, images, dets, counts, streams, steps, layout, cap, params, ms.empty_state(streams), out_cap,
                                           (streams, steps, layout))
        assert ts.by_frame(results[ts.TIME], streams, steps, ts.TIME) == ts.by_frame(results[ts.STREAM], streams, steps, ts.STREAM)
    assert (results[ts.TIME].out_counts > 0).any() and results[ts.TIME].state["issued"].all()       # at 7 steps every stream has had tracks


def test_a_workgroup_that_takes_a_second_stream(torch_cuda, images):
    """more streams than the launch has workgroups (the device's CUs times the launcher's own number per CU; the table of weights in LDS
    is reused for the second stream without a barrier): the device against the host build in every byte, from the empty state and from
    the state that call left"""
    grid = torch_cuda.cuda.get_device_properties(0).multi_processor_count * ts.per_cu("Assign")
    host = lambda d, c, streams, steps, layout, cap, p, state0, out_cap: asg.host_run(d, c, streams, steps, layout, cap, p, asg.OPTIMAL, state0, out_cap)
    device = lambda d, c, streams, steps, layout, cap, p, state0, out_cap: device_run(torch_cuda, images, d, c, streams, steps, layout, cap, p,
                                                                                     asg.OPTIMAL, state0, out_cap)
    ts.beyond_the_grid(device, host, grid, (0.3, 2, 1) + asg.SUGGESTED, ms.empty_state)


def test_one_call_of_many_steps_equals_many_calls_of_one(torch_cuda, images):
    params = ms.R_BASE + asg.SUGGESTED
    dets, counts = ts.lay_out(ms.random_frames(), ms.R_CAP, ts.TIME)
    want = asg.host_run(dets, counts, ms.R_STREAMS, ms.R_STEPS, ts.TIME, ms.R_CAP, params, asg.OPTIMAL, ms.empty_state(ms.R_STREAMS), ms.R_OUT_CAP)
    run = lambda d, c, streams, steps, layout, cap, p, state0, out_cap: device_run(torch_cuda, images, d, c, streams, steps, layout, cap, p, asg.OPTIMAL,
                                                                                 state0, out_cap)
    got = ts.split_calls(run, dets, counts, ms.R_STREAMS, ms.R_STEPS, ms.R_CAP, params, ms.empty_state(ms.R_STREAMS), ms.R_OUT_CAP)
    assert ts.same(got, want)


def test_one_streams_records_change_no_other_streams_bytes(torch_cuda, images):
    streams, steps, cap, out_cap, params = 5, 7, 10, 6, (0.3, 1, 2) + ms.SUGGESTED + (1,)
    frames = crowd_frames(streams, steps)
    other = [list(clip) for clip in frames]
    other[2] = [([(7, 7, 30 + t, 30), (200, 100, 240, 150 - t), (9, 8, 33 + t, 31)], None) for t in range(steps)]
    for layout in ts.LAYOUTS:
        a = device_run(torch_cuda, images, *ts.lay_out(frames, cap, layout), streams, steps, layout, cap, params, asg.OPTIMAL, ms.empty_state(streams), out_cap)
        b = device_run(torch_cuda, images, *ts.lay_out(other, cap, layout), streams, steps, layout, cap, params, asg.OPTIMAL, ms.empty_state(streams), out_cap)
        for s in range(streams):
            rows = [ts.frame_of(s, t, streams, steps, layout) for t in range(steps)]
            equal = all(x[rows].tobytes() == y[rows].tobytes() for x, y in zip(a[2:], b[2:])) and a.state[s].tobytes() == b.state[s].tobytes()
            assert equal == (s != 2), (layout, s)


def test_greedy_is_the_motion_entry_and_optimal_is_greedy_where_no_pair_competes(torch_cuda, images):
    for layout in ts.LAYOUTS:
        calls = [(*ts.lay_out(ms.random_frames(), ms.R_CAP, layout), ms.R_STREAMS, ms.R_STEPS, layout, ms.R_CAP, ms.R_BASE + asg.SUGGESTED,
                  ms.empty_state(ms.R_STREAMS), ms.R_OUT_CAP),
                 (*ts.lay_out(asg.crossing_frames(), asg.C_CAP, layout), 2, asg.C_STEPS, layout, asg.C_CAP, asg.M_PARAMS + asg.BASE_GAINS,
                  ms.empty_state(2), 8)]
        d, c, junk = asg.junk_call(layout)
        calls.append((d, c, 2, 3, layout, 6, (0.3, 2, 1) + ms.SUGGESTED + (1,), junk, 64))
        for dets, counts, streams, steps, layout, cap, params, state0, out_cap in calls:
            want = motion_device_run(torch_cuda, images, dets, counts, streams, steps, layout, cap, params, state0, out_cap)
            got = device_run(torch_cuda, images, dets, counts, streams, steps, layout, cap, params, asg.GREEDY, state0, out_cap)
            assert want.rc == streams * steps and ts.same(got, want), (layout, cap)
        # the sequences of tests/test_track_assign_host.py on which every detection and every slot has at most one eligible partner
        frames = asg.sparse_frames()
        streams, steps, cap = len(frames), len(frames[0]), 8
        for gains in (asg.SUGGESTED, asg.BASE_GAINS):
            params = (0.3, 1, 2) + gains
            dets, counts = ts.lay_out(frames, cap, layout)
            assert asg.max_degree(dets, counts, streams, steps, layout, cap, params, ms.empty_state(streams)) == 1
            g = device_run(torch_cuda, images, dets, counts, streams, steps, layout, cap, params, asg.GREEDY, ms.empty_state(streams), 8)
            o = device_run(torch_cuda, images, dets, counts, streams, steps, layout, cap, params, asg.OPTIMAL, ms.empty_state(streams), 8)
            assert g.rc == streams * steps and ts.same(g, o) and (g.out_counts > 1).any(), (gains, layout)


def test_an_empty_batch_and_the_argument_checks(torch_cuda, images):
    torch = torch_cuda
    lib = images.load()
    # every fault is refused before anything is launched: the addresses of these calls are made up and never used
    names = ("dets", "counts", "streams", "steps", "layout", "cap", "params", "assign", "state", "out", "info", "out_counts", "out_cap", "status")
    faults = [(kw, assign, text) for kw, text in ms.FAULTS for assign in (asg.OPTIMAL, asg.GREEDY, 7)]
    faults += [({}, bad, "assign must be") for bad in asg.BAD_ASSIGNS]
    for kw, assign, text in faults:
        a = dict(ms.VALID, assign=assign, **kw)
        p = None if a["params"] is None else ctypes.byref(ms.c_params(a["params"]))
        rc = lib.yf_images_track_motion_assign_device(*(p if k == "params" else (a[k] or None) if k in ("dets", "counts", "state", "out", "info", "out_counts", "status")
                                                        else a[k] for k in names), None)
        assert rc == -1 and text in last_error(lib), (kw, assign, rc, last_error(lib))
    # a refused call with real arrays writes nothing; neither does an empty batch, which is taken after the checks
    dets, counts = ts.lay_out(ms.scenario(), ms.S_CAP, ts.TIME)
    state0 = ms.junk_state(1)
    good = ms.S_BASE + asg.SUGGESTED
    for params, assign, cap in ((good, 2, ms.S_CAP), (good, -1, ms.S_CAP), (ms.S_BASE + (257, 0, 0, 0), asg.OPTIMAL, ms.S_CAP), (good, asg.OPTIMAL, 0),
                                (good, asg.OPTIMAL, 1201), (ms.S_BASE + ms.SUGGESTED + (2,), asg.GREEDY, ms.S_CAP)):
        r = device_run(torch, images, dets, counts, 1, ms.S_STEPS, ts.TIME, cap, params, assign, state0, 4)
        assert r.rc == -1 and r.state.tobytes() == state0.tobytes() and (r.out_counts == ts.SENTINEL32).all(), (params, assign, cap)
    for assign in (asg.OPTIMAL, asg.GREEDY):
        for streams0, steps0 in ((0, 5), (1, 0), (0, 0)):
            r = device_run(torch, images, dets, counts, streams0, steps0, ts.TIME, ms.S_CAP, good, assign, state0, 4)
            assert r.rc == 0 and r.state.tobytes() == state0.tobytes() and (r.out_counts == ts.SENTINEL32).all()
            assert (r.out.view(np.uint8) == 0xA5).all() and (r.status == ts.SENTINEL32).all()
    with pytest.raises(images.ImagesError, match="beta"):
        images.track_motion_assign_device(8, 8, 1, 1, "time", 4, (0.3, 1, 1, 256, 300, 0, 0), "optimal", 8, 8, 8, 8, 4)
    with pytest.raises(ValueError, match="assign"):
        images.track_motion_assign_device(8, 8, 1, 1, "time", 4, (0.3, 1, 1, 256, 0, 0, 0), "hungarian", 8, 8, 8, 8, 4)
    with pytest.raises(ValueError, match="assign"):
        images.Tracker(1, assign="best")
    assert images.Tracker(2).d_state.shape == (2, 2824) and images.Tracker(2, assign="greedy", motion=True).d_state.shape == (2, 7176)
    assert images.Tracker(2, assign="optimal").d_state.shape == (2, 7176) and images.Tracker(2, assign="optimal").motion is None
    assert images.Tracker(1, motion=True, smooth=True, assign="OPTIMAL").assign == "optimal"


def test_a_tracker_with_assign_optimal_equals_the_statement_with_and_without_motion(torch_cuda, images, ptq):
    torch = torch_cuda
    frames = asg.crossing_frames()
    dets, counts = ts.lay_out(frames, asg.C_CAP, ts.TIME)
    n = 2 * asg.C_STEPS
    d_dets = torch.from_numpy(dets.view(np.uint8).reshape(n, asg.C_CAP, 28).copy()).cuda()
    d_counts = torch.from_numpy(counts.copy()).cuda()
    seen = {}
    for motion, gains in ((None, asg.BASE_GAINS), (True, asg.SUGGESTED), (ms.DIFFERENCE, ms.DIFFERENCE + (0,))):
        for assign in ("optimal", "greedy"):
            tracker = images.Tracker(2, *asg.M_PARAMS, motion=motion, assign=assign)
            # the clip in two calls: the tracker carries on
            first = tracker.update(d_dets[:10], d_counts[:10], 5, "time", out_cap=8)
            second = tracker.update(d_dets[10:], d_counts[10:], asg.C_STEPS - 5, "time", out_cap=8)
            torch.cuda.synchronize()
            got = images._track_tuples(*first[:3], 10) + images._track_tuples(*second[:3], n - 10)
            want = [None] * n
            for s in range(2):
                state = ptq.track_motion_empty_state()
                for t in range(asg.C_STEPS):
                    f = ts.frame_of(s, t, 2, asg.C_STEPS, ts.TIME)
                    recs = [tuple(r) for r in dets[f, :counts[f]].view(images.binding.DET_DTYPE).tolist()]
                    state, emitted, status = ptq.track_motion_step(state, recs, asg.M_PARAMS + gains, frame=f, assign=assign)
                    want[f] = [(i, r[6], r[7], r[8], r[9], r[5], hits, misses) for r, (i, hits, misses, _) in emitted]
            assert got == want, (motion, assign)
            seen[motion if motion is None or motion is True else "difference", assign] = got
    assert seen[None, "optimal"] != seen[None, "greedy"]                              # without a motion model the matches part on this clip
    # ... and a plain tracker (the 2824-byte state) is assign="greedy", motion=None as before
    plain = images.Tracker(2, *asg.M_PARAMS)
    out = plain.update(d_dets, d_counts, asg.C_STEPS, "time", out_cap=8)
    torch.cuda.synchronize()
    assert images._track_tuples(*out[:3], n) == seen[None, "greedy"] and plain.d_state.shape == (2, 2824)


def _regions(ptq, rows, w, h):
    return [ptq.crop_region(tuple(row[1:5]), w, h) for row in rows]


def test_detect_redacted_with_an_optimal_tracker_on_a_clip_of_the_real_images(network, torch_cuda, images, ptq, yf):
    """two streams of three frames from the real images -- image s, image s again, a picture without a face (the track is held over) --
    against `ptq.track_motion_step(assign="optimal")` over the records of the same frames, then `ptq.redact_u8` over the reported tracks"""
    torch = torch_cuda
    real = real_images(ptq)
    streams, steps = 2, 3

    def blank(like):
        y, x = np.mgrid[:like.shape[0], :like.shape[1]]
        return np.repeat((127 + 2 * ((x + y) % 8 < 4)).astype(np.uint8)[..., None], 3, axis=2)
    pictures = [(real[s], real[s], blank(real[s]))[t] for t in range(steps) for s in range(streams)]          # time-major
    b = Batch(torch, images, pictures, 0)
    b.run_decode(images, network)
    images.nms_device(b.d_dets.data_ptr(), b.d_counts.data_ptr(), b.n, b.cap, 0.4)
    dets, counts = to_host(yf, b.d_dets, b.d_counts, b.cap)
    params = (0.3, 1, 5) + asg.SUGGESTED
    want = [None] * b.n
    for s in range(streams):
        state = ptq.track_motion_empty_state()
        for t in range(steps):
            f = ts.frame_of(s, t, streams, steps, ts.TIME)
            state, emitted, status = ptq.track_motion_step(state, dets[f, :counts[f]].tolist(), params, frame=f, assign="optimal")
            want[f] = [(i, r[6], r[7], r[8], r[9], r[5], hits, misses) for r, (i, hits, misses, _) in emitted]
            assert status == 0
    blanks = [ts.frame_of(s, 2, streams, steps, ts.TIME) for s in range(streams)]
    assert all(counts[f] == 0 for f in blanks) and all(want[f] and all(w[7] == 1 for w in want[f]) for f in blanks)
    got, tracks = images.detect_redacted(network, pictures, tracker=images.Tracker(streams, motion=True, assign="optimal"), layout="time")
    assert tracks == want
    for f, p in enumerate(pictures):
        assert np.array_equal(got[f], ptq.redact_u8(p, _regions(ptq, want[f], p.shape[1], p.shape[0]), "mosaic", 8, None)), f
    assert all(not np.array_equal(got[f], pictures[f]) for f in blanks)               # the frame without a face is hidden too
