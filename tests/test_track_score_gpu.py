"""The score of tracks against labelled identities on the MI355X (yf_images_score_tracks_device): the device against the host build of
csrc/yf_images_score.h, exactly -- the whole state, the matches and the status, every array between guard bytes and every place that must
not be written a sentinel -- on the designed scenes (once against the plain-Python statement too, so that this file stands alone); 0, 1,
2, 63 and 64 rows against 0, 1 and 64 columns; the 64 x 64 table of equal weights (2080 rounds of the search) and the staircase whose last
augmenting path runs through all 64 columns; 1, 3 and 130 streams by 1 and 7 steps in both layouts; one call of many steps against many
calls of one; d_match and d_status NULL; more streams than the launch has workgroups; an empty batch and the argument checks;
`TrackScore` on what a `Tracker` reported on the device; and `evaluate_tracking` on a still video of the real images."""
import numpy as np
import pytest

import assign_support as asg
import score_support as sc
import track_support as ts
from images_support import images_after_network, last_error, ptq, real_images, torch_cuda      # noqa: F401 (fixtures; `images` is images_after_network)

pytestmark = pytest.mark.gpu


def device_run(torch, images, call, streams, steps, layout, gt_cap, out_cap, score_iou, state0, with_match=True, with_status=True):
    """the device entry on uploaded copies -> sc.Result, as `sc.host_run` gives it"""
    lib = images.load()

    def fn(*a):
        rc = lib.yf_images_score_tracks_device(*a, None)
        torch.cuda.synchronize()
        return rc
    return sc.run_with(fn, call, streams, steps, layout, gt_cap, out_cap, score_iou, state0, with_match, with_status,
                       upload=lambda a: torch.from_numpy(a.copy()).cuda(), download=lambda b: b.cpu().numpy())


def same_as_host(torch, images, call, streams, steps, layout, gt_cap, out_cap, score_iou, state0, what):
    want = sc.host_run(call, streams, steps, layout, gt_cap, out_cap, score_iou, state0)
    got = device_run(torch, images, call, streams, steps, layout, gt_cap, out_cap, score_iou, state0)
    assert want.rc == streams * steps and sc.same(got, want), what
    return got


def test_device_equals_the_host_build_and_the_statement_on_the_designed_scenes(torch_cuda, images):
    for case in sc.designed():
        for layout in ts.LAYOUTS:
            call, streams, steps, state0 = sc.laid_out(case, layout)
            got = same_as_host(torch_cuda, images, call, streams, steps, layout, case.gt_cap, case.out_cap, case.score_iou, state0, (case.name, layout))
            # ... and the host build is the statement (tests/test_track_score_host.py); here too, so that this file stands alone
            assert sc.same(got, sc.expected(call, streams, steps, layout, case.gt_cap, case.out_cap, case.score_iou, state0)), (case.name, layout)
        if case.name == "swap":
            assert int(got.state["switches"][0]) == 2 and int(got.state["matches"][0]) == 10 and got.match.tolist() == [[0, 1]] * 5
        if case.name == "voids":
            assert got.status.tolist() == [sc.GT_VOID, sc.HYP_VOID, sc.GT_CLIPPED, sc.HYP_CLIPPED, 15, 0, 0]


def test_every_number_of_rows_against_every_number_of_columns(torch_cuda, images):
    frames = sc.sweep_frames()
    for score_iou in (0.05, 0.5):
        for layout in ts.LAYOUTS:
            call = sc.lay_out(frames, 64, 64, layout)
            r = same_as_host(torch_cuda, images, call, 15, 2, layout, 64, 64, score_iou, sc.empty_state(15), (score_iou, layout))
    assert (r.state["matches"] > 0).any() and (r.state["switches"] > 0).any() and (r.state["misses"] > 0).any()


def test_the_dense_tables_all_weights_equal_and_the_staircase(torch_cuda, images):
    for layout in ts.LAYOUTS:
        r = same_as_host(torch_cuda, images, sc.lay_out(sc.equal_frames(), 64, 64, layout), 1, 2, layout, 64, 64, 0.3, sc.empty_state(1), ("equal", layout))
        first, second = ts.frame_of(0, 0, 1, 2, layout), ts.frame_of(0, 1, 1, 2, layout)
        assert r.match[first].tolist() == list(range(64)) and r.match[second].tolist() == list(range(63, -1, -1))
        assert int(r.state["matches"][0]) == 128 and int(r.state["switches"][0]) == 0
        r = same_as_host(torch_cuda, images, sc.lay_out(sc.staircase_frames(), 64, 64, layout), 1, 2, layout, 64, 64, asg.STAIR_IOU,
                         sc.junk_state(1), ("stair", layout))
        assert r.match[first].tolist() == list(range(63, -1, -1))


@pytest.mark.parametrize("streams", [1, 3, 130])
def test_streams_by_steps_in_both_layouts(torch_cuda, images, streams):
    for steps in (1, 7):
        frames = sc.drift_frames(streams, steps)
        results = {}
        for layout in ts.LAYOUTS:
            call = sc.lay_out(frames, sc.D_GT_CAP, sc.D_OUT_CAP, layout)
            results[layout] = same_as_host(torch_cuda, images, call, streams, steps, layout, sc.D_GT_CAP, sc.D_OUT_CAP, 0.5, sc.junk_state(streams),
                                           (streams, steps, layout))
        assert results[ts.TIME].state.tobytes() == results[ts.STREAM].state.tobytes()
    assert (results[ts.TIME].status != 0).any() or streams == 1


def test_one_call_of_many_steps_equals_many_calls_of_one_with_and_without_the_optional_outputs(torch_cuda, images):
    streams, steps = 3, 40
    call = sc.lay_out(sc.drift_frames(streams, steps), sc.D_GT_CAP, sc.D_OUT_CAP, ts.TIME)
    want = sc.host_run(call, streams, steps, ts.TIME, sc.D_GT_CAP, sc.D_OUT_CAP, 0.5, sc.junk_state(streams))
    run = lambda part, streams, steps, layout, gt_cap, out_cap, score_iou, state0: device_run(torch_cuda, images, part, streams, steps, layout, gt_cap,
                                                                                           out_cap, score_iou, state0)
    got = sc.split_calls(run, call, streams, steps, sc.D_GT_CAP, sc.D_OUT_CAP, 0.5, sc.junk_state(streams))
    assert sc.same(got, want) and (want.state["switches"] != sc.junk_state(streams)["switches"]).any()
    bare = device_run(torch_cuda, images, call, streams, steps, ts.TIME, sc.D_GT_CAP, sc.D_OUT_CAP, 0.5, sc.junk_state(streams), with_match=False,
                      with_status=False)
    assert (bare.match == ts.SENTINEL32).all() and (bare.status == ts.SENTINEL32).all() and bare.state.tobytes() == want.state.tobytes()
    half = device_run(torch_cuda, images, call, streams, steps, ts.TIME, sc.D_GT_CAP, sc.D_OUT_CAP, 0.5, sc.junk_state(streams), with_match=False)
    assert (half.match == ts.SENTINEL32).all() and half.status.tobytes() == want.status.tobytes()


def test_a_workgroup_that_takes_a_second_stream(torch_cuda, images):
    """three streams more than the launch has workgroups (the device's CUs times the launcher's own number per CU): a workgroup's
    counters and tables are reloaded for its second stream and the table of weights in LDS is reused without a barrier; two steps at
    caps 4, then the same again in the other layout on the state the first call left"""
    streams, steps, cap = torch_cuda.cuda.get_device_properties(0).multi_processor_count * sc.per_cu() + 3, 2, 4
    frames = [[(truths[:cap], hyps[:cap], None, None) for truths, hyps, _, _ in clip] for clip in sc.drift_frames(streams, steps)]
    state = sc.empty_state(streams)
    for layout in ts.LAYOUTS:
        got = same_as_host(torch_cuda, images, sc.lay_out(frames, cap, cap, layout), streams, steps, layout, cap, cap, 0.5, state, layout)
        state = got.state
    assert (got.state["frames"] == 4).all() and (got.state["matches"] > 0).mean() > 0.9


def test_an_empty_batch_and_the_argument_checks(torch_cuda, images):
    lib = images.load()
    # every fault is refused before anything is launched: the addresses of these calls are made up and never used
    for kw, text in sc.FAULTS:
        a = dict(sc.VALID, **kw)
        rc = lib.yf_images_score_tracks_device(*((a[k] or None) if k in sc.POINTERS else a[k] for k in sc.NAMES), None)
        assert rc == -1 and text in last_error(lib), (kw, rc, last_error(lib))
    case = next(c for c in sc.designed() if c.name == "swap")
    call, streams, steps, _ = sc.laid_out(case, ts.TIME)
    state0 = sc.junk_state(1)
    for gt_cap, out_cap, score_iou, layout in ((65, 2, 0.5, ts.TIME), (0, 2, 0.5, ts.TIME), (2, 0, 0.5, ts.TIME), (2, 2, float("nan"), ts.TIME), (2, 2, 0.5, 2)):
        def fn(*p):
            a = dict(zip(sc.NAMES, p), gt_cap=gt_cap, out_cap=out_cap, score_iou=score_iou, layout=layout)
            return lib.yf_images_score_tracks_device(*(a[k] for k in sc.NAMES), None)
        r = sc.run_with(fn, call, 1, steps, ts.TIME, 2, 2, 0.5, state0, upload=lambda a: torch_cuda.from_numpy(a.copy()).cuda(),
                        download=lambda b: b.cpu().numpy())
        assert r.rc == -1 and r.state.tobytes() == state0.tobytes() and (r.match == ts.SENTINEL32).all() and (r.status == ts.SENTINEL32).all()
    for streams0, steps0 in ((0, 5), (1, 0), (0, 0)):
        r = device_run(torch_cuda, images, call, streams0, steps0, ts.TIME, 2, 2, 0.5, state0)
        assert r.rc == 0 and r.state.tobytes() == state0.tobytes() and (r.match == ts.SENTINEL32).all() and (r.status == ts.SENTINEL32).all()
    assert images.score_state_bytes(3) == 3 * 3136 and images.score_state_bytes(0) == 0
    with pytest.raises(images.ImagesError, match="gt_cap"):
        images.score_tracks_device(8, 8, 8, 4, 8, 8, 65, 1, 1, "time", 0.5, 8)
    with pytest.raises(ValueError, match="layout"):
        images.score_tracks_device(8, 8, 8, 4, 8, 8, 4, 1, 1, "rows", 0.5, 8)
    with pytest.raises(ValueError, match="at most 64"):
        images.pack_track_truth([[(k + 1, 0, 0, 9, 9) for k in range(65)]])
    gt, counts = images.pack_track_truth([[(3, 1, 2, 3, 4)], [], [(1, 0, 0, 9, 9), (2, 5, 5, 8, 8)]])
    assert gt.shape == (3, 2) and counts.tolist() == [1, 0, 2] and gt[2, 1].tolist() == (2, 5, 5, 8, 8) and gt.dtype.itemsize == 20
    assert sc.same_summary(images.score_summary(sc.junk_state(3)), sc.py_summary(sc.junk_state(3)))


def test_a_track_score_of_what_a_tracker_reported_on_the_device(torch_cuda, images):
    torch = torch_cuda
    frames, truth = [asg.crossing_frames()[1]], [sc.clip_truth()[1]]                     # the pan
    dets, counts = ts.lay_out(frames, asg.C_CAP, ts.TIME)
    d_dets = torch.from_numpy(dets.view(np.uint8).reshape(asg.C_STEPS, asg.C_CAP, 28).copy()).cuda()
    d_counts = torch.from_numpy(counts.copy()).cuda()
    gt, gt_counts = sc.truth_arrays(truth, 2, ts.TIME)
    d_gt = torch.from_numpy(gt.view(np.uint8).reshape(asg.C_STEPS, 2, 20).copy()).cuda()
    d_gt_counts = torch.from_numpy(gt_counts.copy()).cuda()
    seen = {}
    for assign, code in (("greedy", asg.GREEDY), ("optimal", asg.OPTIMAL)):
        tracker = images.Tracker(1, *sc.TRACKER, assign=assign)
        score = images.TrackScore(1, sc.SCORE_IOU)
        # the clip in two calls: the tracker and the score carry on
        for lo, hi in ((0, 5), (5, asg.C_STEPS)):
            d_out, d_info, d_out_counts, _ = tracker.update(d_dets[lo:hi], d_counts[lo:hi], hi - lo, "time", out_cap=8)
            d_match, d_status = score.update(d_out, d_info, d_out_counts, d_gt[lo:hi], d_gt_counts[lo:hi], hi - lo, "time", with_match=True)
        got = score.summary()
        tracked = sc.tracked_on_host(frames, asg.C_CAP, asg.BASE_GAINS, code)
        want = sc.host_run((tracked.out, tracked.info, tracked.out_counts, gt, gt_counts), 1, asg.C_STEPS, ts.TIME, 2, 8, sc.SCORE_IOU, sc.empty_state(1))
        assert sc.same_summary(got, sc.host_summary(want.state)) and score.states().tobytes() == want.state.tobytes(), assign
        assert d_match.cpu().numpy().tobytes() == want.match[5:].tobytes() and not d_status.cpu().numpy().any()
        seen[assign] = got
        score.reset()
        assert score.summary()["frames"] == 0
    assert seen["greedy"]["switches"] > 0 and seen["greedy"]["false_positives"] > 0
    assert seen["optimal"]["switches"] == 0 and seen["optimal"]["mota"] == 1.0


def test_evaluate_tracking_on_a_still_video_of_the_real_images(network, torch_cuda, images, ptq):
    """three of the real pictures, each repeated for 4 steps as one stream; the labelled objects are `detect`'s suppressed boxes with the
    ids 1, 2, ... in their order: every face is tracked from the first frame on, nothing is missed, nothing is reported beside them"""
    real = real_images(ptq)
    streams, steps = 3, 4
    pictures = [real[s] for t in range(steps) for s in range(streams)]                     # time-major
    boxes = images.detect(network, pictures, iou_threshold=0.4)
    truths = [[(k + 1, *(int(v) for v in box)) for k, box in enumerate(b)] for b in boxes]
    assert sum(len(t) for t in truths) > 0 and max(len(t) for t in truths) <= 64
    got = images.evaluate_tracking(network, pictures, truths, images.Tracker(streams, min_hits=1), steps, layout="time")
    assert (got["switches"], got["misses"], got["false_positives"], got["mota"]) == (0, 0, 0, 1.0)
    assert got["frames"] == streams * steps and got["gt"] == got["matches"] == sum(len(t) for t in truths) and got["mostly_lost"] == 0
    # ... equal to the statement over the downloaded records
    tracks = images.detect_tracked(network, pictures, images.Tracker(streams, min_hits=1), steps, layout="time")
    states = []
    for s in range(streams):
        st = ptq.track_score_empty_state()
        for t in range(steps):
            f = ts.frame_of(s, t, streams, steps, ts.TIME)
            st = ptq.track_score_step(st, truths[f], [row[:5] for row in tracks[f]], 0.5)[0]
        states.append(st)
    assert sc.same_summary(got, ptq.track_score_summary(states))
    # a TrackScore carries the score across calls: two calls of two steps are the one of four
    tracker, score = images.Tracker(streams, min_hits=1), images.TrackScore(streams, 0.5)
    half = streams * 2
    images.evaluate_tracking(network, pictures[:half], truths[:half], tracker, 2, layout="time", score=score)
    assert sc.same_summary(images.evaluate_tracking(network, pictures[half:], truths[half:], tracker, 2, layout="time", score=score), got)
    with pytest.raises(ValueError, match="streams"):
        images.evaluate_tracking(network, pictures, truths, tracker, steps, score=images.TrackScore(streams + 1))
