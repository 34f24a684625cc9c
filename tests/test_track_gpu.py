"""The tracker on the MI355X (yf_images_track_device): the device against the host build of csrc/yf_images_track.h, exactly -- records,
infos, counts, status and the whole state buffer, every array between guard bytes and every place that must not be written a sentinel --
on the designed and the seeded random sequences of tests/track_support.py (once against the plain-Python statement too, so that this file
stands alone); 1, 3, 5 and 130 streams by 1 and 7 steps in both layouts; one call of many steps (the state in registers) against many
calls of one (the state reloaded); one stream's records changed, every other stream's bytes the same; an empty batch; the argument
checks; the tracker's output straight into the redaction; and `detect_tracked` end to end on a clip of the real images."""
import ctypes

import numpy as np
import pytest

import redact_support as rs
import track_support as ts
from images_support import Batch, images_after_network, last_error, ptq, real_images, to_host, torch_cuda      # noqa: F401 (fixtures; `images` is images_after_network)

pytestmark = pytest.mark.gpu


def device_run(torch, images, dets, counts, streams, steps, layout, cap, params, state0, out_cap, with_status=True):
    """the device entry on uploaded copies -> ts.Result, as `ts.host_run` gives it"""
    lib = images.load()

    def call(d, c, streams, steps, layout, cap, params, state, out, info, oc, out_cap, status):
        p = ts.Params(*params)
        rc = lib.yf_images_track_device(d, c, streams, steps, layout, cap, ctypes.byref(p), state, out, info, oc, out_cap, status, None)
        torch.cuda.synchronize()
        return rc
    return ts.run_with(call, dets, counts, streams, steps, layout, cap, params, state0, out_cap, with_status,
                       upload=lambda a: torch.from_numpy(a.copy()).cuda(), download=lambda b: b.cpu().numpy())


def test_device_equals_the_host_build_on_the_designed_sequences(torch_cuda, images):
    for case in ts.designed():
        for layout in ts.LAYOUTS:
            dets, counts, streams, steps, state0 = ts.laid_out(case, layout)
            want = ts.host_run(dets, counts, streams, steps, layout, case.cap, case.params, state0, case.out_cap)
            got = device_run(torch_cuda, images, dets, counts, streams, steps, layout, case.cap, case.params, state0, case.out_cap)
            assert want.rc == streams * steps and ts.same(got, want), (case.name, layout)
        # ... and the host build is the statement (tests/test_track_host.py); here too, so that this file stands alone
        assert ts.same(got, ts.expected(dets, counts, streams, steps, layout, case.cap, case.params, state0, case.out_cap)), case.name
        bare = device_run(torch_cuda, images, dets, counts, streams, steps, layout, case.cap, case.params, state0, case.out_cap, with_status=False)
        assert (bare.status == ts.SENTINEL32).all() and ts.same(bare._replace(status=want.status), want), case.name


def test_device_equals_the_host_build_on_the_random_sequences(torch_cuda, images):
    for layout in ts.LAYOUTS:
        dets, counts, want = ts.random_call(layout)
        got = device_run(torch_cuda, images, dets, counts, ts.R_STREAMS, ts.R_STEPS, layout, ts.R_CAP, ts.R_PARAMS, ts.empty_state(ts.R_STREAMS),
                         ts.R_OUT_CAP)
        assert ts.same(got, want), layout                                      # the statement's expectation
        assert ts.same(got, ts.host_run(dets, counts, ts.R_STREAMS, ts.R_STEPS, layout, ts.R_CAP, ts.R_PARAMS, ts.empty_state(ts.R_STREAMS),
                                        ts.R_OUT_CAP)), layout


@pytest.mark.parametrize("streams", [1, 3, 5, 130])
def test_streams_by_steps_in_both_layouts(torch_cuda, images, streams):
    cap, out_cap, params = 6, 5, (0.3, 2, 1)
    for steps in (1, 7):
        frames = ts.drift_frames(streams, steps)
        results = {}
        for layout in ts.LAYOUTS:
            dets, counts = ts.lay_out(frames, cap, layout)
            want = ts.host_run(dets, counts, streams, steps, layout, cap, params, ts.empty_state(streams), out_cap)
            got = device_run(torch_cuda, images, dets, counts, streams, steps, layout, cap, params, ts.empty_state(streams), out_cap)
            assert got.rc == streams * steps and ts.same(got, want), (streams, steps, layout)
            results[layout] = got
        assert ts.by_frame(results[ts.TIME], streams, steps, ts.TIME) == ts.by_frame(results[ts.STREAM], streams, steps, ts.STREAM)
    assert (results[ts.TIME].out_counts > 0).any() and results[ts.TIME].state["issued"].all()       # at 7 steps every stream has had tracks


def test_a_workgroup_that_takes_a_second_stream(torch_cuda, images):
    """more streams than the launch has workgroups (the device's CUs times the launcher's own number per CU): the device against the
    host build in every byte, from the empty state and from the state that call left"""
    grid = torch_cuda.cuda.get_device_properties(0).multi_processor_count * ts.per_cu("Track")
    ts.beyond_the_grid(lambda *a: device_run(torch_cuda, images, *a), ts.host_run, grid, (0.3, 2, 1), ts.empty_state)


def test_one_call_of_many_steps_equals_many_calls_of_one(torch_cuda, images):
    dets, counts, want = ts.random_call(ts.TIME)
    run = lambda *a: device_run(torch_cuda, images, *a)
    got = ts.split_calls(run, dets, counts, ts.R_STREAMS, ts.R_STEPS, ts.R_CAP, ts.R_PARAMS, ts.empty_state(ts.R_STREAMS), ts.R_OUT_CAP)
    assert ts.same(got, want)


def test_one_streams_records_change_no_other_streams_bytes(torch_cuda, images):
    streams, steps, cap, out_cap, params = 5, 7, 6, 5, (0.3, 1, 2)
    frames = ts.drift_frames(streams, steps)
    other = [list(clip) for clip in frames]
    other[2] = [([(7, 7, 30 + t, 30), (200, 100, 240, 150 - t)], None) for t in range(steps)]
    for layout in ts.LAYOUTS:
        a = device_run(torch_cuda, images, *ts.lay_out(frames, cap, layout), streams, steps, layout, cap, params, ts.empty_state(streams), out_cap)
        b = device_run(torch_cuda, images, *ts.lay_out(other, cap, layout), streams, steps, layout, cap, params, ts.empty_state(streams), out_cap)
        for s in range(streams):
            rows = [ts.frame_of(s, t, streams, steps, layout) for t in range(steps)]
            equal = all(x[rows].tobytes() == y[rows].tobytes() for x, y in zip(a[2:], b[2:])) and a.state[s].tobytes() == b.state[s].tobytes()
            assert equal == (s != 2), (layout, s)


def test_an_empty_batch_and_the_argument_checks(torch_cuda, images):
    torch = torch_cuda
    lib = images.load()
    case = ts.designed()[0]
    dets, counts, streams, steps, state0 = ts.laid_out(case, ts.TIME)
    # every fault is refused before anything is launched: the addresses of these calls are made up and never used
    names = ("dets", "counts", "streams", "steps", "layout", "cap", "params", "state", "out", "info", "out_counts", "out_cap", "status")
    valid = dict(dets=8, counts=8, streams=2, steps=3, layout=ts.TIME, cap=8, params=ts.DEFAULT, state=8, out=8, info=8, out_counts=8, out_cap=4,
                 status=0)
    for kw, text in ts.FAULTS:
        a = dict(valid, **kw)
        p = None if a["params"] is None else ctypes.byref(ts.Params(*a["params"]))
        rc = lib.yf_images_track_device(*(p if k == "params" else (a[k] or None) if k in ("dets", "counts", "state", "out", "info", "out_counts", "status")
                                          else a[k] for k in names), None)
        assert rc == -1 and text in last_error(lib), (kw, rc, last_error(lib))
    # a refused call with real arrays writes nothing; neither does an empty batch, which is taken after the checks
    for params, cap, out_cap in (((float("nan"), 1, 1), case.cap, 4), ((0.3, 0, 1), case.cap, 4), ((0.3, 1, 1), 0, 4), ((0.3, 1, 1), 1201, 4)):
        r = device_run(torch, images, dets, counts, streams, steps, ts.TIME, cap, params, state0, out_cap)
        assert r.rc == -1 and r.state.tobytes() == state0.tobytes() and (r.out_counts == ts.SENTINEL32).all(), (params, cap)
    for streams0, steps0 in ((0, 5), (1, 0), (0, 0)):
        r = device_run(torch, images, dets, counts, streams0, steps0, ts.TIME, case.cap, case.params, state0, 4)
        assert r.rc == 0 and r.state.tobytes() == state0.tobytes() and (r.out_counts == ts.SENTINEL32).all()
        assert (r.out.view(np.uint8) == 0xA5).all() and (r.status == ts.SENTINEL32).all()
    assert images.track_state_bytes(3) == 3 * 2824 and images.track_state_bytes(0) == 0 and images.track_state_bytes(-2) == 0
    with pytest.raises(images.ImagesError, match="min_hits"):
        images.track_device(8, 8, 1, 1, "time", 4, (0.3, 0, 1), 8, 8, 8, 8, 4)
    with pytest.raises(ValueError, match="layout"):
        images.track_device(8, 8, 1, 1, "rows", 4, (0.3, 1, 1), 8, 8, 8, 8, 4)


def test_tracked_records_go_straight_into_the_redaction(torch_cuda, images, ptq):
    """a clip of three frames whose middle frame has no detection: the tracker holds the face over, and the redaction, which takes the
    tracker's output as its records, hides it there too"""
    torch = torch_cuda
    fmt, cap, out_cap, params = 0, 4, 8, (0.3, 1, 2)
    frames = [[([(10, 8, 33, 30), (40, 20, 55, 41)], None), ([], None), ([(12, 9, 35, 31)], None)]]
    dets, counts = ts.lay_out(frames, cap, ts.TIME)
    want = ts.expected(dets, counts, 1, 3, ts.TIME, cap, params, ts.empty_state(1), out_cap)
    assert want.out_counts.tolist() == [2, 2, 2] and want.info[1]["misses"][:2].tolist() == [1, 1]
    pictures = [rs.cs.in_format(rs.picture(f), fmt) for f in (1, 4, 6)]          # three 64 x 48 pictures
    buf, desc = rs.lay_out_packed(pictures)
    tracker = images.Tracker(1, *params)
    d_dets = torch.from_numpy(dets.view(np.uint8).reshape(3, cap, 28).copy()).cuda()
    d_counts = torch.from_numpy(counts.copy()).cuda()
    d_out, d_info, d_oc, d_status = tracker.update(d_dets, d_counts, 3, "time", out_cap=out_cap)
    d_px = torch.from_numpy(buf.copy()).cuda()
    d_desc = torch.from_numpy(desc.view(np.uint8).copy()).cuda()
    d_first = torch.empty(4, dtype=torch.int32, device="cuda")
    d_rstatus = torch.empty(3, dtype=torch.int32, device="cuda")
    images.redact_records_device(d_px.data_ptr(), buf.nbytes, fmt, d_desc.data_ptr(), d_out.data_ptr(), d_oc.data_ptr(), 3, out_cap,
                                 d_first.data_ptr(), d_rstatus.data_ptr(), mode="mosaic", block=8)
    torch.cuda.synchronize()
    assert d_oc.cpu().numpy().tolist() == [2, 2, 2] and not d_status.cpu().numpy().any() and not d_rstatus.cpu().numpy().any()
    assert d_out.cpu().numpy().tobytes()[:2 * 28] == want.out[0, :2].tobytes()
    redacted = []
    for f, p in enumerate(pictures):
        regions = [ptq.crop_region((int(d["x1"]), int(d["y1"]), int(d["x2"]), int(d["y2"])), 64, 48) for d in want.out[f, :want.out_counts[f]]]
        redacted.append(ptq.redact_u8(p, regions, "mosaic", 8, None))
    got = d_px.cpu().numpy()
    assert np.array_equal(got, rs.lay_out_packed(redacted)[0])
    assert not np.array_equal(redacted[1], pictures[1])                        # the middle frame is redacted although it has no detection
    # the tracker object carried the state: a reset empties it
    assert int(tracker.d_state.cpu().numpy().view(ts.STATE).reshape(-1)[0]["issued"]) == 2
    tracker.reset()
    assert not tracker.d_state.cpu().numpy().any()


def test_detect_tracked_on_a_clip_of_the_real_images(network, torch_cuda, images, ptq, yf):
    """three streams of four frames from the real images: stream s shows image s, then image s again, then a blank picture (the face is
    held over), then image s + 3; against `ptq.track_step` over the records of the same frames"""
    torch = torch_cuda
    real = real_images(ptq)
    streams, steps = 3, 4
    blank = np.full((64, 64, 3), 128, np.uint8)
    clip = {(s, t): (real[s], real[s], blank, real[s + 3])[t] for s in range(streams) for t in range(steps)}
    for layout, code in (("time", ts.TIME), ("stream", ts.STREAM)):
        order = sorted(clip, key=lambda st: ts.frame_of(st[0], st[1], streams, steps, code))
        pictures = [clip[st] for st in order]
        boxes = images.detect(network, pictures, iou_threshold=0.4)
        assert sum(b.shape[0] for b in boxes) >= 3 and all(boxes[order.index((s, 2))].shape[0] == 0 for s in range(streams))
        # the same frames' records with their confidences: the ragged run and the suppression, as `detect` launches them
        b = Batch(torch, images, pictures, 0)
        b.run_decode(images, network)
        images.nms_device(b.d_dets.data_ptr(), b.d_counts.data_ptr(), b.n, b.cap, 0.4)
        dets, counts = to_host(yf, b.d_dets, b.d_counts, b.cap)
        for f in range(b.n):
            d = dets[f, :counts[f]]
            assert np.array_equal(np.stack([d["x1"], d["y1"], d["x2"], d["y2"]], axis=1).reshape(-1, 4), boxes[f]), f
        tracker = images.Tracker(streams)
        states = [ptq.track_empty_state() for _ in range(streams)]
        held = 0
        for call in range(2):                                                  # the second call carries on where the first ended
            got = images.detect_tracked(network, pictures, tracker, steps, layout=layout)
            for s in range(streams):
                for t in range(steps):
                    f = ts.frame_of(s, t, streams, steps, code)
                    states[s], emitted, status = ptq.track_step(states[s], dets[f, :counts[f]].tolist(), tracker.params, frame=f)
                    want = [(i, r[6], r[7], r[8], r[9], r[5], hits, misses) for r, (i, hits, misses, _) in emitted]
                    assert status == 0 and got[f] == want, (layout, call, s, t, got[f], want)
                    held += sum(w[7] > 0 for w in want)
        assert held >= 6, layout
    assert images.detect_tracked(network, [], images.Tracker(2), 0) == []
    with pytest.raises(ValueError, match="streams"):
        images.detect_tracked(network, real[:5], images.Tracker(2), 2)
