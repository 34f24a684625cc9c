"""The tracker with a motion model on the MI355X (yf_images_track_motion_device): the device against the host build of
csrc/yf_images_motion.h, exactly -- records, infos, counts, status and the whole state buffer, every array between guard bytes and every
place that must not be written a sentinel -- on the scenario of a moving box whose detections have a gap, the designed sequences of
tests/track_support.py, the seeded random sequences of tests/motion_support.py and a state of random bytes (once against the plain-Python
statement too, so that this file stands alone); 1, 3, 5 and 130 streams by 1 and 7 steps in both layouts; a full table in which every
lane takes part in the match, the births and the output; one call of many steps (the state in registers) against many calls of one (the
state reloaded); one stream's records changed, every other stream's bytes the same; the base device entry's bytes at (256, 0); an empty
batch; the argument checks; a `Tracker(motion=...)`'s output straight into the redaction; and `detect_redacted` / `detect_blurred` with a
tracker on a clip of the real images."""
import ctypes

import numpy as np
import pytest

import motion_support as ms
import redact_support as rs
import track_support as ts
from images_support import Batch, images_after_network, last_error, ptq, real_images, to_host, torch_cuda      # noqa: F401 (fixtures; `images` is images_after_network)

pytestmark = pytest.mark.gpu


def device_run(torch, images, dets, counts, streams, steps, layout, cap, params, state0, out_cap, with_status=True):
    """the device entry on uploaded copies -> ts.Result, as `ms.host_run` gives it"""
    lib = images.load()

    def call(d, c, streams, steps, layout, cap, params, state, out, info, oc, out_cap, status):
        p = ms.c_params(params)
        rc = lib.yf_images_track_motion_device(d, c, streams, steps, layout, cap, ctypes.byref(p), state, out, info, oc, out_cap, status, None)
        torch.cuda.synchronize()
        return rc
    return ts.run_with(call, dets, counts, streams, steps, layout, cap, params, state0, out_cap, with_status,
                       upload=lambda a: torch.from_numpy(a.copy()).cuda(), download=lambda b: b.cpu().numpy())


def base_device_run(torch, images, dets, counts, streams, steps, layout, cap, params, state0, out_cap):
    lib = images.load()

    def call(d, c, streams, steps, layout, cap, params, state, out, info, oc, out_cap, status):
        p = ts.Params(*params)
        rc = lib.yf_images_track_device(d, c, streams, steps, layout, cap, ctypes.byref(p), state, out, info, oc, out_cap, status, None)
        torch.cuda.synchronize()
        return rc
    return ts.run_with(call, dets, counts, streams, steps, layout, cap, params, state0, out_cap,
                       upload=lambda a: torch.from_numpy(a.copy()).cuda(), download=lambda b: b.cpu().numpy())


def same_as_host(torch, images, dets, counts, streams, steps, layout, cap, params, state0, out_cap, what):
    want = ms.host_run(dets, counts, streams, steps, layout, cap, params, state0, out_cap)
    got = device_run(torch, images, dets, counts, streams, steps, layout, cap, params, state0, out_cap)
    assert want.rc == streams * steps and ts.same(got, want), what
    return got


def test_device_equals_the_host_build_on_the_scenario(torch_cuda, images):
    for gains in ms.GAIN_SETS:
        for smooth in (0, 1):
            for layout in ts.LAYOUTS:
                dets, counts = ts.lay_out(ms.scenario(), ms.S_CAP, layout)
                params = ms.S_BASE + gains + (smooth,)
                got = same_as_host(torch_cuda, images, dets, counts, 1, ms.S_STEPS, layout, ms.S_CAP, params, ms.empty_state(1), 4, (gains, smooth, layout))
            # ... and the host build is the statement (tests/test_track_motion_host.py); here too, so that this file stands alone
            assert ts.same(got, ms.expected(dets, counts, 1, ms.S_STEPS, layout, ms.S_CAP, params, ms.empty_state(1), 4)), (gains, smooth)
            ids, held = ms.S_EXPECTED[gains]
            assert [ms.boxes_of(got, t) for t in ms.S_GAP] == [[(1, *held[k], k + 1)] for k in range(3)], gains
            assert [row[0] for row in ms.boxes_of(got, 9) if row[5] == 0] == [ids[9]], gains


def test_device_equals_the_host_build_on_the_designed_sequences(torch_cuda, images):
    for case in ts.designed():
        params = tuple(case.params) + ms.SUGGESTED + (len(case.name) % 2,)          # smooth 0 for some cases, 1 for the others
        for layout in ts.LAYOUTS:
            dets, counts, streams, steps, base0 = ts.laid_out(case, layout)
            state0 = ms.lift(base0)
            got = same_as_host(torch_cuda, images, dets, counts, streams, steps, layout, case.cap, params, state0, case.out_cap, (case.name, layout))
        bare = device_run(torch_cuda, images, dets, counts, streams, steps, layout, case.cap, params, state0, case.out_cap, with_status=False)
        assert (bare.status == ts.SENTINEL32).all() and ts.same(bare._replace(status=got.status), got), case.name


def test_device_equals_the_host_build_on_the_random_sequences_and_a_state_of_random_bytes(torch_cuda, images):
    for gains in ms.R_GAINS:
        for layout in ts.LAYOUTS:
            dets, counts, want = ms.random_call(layout, gains)                         # the statement's expectation
            got = same_as_host(torch_cuda, images, dets, counts, ms.R_STREAMS, ms.R_STEPS, layout, ms.R_CAP, ms.R_BASE + gains,
                               ms.empty_state(ms.R_STREAMS), ms.R_OUT_CAP, (gains, layout))
            assert ts.same(got, want), (gains, layout)
    # random bytes (the last stream's table full) and pos / vel at the int64 extremes, met by records at the boxes the slots predict
    junk = ms.junk_state(ms.R_STREAMS, full=(ms.R_STREAMS - 1,))
    frames = [list(clip) for clip in ms.random_frames()]
    for s in range(ms.R_STREAMS):
        frames[s][0] = ([ms.predicted_box(junk, s, k) for k in (3, 17, 40)] + frames[s][0][0][:3], None)
    for layout in ts.LAYOUTS:
        dets, counts = ts.lay_out(frames, ms.R_CAP, layout)
        same_as_host(torch_cuda, images, dets, counts, ms.R_STREAMS, ms.R_STEPS, layout, ms.R_CAP, ms.R_BASE + ms.SUGGESTED + (1,), junk, 64, layout)
        near = [(10, 10, 40, 40), (100, 100, 140, 140), (12, 9, 41, 42)]
        dets, counts = ts.lay_out([[(near, None), (near[::-1], None), ([], None), (near, None)]], 3, layout)
        same_as_host(torch_cuda, images, dets, counts, 1, 4, layout, 3, (0.1, 1, 3) + ms.DIFFERENCE + (1,), ms.extreme_state(), 64, layout)


@pytest.mark.parametrize("streams", [1, 3, 5, 130])
def test_streams_by_steps_in_both_layouts(torch_cuda, images, streams):
    cap, out_cap, params = 6, 5, (0.3, 2, 1) + ms.SUGGESTED + (0,)
    for steps in (1, 7):
        frames = ts.drift_frames(streams, steps)
        results = {}
        for layout in ts.LAYOUTS:
            dets, counts = ts.lay_out(frames, cap, layout)
            results[layout] = same_as_host(torch_cuda, images, dets, counts, streams, steps, layout, cap, params, ms.empty_state(streams), out_cap,
                                           (streams, steps, layout))
        assert ts.by_frame(results[ts.TIME], streams, steps, ts.TIME) == ts.by_frame(results[ts.STREAM], streams, steps, ts.STREAM)
    assert (results[ts.TIME].out_counts > 0).any() and results[ts.TIME].state["issued"].all()       # at 7 steps every stream has had tracks
    assert results[ts.TIME].state["slot"]["vel"].any()


def test_a_workgroup_that_takes_a_second_stream(torch_cuda, images):
    """more streams than the launch has workgroups (the device's CUs times the launcher's own number per CU): the device against the
    host build in every byte, from the empty state and from the state that call left"""
    grid = torch_cuda.cuda.get_device_properties(0).multi_processor_count * ts.per_cu("Motion")
    ts.beyond_the_grid(lambda *a: device_run(torch_cuda, images, *a), ms.host_run, grid, (0.3, 2, 1) + ms.SUGGESTED + (1,), ms.empty_state)


def full_table():
    """one stream, 64 occupied slots with a velocity each, 64 detections: 40 slots are seen again where they moved to, 24 are not -- 10
    of those at max_misses, which go --, and 24 new boxes find 10 free slots: 14 are dropped"""
    st = ms.empty_state(1)
    boxes = []
    for k in range(64):
        x, y = (k % 8) * 40, (k // 8) * 40
        vx, vy = (k % 5) - 2, (k % 3) - 1
        st["slot"]["base"][0, k] = (k + 1, 3, 2 if k >= 54 else 0, 5, (7, 1, 2, 3, 4, ts.conf_bits(k), x, y, x + 19, y + 24))
        st["slot"]["pos"][0, k] = (256 * x + 77, 256 * y - 77, 256 * (x + 19) + 128, 256 * (y + 24) - 128)
        st["slot"]["vel"][0, k] = (256 * vx, 256 * vy, 256 * vx + 60, 256 * vy - 60)
        if k < 40:
            boxes.append((x + vx + 1, y + vy, x + 20 + vx, y + 24 + vy))
    st["issued"] = 64
    boxes += [(1000 + 30 * k, 500, 1019 + 30 * k, 520) for k in range(24)]
    order = np.random.default_rng(6300).permutation(64)
    return st, [[([boxes[int(k)] for k in order], None), ([boxes[int(k)] for k in order[::-1]], None)]]


def test_a_full_table_matches_removes_bears_and_drops_in_one_step(torch_cuda, images):
    state0, frames = full_table()
    params = (0.3, 1, 2) + ms.SUGGESTED + (0,)
    stats = {}
    for layout in ts.LAYOUTS:
        dets, counts = ts.lay_out(frames, 64, layout)
        got = same_as_host(torch_cuda, images, dets, counts, 1, 2, layout, 64, params, state0, 64, layout)
    want = ms.expected(dets[:1], counts[:1], 1, 1, ts.TIME, 64, params, state0, 64, stats)
    assert stats == dict(matches=40, births=10, removals=10, held=14, ties=0, dropped=14) and want.status[0] == 2
    assert got.out_counts[0] == 64 and got.status[0] == 2 and got.out[0].tobytes() == want.out[0].tobytes()


def test_one_call_of_many_steps_equals_many_calls_of_one(torch_cuda, images):
    gains = ms.SUGGESTED + (0,)
    dets, counts, want = ms.random_call(ts.TIME, gains)
    run = lambda *a: device_run(torch_cuda, images, *a)
    got = ts.split_calls(run, dets, counts, ms.R_STREAMS, ms.R_STEPS, ms.R_CAP, ms.R_BASE + gains, ms.empty_state(ms.R_STREAMS), ms.R_OUT_CAP)
    assert ts.same(got, want)


def test_one_streams_records_change_no_other_streams_bytes(torch_cuda, images):
    streams, steps, cap, out_cap, params = 5, 7, 6, 5, (0.3, 1, 2) + ms.SUGGESTED + (1,)
    frames = ts.drift_frames(streams, steps)
    other = [list(clip) for clip in frames]
    other[2] = [([(7, 7, 30 + t, 30), (200, 100, 240, 150 - t)], None) for t in range(steps)]
    for layout in ts.LAYOUTS:
        a = device_run(torch_cuda, images, *ts.lay_out(frames, cap, layout), streams, steps, layout, cap, params, ms.empty_state(streams), out_cap)
        b = device_run(torch_cuda, images, *ts.lay_out(other, cap, layout), streams, steps, layout, cap, params, ms.empty_state(streams), out_cap)
        for s in range(streams):
            rows = [ts.frame_of(s, t, streams, steps, layout) for t in range(steps)]
            equal = all(x[rows].tobytes() == y[rows].tobytes() for x, y in zip(a[2:], b[2:])) and a.state[s].tobytes() == b.state[s].tobytes()
            assert equal == (s != 2), (layout, s)


def test_alpha_256_beta_0_is_the_base_device_entry(torch_cuda, images):
    for layout in ts.LAYOUTS:
        dets, counts = ts.lay_out(ms.random_frames(), ms.R_CAP, layout)
        base = base_device_run(torch_cuda, images, dets, counts, ms.R_STREAMS, ms.R_STEPS, layout, ms.R_CAP, ms.R_BASE, ts.empty_state(ms.R_STREAMS),
                               ms.R_OUT_CAP)
        got = device_run(torch_cuda, images, dets, counts, ms.R_STREAMS, ms.R_STEPS, layout, ms.R_CAP, ms.R_BASE + (256, 0, 256, 0),
                         ms.empty_state(ms.R_STREAMS), ms.R_OUT_CAP)
        assert got.rc == base.rc == ms.R_STREAMS * ms.R_STEPS and (base.out_counts > 0).any()
        assert all(getattr(got, name).tobytes() == getattr(base, name).tobytes() for name in ("out", "info", "out_counts", "status")), layout
        assert got.state["slot"]["base"].tobytes() == base.state["slot"].tobytes()


def test_an_empty_batch_and_the_argument_checks(torch_cuda, images):
    torch = torch_cuda
    lib = images.load()
    # every fault is refused before anything is launched: the addresses of these calls are made up and never used
    names = ("dets", "counts", "streams", "steps", "layout", "cap", "params", "state", "out", "info", "out_counts", "out_cap", "status")
    for kw, text in ms.FAULTS:
        a = dict(ms.VALID, **kw)
        p = None if a["params"] is None else ctypes.byref(ms.c_params(a["params"]))
        rc = lib.yf_images_track_motion_device(*(p if k == "params" else (a[k] or None) if k in ("dets", "counts", "state", "out", "info", "out_counts", "status")
                                                 else a[k] for k in names), None)
        assert rc == -1 and text in last_error(lib), (kw, rc, last_error(lib))
    # a refused call with real arrays writes nothing; neither does an empty batch, which is taken after the checks
    dets, counts = ts.lay_out(ms.scenario(), ms.S_CAP, ts.TIME)
    state0 = ms.junk_state(1)
    good = ms.S_BASE + ms.SUGGESTED + (0,)
    for params, cap in ((ms.S_BASE + (257, 0, 0, 0), ms.S_CAP), (ms.S_BASE + ms.SUGGESTED + (2,), ms.S_CAP), ((0.3, 0, 1) + ms.SUGGESTED + (0,), ms.S_CAP),
                        (good, 0), (good, 1201)):
        r = device_run(torch, images, dets, counts, 1, ms.S_STEPS, ts.TIME, cap, params, state0, 4)
        assert r.rc == -1 and r.state.tobytes() == state0.tobytes() and (r.out_counts == ts.SENTINEL32).all(), (params, cap)
    for streams0, steps0 in ((0, 5), (1, 0), (0, 0)):
        r = device_run(torch, images, dets, counts, streams0, steps0, ts.TIME, ms.S_CAP, good, state0, 4)
        assert r.rc == 0 and r.state.tobytes() == state0.tobytes() and (r.out_counts == ts.SENTINEL32).all()
        assert (r.out.view(np.uint8) == 0xA5).all() and (r.status == ts.SENTINEL32).all()
    assert images.track_motion_state_bytes(3) == 3 * 7176 == 3 * images.TRACK_MOTION_STATE_BYTES
    assert images.track_motion_state_bytes(0) == 0 and images.track_motion_state_bytes(-2) == 0
    with pytest.raises(images.ImagesError, match="beta"):
        images.track_motion_device(8, 8, 1, 1, "time", 4, (0.3, 1, 1, 256, 300, 0, 0), 8, 8, 8, 8, 4)
    with pytest.raises(ValueError, match="layout"):
        images.track_motion_device(8, 8, 1, 1, "rows", 4, (0.3, 1, 1, 256, 0, 0, 0), 8, 8, 8, 8, 4)
    with pytest.raises(ValueError, match="motion"):
        images.Tracker(1, motion=(256, 256, 300))
    assert images.Tracker(2).d_state.shape == (2, 2824) and images.Tracker(2, motion=True).d_state.shape == (2, 7176)
    assert images.Tracker(1, motion=True, smooth=True).motion == (192, 128, 256, 1)


def _regions(ptq, rows, w, h):
    return [ptq.crop_region(tuple(row[1:5]), w, h) for row in rows]


def test_a_motion_trackers_records_go_straight_into_the_redaction(torch_cuda, images, ptq):
    """the scenario through `Tracker.update` into `redact_records_device`: on the frames without a detection the region hidden is the
    predicted box, the true one at these gains -- not the place the face was last seen at, which the plain tracker hides"""
    torch = torch_cuda
    fmt, out_cap, n = 0, 8, ms.S_STEPS
    dets, counts = ts.lay_out(ms.scenario(), ms.S_CAP, ts.TIME)
    parent = rs.picture(3)                                                     # 410 x 362; a 160 x 120 window of it per step
    pictures = [rs.cs.in_format(parent[3 * t:3 * t + 120, 5 * t:5 * t + 160], fmt) for t in range(n)]
    buf, desc = rs.lay_out_packed(pictures)
    d_dets = torch.from_numpy(dets.view(np.uint8).reshape(n, ms.S_CAP, 28).copy()).cuda()
    d_counts = torch.from_numpy(counts.copy()).cuda()
    d_desc = torch.from_numpy(desc.view(np.uint8).copy()).cuda()
    hidden = {}
    for name, tracker in (("motion", images.Tracker(1, *ms.S_BASE, motion=ms.DIFFERENCE)), ("plain", images.Tracker(1, *ms.S_BASE))):
        d_out, d_info, d_oc, d_status = tracker.update(d_dets, d_counts, n, "time", out_cap=out_cap)
        d_px = torch.from_numpy(buf.copy()).cuda()
        d_first = torch.empty(n + 1, dtype=torch.int32, device="cuda")
        d_rstatus = torch.empty(n, dtype=torch.int32, device="cuda")
        images.redact_records_device(d_px.data_ptr(), buf.nbytes, fmt, d_desc.data_ptr(), d_out.data_ptr(), d_oc.data_ptr(), n, out_cap,
                                     d_first.data_ptr(), d_rstatus.data_ptr(), mode="mosaic", block=8)
        torch.cuda.synchronize()
        assert not d_status.cpu().numpy().any() and not d_rstatus.cpu().numpy().any()
        hidden[name] = (d_px.cpu().numpy(), images._track_tuples(d_out, d_info, d_oc, n))
    got, tracks = hidden["motion"]
    held = ms.S_EXPECTED[ms.DIFFERENCE][1]
    assert [tracks[t] for t in ms.S_GAP] == [[(1, *held[k], tracks[0][0][5], 6, k + 1)] for k in range(3)]
    redacted = [ptq.redact_u8(p, _regions(ptq, tracks[t], 160, 120), "mosaic", 8, None) for t, p in enumerate(pictures)]
    assert np.array_equal(got, rs.lay_out_packed(redacted)[0])
    for k, t in enumerate(ms.S_GAP):                                           # the bytes of the table's boxes, and not the plain tracker's
        assert np.array_equal(redacted[t], ptq.redact_u8(pictures[t], [ptq.crop_region(held[k], 160, 120)], "mosaic", 8, None))
        assert not np.array_equal(redacted[t], pictures[t])
    plain, plain_tracks = hidden["plain"]
    assert [row[1:5] for t in ms.S_GAP for row in plain_tracks[t]] == [(70, 40, 109, 89)] * 3 and not np.array_equal(plain, got)
    assert int(tracker.d_state.cpu().numpy().view(ts.STATE).reshape(-1)[0]["issued"]) == 2


def test_detect_redacted_and_detect_blurred_with_a_tracker_on_a_clip_of_the_real_images(network, torch_cuda, images, ptq, yf):
    """three streams of four frames from the real images: stream s shows image s, then image s again, then a picture of its size without
    a face (grey with a fine texture of +-1, so that a mosaic or a blur of any region of it changes bytes: the face is held over and
    hidden there too), then image s + 3; against `ptq.track_motion_step` over the records of the same frames, then
    `ptq.redact_u8` / `ptq.blur_u8` over the reported tracks"""
    torch = torch_cuda
    real = real_images(ptq)
    streams, steps = 3, 4
    def blank(like):
        y, x = np.mgrid[:like.shape[0], :like.shape[1]]
        return np.repeat((127 + 2 * ((x + y) % 8 < 4)).astype(np.uint8)[..., None], 3, axis=2)
    clip = {(s, t): (real[s], real[s], blank(real[s]), real[s + 3])[t] for s in range(streams) for t in range(steps)}
    for layout, code in (("time", ts.TIME), ("stream", ts.STREAM)):
        order = sorted(clip, key=lambda st: ts.frame_of(st[0], st[1], streams, steps, code))
        pictures = [clip[st] for st in order]
        b = Batch(torch, images, pictures, 0)
        b.run_decode(images, network)
        images.nms_device(b.d_dets.data_ptr(), b.d_counts.data_ptr(), b.n, b.cap, 0.4)
        dets, counts = to_host(yf, b.d_dets, b.d_counts, b.cap)
        params = (0.3, 1, 5) + ms.SUGGESTED + (0,)
        want = [None] * b.n
        for s in range(streams):
            state = ptq.track_motion_empty_state()
            for t in range(steps):
                f = ts.frame_of(s, t, streams, steps, code)
                state, emitted, status = ptq.track_motion_step(state, dets[f, :counts[f]].tolist(), params, frame=f)
                want[f] = [(i, r[6], r[7], r[8], r[9], r[5], hits, misses) for r, (i, hits, misses, _) in emitted]
                assert status == 0
        blanks = [order.index((s, 2)) for s in range(streams)]
        assert all(counts[f] == 0 for f in blanks) and sum(len(want[f]) for f in blanks) >= 3 and all(w[7] == 1 for f in blanks for w in want[f])
        for call, restated in ((lambda **kw: images.detect_redacted(network, pictures, **kw), lambda p, reg: ptq.redact_u8(p, reg, "mosaic", 8, None)),
                               (lambda **kw: images.detect_blurred(network, pictures, **kw), lambda p, reg: ptq.blur_u8(p, reg, 8))):
            got, tracks = call(tracker=images.Tracker(streams, motion=True), layout=layout)
            assert tracks == want, layout
            for f, p in enumerate(pictures):
                assert np.array_equal(got[f], restated(p, _regions(ptq, want[f], p.shape[1], p.shape[0]))), (layout, f)
            assert all(want[f] and not np.array_equal(got[f], pictures[f]) for f in blanks)       # the frame without a face is hidden too
            # without a tracker the call is what it was: `detect`'s boxes, and the blank frame untouched
            plain, boxes = call()
            for f, p in enumerate(pictures):
                d = dets[f, :counts[f]]
                assert np.array_equal(boxes[f], np.stack([d["x1"], d["y1"], d["x2"], d["y2"]], axis=1).reshape(-1, 4)), f
                assert np.array_equal(plain[f], restated(p, [ptq.crop_region(tuple(int(v) for v in box), p.shape[1], p.shape[0]) for box in boxes[f]]))
            assert all(np.array_equal(plain[f], pictures[f]) for f in blanks)
    with pytest.raises(ValueError, match="streams"):
        images.detect_redacted(network, real[:5], tracker=images.Tracker(2, motion=True), steps=2)
    with pytest.raises(ValueError, match="suppressed"):
        images.detect_blurred(network, real[:4], tracker=images.Tracker(2, motion=True), iou_threshold=None)
