"""The appearance descriptors and the re-identification on the MI355X (yf_images_describe_records_device, _yuv_device,
yf_images_reid_device): the device against the host build of csrc/yf_images_describe.h and csrc/yf_images_reid.h, exactly -- every array
between guard bytes and every place that must not be written a sentinel -- on the designed cases (once against the plain-Python
statements too, so that this file stands alone); batches with 0, 1 and cap records per frame over pictures of 8 x 8 up to 97 x 61; 1, 3
and 130 streams by 1 and 7 steps in both layouts; one call of 40 steps against 40 calls of one; more streams than the launch has
workgroups; empty batches and the argument checks; `ReId` behind a `Tracker` on the device against the host chain; the behavioural test
on textured clips; and `detect_tracked(..., reid=...)` on a still video of the real images."""
import numpy as np
import pytest

import reid_support as rs
import score_support as sc
import track_support as ts
from images_support import images_after_network, last_error, ptq, real_images, torch_cuda      # noqa: F401 (fixtures; `images` is images_after_network)

pytestmark = pytest.mark.gpu


def _ways(torch):
    return dict(upload=lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).cuda(), download=lambda b: b.cpu().numpy())


def device_describe(torch, images, batch, n=None):
    lib = images.load()
    name = "yf_images_describe_records_yuv_device" if batch.fmt in ("nv12", "nv21") else "yf_images_describe_records_device"

    def fn(*a):
        rc = getattr(lib, name)(*a, None)
        torch.cuda.synchronize()
        return rc
    return rs.describe_run_with(fn, batch, n=n, **_ways(torch))


def device_run(torch, images, call, streams, steps, layout, out_cap, params, state0, with_what=True, with_status=True, in_place=False):
    """the device entry on uploaded copies -> rs.Result, as `rs.host_run` gives it"""
    lib = images.load()

    def fn(*a):
        rc = lib.yf_images_reid_device(*a, None)
        torch.cuda.synchronize()
        return rc
    return rs.run_with(fn, call, streams, steps, layout, out_cap, params, state0, with_what, with_status, in_place, **_ways(torch))


def same_as_host(torch, images, call, streams, steps, layout, out_cap, params, state0, what, **kw):
    want = rs.host_run(call, streams, steps, layout, out_cap, params, state0, **kw)
    got = device_run(torch, images, call, streams, steps, layout, out_cap, params, state0, **kw)
    assert want.rc == streams * steps and rs.same(got, want), what
    return got


def test_the_device_descriptors_equal_the_host_build_and_the_statement(torch_cuda, images):
    for batch in rs.describe_batches() + rs.gpu_describe_batches():
        want = rs.describe_host_run(batch)
        got = device_describe(torch_cuda, images, batch)
        assert got.rc == len(batch.pictures) and rs.same_desc(got, want), batch.name
        if batch.name in ("sizes_bgra", "sizes_nv21", "counts", "ragged_nv12"):             # ... here too, so that this file stands alone
            assert rs.same_desc(got, rs.describe_expected(batch)), batch.name
    # (the last batch is the NV12 one: its odd-sided surface is refused, the even-sided one described)
    assert got.status.tolist() == [0, 0, 1, 0, 0] and not got.desc["flags"][2].any() and (got.desc["flags"][4] == 1).any()
    assert (got.desc["flags"][0] == 0xA5A5A5A5).all()


def test_the_describe_argument_checks_and_an_empty_batch(torch_cuda, images):
    lib = images.load()
    # every fault is refused before anything is launched: the addresses of these calls are made up and never used
    for kw, text in rs.D_FAULTS:
        a = dict(rs.D_VALID, **kw)
        args = [a["pixels"] or None, 64, 0, a["images"] or None, a["dets"] or None, a["counts"] or None, a["n"], a["cap"], a["margin"], a["flags"],
                a["desc"] or None, a["first"] or None, a["status"] or None, None]
        assert lib.yf_images_describe_records_device(*args) == 0 and text in last_error(lib), (kw, last_error(lib))
    assert lib.yf_images_describe_records_device(8, 64, 4, 8, 8, 8, 2, 4, 0, 0, 8, 8, 8, None) == 0 and "yuv_device" in last_error(lib)
    assert lib.yf_images_describe_records_yuv_device(8, 64, 1, 8, 8, 8, 2, 4, 0, 0, 8, 8, 8, None) == 0 and "describe_records_device" in last_error(lib)
    assert lib.yf_images_describe_records_device(8, 64, 9, 8, 8, 8, 2, 4, 0, 0, 8, 8, 8, None) == 0 and "format must be" in last_error(lib)
    batch = rs.describe_batches()[0]
    for n, cap_fault in ((0, False), (None, True)):
        def fn(*a):
            name = "yf_images_describe_records_device"
            rc = getattr(lib, name)(*(a[:7] + ((0,) if cap_fault else (a[7],)) + a[8:]), None)
            torch_cuda.cuda.synchronize()
            return rc
        r = rs.describe_run_with(fn, batch, n=n, **_ways(torch_cuda))
        assert r.rc == 0 and (r.desc["flags"] == 0xA5A5A5A5).all() and (r.first == ts.SENTINEL32).all() and (r.status == ts.SENTINEL32).all()
    with pytest.raises(ValueError):
        images.describe_records_device(8, 64, "nv12", 8, 8, 8, 1, 4, 8, 8, 8)


def test_device_reid_equals_the_host_build_and_the_statement_on_the_designed_scenes(torch_cuda, images):
    for case in rs.designed():
        for layout in ts.LAYOUTS:
            call, streams, steps, state0 = rs.laid_out(case, layout)
            got = same_as_host(torch_cuda, images, call, streams, steps, layout, case.out_cap, case.params, state0, (case.name, layout))
            # ... and the host build is the statement (tests/test_reid_host.py); here too, so that this file stands alone
            assert rs.same(got, rs.expected(call, streams, steps, layout, case.out_cap, case.params, state0)), (case.name, layout)
        same_as_host(torch_cuda, images, call, streams, steps, layout, case.out_cap, case.params, state0, (case.name, "in place"), in_place=True)
        if case.name == "lost_and_found":
            assert got.info["id"][4].tolist() == [7, 11] and got.what[4].tolist() == [rs.REIDENTIFIED, rs.BORN]
        if case.name == "evict":
            assert [int(got.state["entry"][0]["id"][k]) for k in (6, 13, 20, 27, 34)] == [900, 901, 902, 903, 904]


@pytest.mark.parametrize("streams", [1, 3, 130])
def test_streams_by_steps_in_both_layouts(torch_cuda, images, streams):
    for steps in (1, 7):
        frames = rs.drift_frames(streams, steps)
        results = {}
        for layout in ts.LAYOUTS:
            call = rs.lay_out(frames, rs.D_CAP, layout)
            results[layout] = same_as_host(torch_cuda, images, call, streams, steps, layout, rs.D_CAP, rs.D_PARAMS, rs.junk_state(streams),
                                           (streams, steps, layout))
        assert results[ts.TIME].state.tobytes() == results[ts.STREAM].state.tobytes()


def test_one_call_of_many_steps_equals_many_calls_of_one_with_and_without_the_optional_outputs(torch_cuda, images):
    streams, steps = 3, 40
    call = rs.lay_out(rs.drift_frames(streams, steps), rs.D_CAP, ts.TIME)
    want = rs.host_run(call, streams, steps, ts.TIME, rs.D_CAP, rs.D_PARAMS, rs.empty_state(streams))
    run = lambda part, streams, steps, layout, out_cap, params, state0: device_run(torch_cuda, images, part, streams, steps, layout, out_cap, params, state0)
    got = rs.split_calls(run, call, streams, steps, rs.D_CAP, rs.D_PARAMS, rs.empty_state(streams))
    assert rs.same(got, want)
    kinds = want.what[want.what != ts.SENTINEL32]
    assert all((kinds == k).any() for k in (0, rs.KNOWN, rs.REIDENTIFIED, rs.BORN))
    bare = device_run(torch_cuda, images, call, streams, steps, ts.TIME, rs.D_CAP, rs.D_PARAMS, rs.empty_state(streams), with_what=False, with_status=False)
    assert (bare.what == ts.SENTINEL32).all() and (bare.status == ts.SENTINEL32).all()
    assert bare.state.tobytes() == want.state.tobytes() and bare.info.tobytes() == want.info.tobytes()


def test_a_workgroup_that_takes_a_second_stream(torch_cuda, images):
    """three streams more than the launch has workgroups (the device's CUs times the launcher's own number per CU): a workgroup's entries
    are reloaded for its second stream and the table of distances in LDS is reused without a barrier; two steps, then the same again in
    the other layout on the state the first call left"""
    streams, steps = torch_cuda.cuda.get_device_properties(0).multi_processor_count * rs.per_cu() + 3, 2
    frames = rs.drift_frames(streams, steps)
    state = rs.empty_state(streams)
    for layout in ts.LAYOUTS:
        got = same_as_host(torch_cuda, images, rs.lay_out(frames, rs.D_CAP, layout), streams, steps, layout, rs.D_CAP, rs.D_PARAMS, state, layout)
        state = got.state
    assert (got.state["clock"] == 4).all() and (got.state["entry"]["id"][:, 0] != 0).mean() > 0.9


def test_an_empty_batch_and_the_argument_checks(torch_cuda, images):
    lib = images.load()
    # every fault is refused before anything is launched: the addresses of these calls are made up and never used
    for kw, text in rs.FAULTS:
        rc = lib.yf_images_reid_device(*rs.call_args(dict(rs.VALID, **kw)), None)
        assert rc == -1 and text in last_error(lib), (kw, rc, last_error(lib))
    case = rs.designed()[0]
    call, streams, steps, state0 = rs.laid_out(case, ts.TIME)
    state0 = rs.junk_state(1)
    for params, out_cap, layout in (((-1, 5, 5), 2, ts.TIME), ((5, 5, 300), 2, ts.TIME), ((5, 5, 5), 0, ts.TIME), ((5, 5, 5), 2, 2)):
        def fn(*a):
            return lib.yf_images_reid_device(*(a[:3] + (out_cap,) + a[4:6] + (layout,) + a[7:]), None)
        r = rs.run_with(fn, call, 1, steps, ts.TIME, case.out_cap, params, state0, **_ways(torch_cuda))
        assert r.rc == -1 and r.state.tobytes() == state0.tobytes() and (r.what == ts.SENTINEL32).all() and (r.status == ts.SENTINEL32).all()
        assert (r.info["id"] == 0xA5A5A5A5).all()
    for streams0, steps0 in ((0, 5), (1, 0), (0, 0)):
        r = device_run(torch_cuda, images, call, streams0, steps0, ts.TIME, case.out_cap, case.params, state0)
        assert r.rc == 0 and r.state.tobytes() == state0.tobytes() and (r.what == ts.SENTINEL32).all() and (r.status == ts.SENTINEL32).all()
    assert images.reid_state_bytes(3) == 3 * 5128 and images.reid_state_bytes(0) == 0
    with pytest.raises(images.ImagesError, match="blend"):
        images.reid_device(8, 8, 8, 4, 1, 1, "time", (5, 5, 300), 8, 8)
    with pytest.raises(ValueError, match="layout"):
        images.reid_device(8, 8, 8, 4, 1, 1, "rows", (5, 5, 5), 8, 8)
    with pytest.raises(ValueError):
        images.ReId(2, blend=300)


def _clip_on_device(torch, images, pictures, boxes, truths, reid_params):
    """one textured clip through `Tracker`, `ReId` (reid_params None: left out) and `TrackScore` on the device, the boxes fed to the
    tracker directly -> (summary, ids per step, reid states or None)"""
    steps, cap, out_cap = len(pictures), 4, 8
    dets, counts = ts.lay_out([[(b, None) for b in boxes]], cap, ts.TIME)
    d_dets = torch.from_numpy(dets.view(np.uint8).reshape(steps, cap, 28).copy()).cuda()
    d_counts = torch.from_numpy(counts.copy()).cuda()
    buf, descs, _, _ = rs.pack(rs.Batch("clip", "bgr", pictures, [[] for _ in pictures], None, out_cap))
    d_px, d_pictures = torch.from_numpy(buf.copy()).cuda(), torch.from_numpy(descs.view(np.uint8).reshape(steps, -1).copy()).cuda()
    gt, gt_counts = sc.truth_arrays([truths], 4, ts.TIME)
    d_gt = torch.from_numpy(gt.view(np.uint8).reshape(steps, 4, 20).copy()).cuda()
    d_gt_counts = torch.from_numpy(gt_counts.copy()).cuda()
    tracker, score = images.Tracker(1, *rs.CLIP_TRACKER), images.TrackScore(1, 0.5)
    reid = None if reid_params is None else images.ReId(1, *reid_params)
    ids = []
    for lo, hi in ((0, 11), (11, steps)):                        # the clip in two calls: the three states carry on
        d_out, d_info, d_out_counts, _ = tracker.update(d_dets[lo:hi], d_counts[lo:hi], hi - lo, "time", out_cap=out_cap)
        if reid is not None:
            # the whole buffer with the descriptors of the call's pictures: their offsets count from the buffer's first byte
            reid.update(d_px, buf.size, "bgr", d_pictures[lo:hi], d_out, d_info, d_out_counts, hi - lo, "time")
        score.update(d_out, d_info, d_out_counts, d_gt[lo:hi], d_gt_counts[lo:hi], hi - lo, "time")
        info, oc = d_info.cpu().numpy().view(ts.INFO).reshape(hi - lo, out_cap), d_out_counts.cpu().numpy()
        ids += [[int(info[t, k]["id"]) for k in range(int(oc[t]))] for t in range(hi - lo)]
    return score.summary(), ids, None if reid is None else reid.states()


def test_a_face_hidden_for_longer_than_max_misses_keeps_its_id_and_a_different_face_does_not_take_it(torch_cuda, images):
    """two textured faces, one of them hidden for 12 steps with max_misses = 5: without reid a switch and two ids for that face, with reid
    none and one; a DIFFERENT face after the gap is not re-identified.  The device chain equals the host chain, which gives these results
    alone (tests/test_reid_host.py)."""
    params = (rs.CLIP_MAX_DISTANCE, 60, 64)
    pictures, boxes, truths = rs.textured_clip("occlusion")
    plain, ids, _ = _clip_on_device(torch_cuda, images, pictures, boxes, truths, None)
    assert plain["switches"] >= 1 and len({i[1] for i in ids if len(i) > 1}) == 2
    fixed, ids, states = _clip_on_device(torch_cuda, images, pictures, boxes, truths, params)
    assert fixed["switches"] == 0 and len({i[1] for i in ids if len(i) > 1}) == 1
    want, want_ids, want_state, _ = rs.host_chain(pictures, boxes, truths, params)
    assert sc.same_summary(fixed, want) and ids == want_ids and states.tobytes() == want_state.tobytes()
    pictures, boxes, truths = rs.textured_clip("replaced")
    other, ids, states = _clip_on_device(torch_cuda, images, pictures, boxes, truths, params)
    assert len({i[1] for i in ids if len(i) > 1}) == 2 and other["switches"] == 0
    want, want_ids, want_state, _ = rs.host_chain(pictures, boxes, truths, params)
    assert sc.same_summary(other, want) and ids == want_ids and states.tobytes() == want_state.tobytes()


def test_detect_tracked_with_reid_on_a_still_video_of_the_real_images(network, torch_cuda, images, ptq):
    """three of the real pictures, each repeated for 4 steps as one stream: nothing is ever lost, so the ids are those without reid; the
    same through evaluate_tracking and detect_drawn; a ReId of another number of streams is refused"""
    real = real_images(ptq)
    streams, steps = 3, 4
    pictures = [real[s] for t in range(steps) for s in range(streams)]                     # time-major
    plain = images.detect_tracked(network, pictures, images.Tracker(streams), steps, layout="time")
    reid = images.ReId(streams, max_distance=rs.CLIP_MAX_DISTANCE)
    seen = images.detect_tracked(network, pictures, images.Tracker(streams), steps, layout="time", reid=reid)
    assert seen == plain and sum(len(f) for f in plain) > 0
    states = reid.states()
    assert (states["clock"] == steps).all() and sum(int((st["entry"]["id"] != 0).sum()) for st in states) == sum(len(f) for f in plain[:streams])
    truths = [[(k + 1, *row[1:5]) for k, row in enumerate(f)] for f in plain]
    a = images.evaluate_tracking(network, pictures, truths, images.Tracker(streams), steps, layout="time")
    b = images.evaluate_tracking(network, pictures, truths, images.Tracker(streams), steps, layout="time", reid=images.ReId(streams, max_distance=rs.CLIP_MAX_DISTANCE))
    assert sc.same_summary(a, b) and a["switches"] == 0
    drawn = images.detect_drawn(network, pictures, tracker=images.Tracker(streams), steps=steps)
    drawn_reid = images.detect_drawn(network, pictures, tracker=images.Tracker(streams), steps=steps, reid=images.ReId(streams, max_distance=rs.CLIP_MAX_DISTANCE))
    assert drawn_reid[1] == plain and all(x.tobytes() == y.tobytes() for x, y in zip(drawn[0], drawn_reid[0]))
    with pytest.raises(ValueError, match="streams"):
        images.detect_tracked(network, pictures, images.Tracker(streams), steps, reid=images.ReId(streams + 1))
    with pytest.raises(ValueError, match="only with a tracker"):
        images.detect_drawn(network, pictures, reid=reid)
