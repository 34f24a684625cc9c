"""The host build of the appearance descriptors and of the re-identification (csrc/yf_images_describe.h, csrc/yf_images_reid.h in
libyf_images_host.so) against their plain-Python statements, `ptq.describe_u8` / `ptq.describe_yuv420sp` and `ptq.reid_step`, exactly:
every byte of every array a call writes, each between guard bytes, every place that must not be written a sentinel.  No GPU."""
import numpy as np
import pytest

import reid_support as rs
import track_support as ts


# ---- descriptors ----
@pytest.mark.parametrize("batch", rs.describe_batches(), ids=lambda b: b.name)
def test_the_host_descriptors_are_the_statement(batch):
    want = rs.describe_expected(batch)
    got = rs.describe_host_run(batch)
    assert got.rc == len(batch.pictures) and rs.same_desc(got, want), batch.name
    if batch.name.startswith("sizes_"):
        # 8 x 8 valid; 7 x 8 and 8 x 7 invalid; 9 x 13 and 64 x 40 valid; inverted and outside: no region; the odd origin valid
        assert got.desc["flags"][0].tolist() == [1, 0, 0, 1, 1, 0, 0, 1]
        assert not got.desc["v"][0][[1, 2, 5, 6]].any() and got.desc["v"][0][[0, 3, 4, 7]].any(axis=1).all()
    if batch.name == "counts":
        # the slots beyond a frame's records are not touched; a count above cap is cap, a negative one 0; the invalid picture's are zero
        assert got.first.tolist() == [0, 0, 1, 4, 7, 7, 9] and got.status.tolist() == [0, 0, 0, 0, 0, 1]
        assert (got.desc["flags"][0] == 0xA5A5A5A5).all() and (got.desc["flags"][1, 1:] == 0xA5A5A5A5).all() and (got.desc["flags"][4] == 0xA5A5A5A5).all()
        assert got.desc["flags"][3].tolist() == [1, 1, 1] and not got.desc[5, :2].tobytes().strip(b"\0") and got.desc["flags"][5, 2] == 0xA5A5A5A5
    if batch.name == "constant":
        assert got.desc["flags"][0, 0] == 1 and (got.desc["v"][0, 0] == 93).all()
    if batch.name == "constant_nv21":
        assert got.desc["flags"][0, 0] == 1 and (got.desc["v"][0, 0] == 201).all()


def test_the_byte_order_is_the_formats_and_alpha_is_never_read():
    rng = np.random.default_rng(9110)
    rgb = rs.noise(rng, 20, 24, 3)
    box = [[(2, 3, 20, 17)]]
    base = rs.describe_host_run(rs.Batch("rgb", "rgb", [rgb], box, None, 1)).desc
    assert rs.describe_host_run(rs.Batch("bgr", "bgr", [rgb[..., ::-1].copy()], box, None, 1)).desc.tobytes() == base.tobytes()
    for alpha in (0, 255):
        a = np.full((20, 24, 1), alpha, np.uint8)
        assert rs.describe_host_run(rs.Batch("rgba", "rgba", [np.concatenate([rgb, a], axis=2)], box, None, 1)).desc.tobytes() == base.tobytes()
        assert rs.describe_host_run(rs.Batch("bgra", "bgra", [np.concatenate([rgb[..., ::-1], a], axis=2)], box, None, 1)).desc.tobytes() == base.tobytes()
    # ... and the weights are R 77, G 150, B 29: a pure colour of value 255 has luma (255 w + 128) // 256
    for ch, luma in ((0, 77), (1, 149), (2, 29)):
        pic = np.zeros((8, 8, 3), np.uint8)
        pic[..., ch] = 255
        assert (rs.describe_host_run(rs.Batch("pure", "rgb", [pic], [[(0, 0, 7, 7)]], None, 1)).desc["v"] == luma).all()


def test_a_constant_brightness_changes_no_distance_by_more_than_rounding_allows():
    """Adding k to every colour byte of a region (no byte clipped) adds exactly 256 k to every pixel's weighted sum, so every cell's exact
    mean luma moves by exactly k and so does its rounded byte: (S + 256 k cnt + 128 cnt) // (256 cnt) = (S + 128 cnt) // (256 cnt) + k.
    The descriptor's bytes all move by k, every term |(64 a_i - A) - (64 b_i - B)| is unchanged: THE BOUND IS 0.  (With clipping, or a
    gain, there is no such bound; the mean removal does not cover them.)  The Y plane likewise: (sum + k cnt + cnt // 2) // cnt."""
    rng = np.random.default_rng(9120)
    p = rs.ptq()
    box = [[(1, 2, 40, 30), (5, 5, 17, 16)]]
    for fmt in ("bgr", "rgba", "nv12"):
        dark = rng.integers(30, 200, (36, 44, 4 if fmt == "rgba" else 3), dtype=np.uint8) if fmt != "nv12" else rng.integers(30, 200, (36, 44), dtype=np.uint8)
        other = rng.integers(30, 200, dark.shape, dtype=np.uint8)
        wrap = (lambda a: (a, np.zeros((18, 44), np.uint8))) if fmt == "nv12" else (lambda a: a)
        d0 = rs.describe_host_run(rs.Batch("d", fmt, [wrap(dark)], box, None, 2)).desc
        d1 = rs.describe_host_run(rs.Batch("l", fmt, [wrap(dark + 37)], box, None, 2)).desc
        d2 = rs.describe_host_run(rs.Batch("o", fmt, [wrap(other)], box, None, 2)).desc
        assert (d1["v"].astype(int) - d0["v"].astype(int) == 37).all()
        for k in range(2):
            assert p.reid_distance(d0["v"][0, k], d1["v"][0, k]) == 0
            assert abs(p.reid_distance(d0["v"][0, k], d2["v"][0, k]) - p.reid_distance(d1["v"][0, k], d2["v"][0, k])) <= 0
            assert p.reid_distance(d0["v"][0, k], d2["v"][0, k]) > 0


def test_the_host_distance_is_the_statement_and_is_bounded():
    rng = np.random.default_rng(9130)
    lib, p = rs.reid_host(), rs.ptq()
    pairs = [(rng.integers(0, 256, 64, dtype=np.uint8), rng.integers(0, 256, 64, dtype=np.uint8)) for _ in range(50)]
    half = np.array([255] * 32 + [0] * 32, np.uint8)
    pairs += [(half, half[::-1].copy()), (np.zeros(64, np.uint8), np.full(64, 255, np.uint8)), (half, np.zeros(64, np.uint8))]
    for a, b in pairs:
        d = lib.yfi_reid_distance_host(a.ctypes.data, b.ctypes.data)
        assert d == p.reid_distance(a, b) == p.reid_distance(b, a) and 0 <= d <= rs.MAX_DISTANCE
    assert p.reid_distance(half, half[::-1]) == rs.MAX_DISTANCE and p.reid_distance(np.zeros(64), np.full(64, 255)) == 0


def test_the_describe_argument_checks():
    assert rs.describe_host_check() == ""
    for kw, text in rs.D_FAULTS:
        assert text in rs.describe_host_check(**kw), (kw, rs.describe_host_check(**kw))
    batch = rs.describe_batches()[0]
    lib = rs.reid_host()
    # a fault, or the other family's format: -1 and nothing written
    for fn, kw in ((lib.yfi_describe_records_yuv_host, {}), (lib.yfi_describe_records_host, dict(cap=0))):
        r = rs.describe_run_with(lambda *a: fn(*(a[:7] + (kw.get("cap", a[7]),) + a[8:])), batch)
        assert r.rc == -1 and (r.desc["flags"] == 0xA5A5A5A5).all() and (r.first == ts.SENTINEL32).all() and (r.status == ts.SENTINEL32).all()
    empty = rs.describe_host_run(batch, n=0)
    assert empty.rc == 0 and (empty.first == ts.SENTINEL32).all() and (empty.status == ts.SENTINEL32).all()


# ---- re-identification ----
@pytest.mark.parametrize("case", rs.designed(), ids=lambda c: c.name)
def test_the_host_reid_is_the_statement_on_the_designed_scenes(case):
    for layout in ts.LAYOUTS:
        call, streams, steps, state0 = rs.laid_out(case, layout)
        want = rs.expected(call, streams, steps, layout, case.out_cap, case.params, state0)
        got = rs.host_run(call, streams, steps, layout, case.out_cap, case.params, state0)
        assert got.rc == streams * steps and rs.same(got, want), (case.name, layout)
        # d_info_out == d_info, and the optionals NULL
        there = rs.host_run(call, streams, steps, layout, case.out_cap, case.params, state0, in_place=True)
        assert rs.same(there, rs.expected(call, streams, steps, layout, case.out_cap, case.params, state0, in_place=True)), (case.name, layout)
        bare = rs.host_run(call, streams, steps, layout, case.out_cap, case.params, state0, with_what=False, with_status=False)
        assert bare.state.tobytes() == want.state.tobytes() and bare.info.tobytes() == want.info.tobytes()
        assert (bare.what == ts.SENTINEL32).all() and (bare.status == ts.SENTINEL32).all()
    ids = lambda f: got.info["id"][f].tolist()
    kinds = lambda f: got.what[f].tolist()
    entry = got.state["entry"][0]
    if case.name == "lost_and_found":
        # (stream-major and time-major are the same for one stream)
        assert [ids(f) for f in range(6)] == [[7, 0xA5A5A5A5], [7, 0xA5A5A5A5], [0xA5A5A5A5] * 2, [0xA5A5A5A5] * 2, [7, 11], [11, 7]]
        assert kinds(4) == [rs.REIDENTIFIED, rs.BORN] and kinds(5) == [rs.KNOWN, rs.KNOWN] and kinds(0)[0] == rs.BORN and kinds(1)[0] == rs.KNOWN
        assert (int(entry["id"][0]), int(entry["alias"][0]), int(entry["seen"][0])) == (7, 9, 6) and int(got.state["clock"][0]) == 6
    if case.name == "ages":
        # entry 0 (age 10 = max_age) is kept and re-identified, entry 1 (age 11) was freed, and record 21 is born into it
        assert ids(0) == [7, 21] and kinds(0) == [rs.REIDENTIFIED, rs.BORN] and int(entry["id"][1]) == 21
    if case.name == "wrap":
        assert int(got.state["clock"][0]) == 1 and ids(2) == [7] and kinds(2) == [rs.REIDENTIFIED]
    if case.name == "wrap_late":
        assert int(got.state["clock"][0]) == 2 and ids(3) == [30] and kinds(3) == [rs.BORN] and int(entry["id"][0]) == 30
    if case.name == "threshold":
        assert ids(0) == [7, 41] and kinds(0) == [rs.REIDENTIFIED, rs.BORN]
    if case.name == "tie_records":
        assert ids(0) == [7, 41] and kinds(0) == [rs.REIDENTIFIED, rs.BORN]
    if case.name == "tie_entries":
        assert ids(0) == [7] and int(entry["alias"][2]) == 40 and int(entry["alias"][6]) == 8
    if case.name == "nearest_first":
        assert ids(0) == [8, 7]
    if case.name == "odd_records":
        assert kinds(0) == [0, rs.KNOWN, rs.KNOWN, rs.KNOWN, rs.KNOWN, rs.BORN, 0, rs.BORN] and ids(0) == [0, 7, 7, 8, 8, 55, 0, 56]
        assert got.status.tolist() == [rs.VOID, 0]
    if case.name == "blend_0":
        assert entry["v"][0].tolist() == rs.vec(1) and kinds(2) == [rs.REIDENTIFIED]
    if case.name == "blend_256":
        assert entry["v"][0].tolist() == rs.vec(3) and kinds(2) == [rs.BORN]             # the stored face had become c
    if case.name == "counts":
        assert got.status.tolist() == [rs.CLIPPED, 0, 0, 0] and kinds(1) == [ts.SENTINEL32] * 3 and kinds(3) == [rs.KNOWN, rs.KNOWN, ts.SENTINEL32]
    if case.name == "beyond_64":
        assert got.status.tolist() == [rs.CLIPPED, rs.CLIPPED] and ids(0)[64:] == [264 + k for k in range(6)] and kinds(0)[64:] == [0] * 6
        assert kinds(1)[:64] == [rs.KNOWN] * 64 and kinds(1)[68:] == [0, ts.SENTINEL32]
    if case.name == "evict":
        # every entry is unbound; ages 1 .. 7 repeat with the index: the oldest are 6, 13, 20, 27, 34
        assert [int(entry["id"][k]) for k in (6, 13, 20, 27, 34)] == [900, 901, 902, 903, 904]
    if case.name == "full_64":
        # 21 records are known by their alias; of the others, records 18 and 21 find the entries of their own descriptors, 36 and 42,
        # the only such entries not yet expired (ages 3 and 2); 41 are born
        assert sorted(kinds(0)) == [rs.KNOWN] * 21 + [rs.REIDENTIFIED] * 2 + [rs.BORN] * 41 and set(kinds(1)) == {rs.KNOWN}
        assert [k for k in range(64) if kinds(0)[k] == rs.REIDENTIFIED] == [18, 21] and ids(0)[18] == 536 and ids(0)[21] == 542


@pytest.mark.parametrize("streams,steps", [(1, 1), (3, 7), (5, 40)])
def test_the_host_reid_is_the_statement_on_random_clips_in_both_layouts(streams, steps):
    frames = rs.drift_frames(streams, steps)
    states = {}
    for state0 in (rs.empty_state(streams), rs.junk_state(streams)):
        for layout in ts.LAYOUTS:
            call = rs.lay_out(frames, rs.D_CAP, layout)
            got = rs.host_run(call, streams, steps, layout, rs.D_CAP, rs.D_PARAMS, state0)
            assert rs.same(got, rs.expected(call, streams, steps, layout, rs.D_CAP, rs.D_PARAMS, state0)), (streams, steps, layout)
            states[layout] = got.state.tobytes()
        assert states[ts.TIME] == states[ts.STREAM]
    if steps == 40:
        call = rs.lay_out(frames, rs.D_CAP, ts.TIME)
        whole = rs.host_run(call, streams, steps, ts.TIME, rs.D_CAP, rs.D_PARAMS, rs.empty_state(streams))
        assert rs.same(rs.split_calls(rs.host_run, call, streams, steps, rs.D_CAP, rs.D_PARAMS, rs.empty_state(streams)), whole)
        kinds = whole.what[whole.what != ts.SENTINEL32]
        assert all((kinds == k).any() for k in (0, rs.KNOWN, rs.REIDENTIFIED, rs.BORN))


def test_the_reid_argument_checks():
    assert rs.host_check() == ""
    for kw, text in rs.FAULTS:
        assert text in rs.host_check(**kw), (kw, rs.host_check(**kw))
    case = rs.designed()[0]
    call, streams, steps, state0 = rs.laid_out(case, ts.TIME)
    for params, out_cap in (((-1, 5, 5), 2), ((5, 5, 300), 2), (None, 2), ((5, 5, 5), 0)):
        lib = rs.reid_host()
        fn = lambda *a: lib.yf_images_reid_host(*(a[:3] + (out_cap,) + a[4:]), None)
        r = rs.run_with(fn, call, streams, steps, ts.TIME, case.out_cap, params, state0)
        assert r.rc == -1 and r.state.tobytes() == state0.tobytes() and (r.what == ts.SENTINEL32).all() and (r.status == ts.SENTINEL32).all()
    for streams0, steps0 in ((0, 5), (1, 0), (0, 0)):
        r = rs.host_run(call, streams0, steps0, ts.TIME, case.out_cap, case.params, state0)
        assert r.rc == 0 and r.state.tobytes() == state0.tobytes() and (r.what == ts.SENTINEL32).all()
    assert rs.reid_host().yf_images_reid_state_bytes_host(3) == 3 * 5128 and rs.reid_host().yf_images_reid_state_bytes_host(0) == 0


# ---- the behaviour, on the host chain: tracker, descriptors, re-identification, score ----
def test_a_face_hidden_for_longer_than_max_misses_keeps_its_id_and_a_different_face_does_not_take_it():
    params = (rs.CLIP_MAX_DISTANCE, 60, 64)
    pictures, boxes, truths = rs.textured_clip("occlusion")
    plain, ids, _, _ = rs.host_chain(pictures, boxes, truths, None)
    assert plain["switches"] >= 1 and len({i[1] for i in ids if len(i) > 1}) == 2            # face 2 under two ids
    fixed, ids, state, _ = rs.host_chain(pictures, boxes, truths, params)
    assert fixed["switches"] == 0 and len({i[1] for i in ids if len(i) > 1}) == 1 and fixed["mota"] > plain["mota"]
    # a DIFFERENT face after the gap must not take the lost identity
    pictures, boxes, truths = rs.textured_clip("replaced")
    other, ids, state, _ = rs.host_chain(pictures, boxes, truths, params)
    assert len({i[1] for i in ids if len(i) > 1}) == 2 and other["switches"] == 0
    # the distances behind the choice of CLIP_MAX_DISTANCE: the stored face 2 against what the returning boxes show
    p = rs.ptq()
    stored = p.describe_u8(pictures[7], boxes[7][1], "bgr")
    same_face = rs.textured_clip("occlusion")
    assert max(p.reid_distance(stored, p.describe_u8(same_face[0][t], same_face[1][t][1], "bgr")) for t in range(20, 30)) < rs.CLIP_MAX_DISTANCE
    assert min(p.reid_distance(stored, p.describe_u8(pictures[t], boxes[t][1], "bgr")) for t in range(20, 30)) > rs.CLIP_MAX_DISTANCE
