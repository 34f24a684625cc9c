"""What the tests of the optimal assignment share (test_track_assign_*): the expectation of a call -- `ptq.track_motion_step(assign=...)`,
the plain-Python statement of csrc/yf_images_assign.h --, the host build's prototypes and runners (the entry, its check, the match alone
and the procedure alone on a table of weights), and the designed scenes: the minimal scene of two tracks and two detections on which the
greedy match strands a detection, sequences of two faces that pass each other, the 64 x 64 scene of equal weights, a staircase of strips
over tiles that forces augmenting paths through all 64 columns, and sequences on which every detection and every slot has at most one eligible
partner (there the two matches are the same).  The record and state layouts, the guarded runner and the random sequences are
tests/track_support.py's and tests/motion_support.py's.

A call's params here are motion_support's seven numbers; `assign` is 0 (greedy) or 1 (optimal)."""
import ctypes
import functools

import numpy as np

import motion_support as ms
import track_support as ts

GREEDY, OPTIMAL = 0, 1
NAMES = {GREEDY: "greedy", OPTIMAL: "optimal"}
TOP = 2 ** 30 + 1
BASE_GAINS = ms.BASE_LIKE + (0,)            # (256, 0, 256, 0): the base tracker, with either match
SUGGESTED = ms.SUGGESTED + (0,)


def rec(box, j=0):
    """a record of `ptq`'s form around a box"""
    return (0, 0, 0, 0, 0, 0.9 - 0.001 * j, *box)


def expected(dets, counts, streams, steps, layout, cap, params, assign, state0, out_cap, stats=None):
    """the call by the Python statement -> ts.Result; nothing of the inputs is changed"""
    ptq = ts._mod("ptq")
    n = streams * steps
    out, info, out_counts, status = ts.sentinels(n, out_cap)
    state = state0.copy()
    for s in range(streams):
        st = ms.state_to_py(state[s])
        for t in range(steps):
            f = ts.frame_of(s, t, streams, steps, layout)
            st, emitted, bits = ptq.track_motion_step(st, dets[f].tolist(), params, count=int(counts[f]), cap=cap, frame=f, stats=stats,
                                                      assign=NAMES[assign])
            out_counts[f], status[f] = len(emitted), bits
            for r, (record, inf) in enumerate(emitted[:out_cap]):
                out[f, r], info[f, r] = record, inf
        state[s] = ms.py_to_state(st)
    return ts.Result(n, state, out, info, out_counts, status)


# ---- the host build ----
@functools.lru_cache(maxsize=None)
def assign_host():
    """libyf_images_host.so with the prototypes of csrc/yf_images_assign.h's host build added"""
    lib = ms.motion_host()
    vp, ci, cl, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_int64
    lib.yf_images_track_motion_assign_host.restype = cl
    lib.yf_images_track_motion_assign_host.argtypes = [vp, vp, cl, cl, ci, ci, vp, ci, vp, vp, vp, vp, ci, vp, vp]
    lib.yfi_assign_check_host.restype = ci
    lib.yfi_assign_check_host.argtypes = [vp, vp, cl, cl, ci, ci, vp, ci, vp, vp, vp, vp, ci, vp, ctypes.c_char_p, ci]
    lib.yfi_assign_match_host.restype = i64
    lib.yfi_assign_match_host.argtypes = [vp, vp, vp, ci, ctypes.c_double, vp, vp, vp]
    lib.yfi_assign_solve_host.restype = i64
    lib.yfi_assign_solve_host.argtypes = [vp, ci, vp, vp]
    return lib


def host_run(dets, counts, streams, steps, layout, cap, params, assign, state0, out_cap, with_status=True):
    lib = assign_host()

    def call(d, c, streams, steps, layout, cap, params, state, out, info, oc, out_cap, status):
        p = ms.c_params(params)
        return lib.yf_images_track_motion_assign_host(d, c, streams, steps, layout, cap, ctypes.byref(p), assign, state, out, info, oc, out_cap,
                                                      status, None)
    return ts.run_with(call, dets, counts, streams, steps, layout, cap, params, state0, out_cap, with_status)


def host_check(assign=OPTIMAL, **kw):
    """yfi_assign_check on made-up addresses -> the text of the first fault, '' for none"""
    a = dict(ms.VALID, **kw)
    text = ctypes.create_string_buffer(256)
    p = None if a["params"] is None else ctypes.byref(ms.c_params(a["params"]))
    rc = assign_host().yfi_assign_check_host(a["dets"], a["counts"], a["streams"], a["steps"], a["layout"], a["cap"], p, assign, a["state"],
                                             a["out"], a["info"], a["out_counts"], a["out_cap"], a["status"], text, 256)
    assert rc == (text.value != b"")
    return text.value.decode()


BAD_ASSIGNS = (-1, 2, 3, ts.I32MIN, ts.I32MAX)


def host_match(boxes, dets, match_iou):
    """the host build's match of one step: boxes {slot: (x1, y1, x2, y2)}, dets [(x1, y1, x2, y2)] -> (slot_det, det_slot, total, weights)
    in `ptq.track_assign_match`'s form, with the table of weights as a list of rows"""
    m = len(dets)
    b = np.zeros((64, 4), np.int32)
    occ = np.zeros(64, np.int32)
    for k, box in boxes.items():
        b[k], occ[k] = box, 1
    d = np.zeros(max(m, 1), ts.RAW)
    for j, box in enumerate(dets):
        d[j] = (0, 0, 0, 0, 0, 0, *box)
    slot_det, det_slot = np.full(64, -7, np.int32), np.full(max(m, 1), -7, np.int32)
    w = np.full((max(m, 1), 64), -7, np.int32)
    total = assign_host().yfi_assign_match_host(b.ctypes.data, occ.ctypes.data, d.ctypes.data, m, match_iou, slot_det.ctypes.data,
                                                det_slot.ctypes.data, w.ctypes.data)
    return ({k: int(j) for k, j in enumerate(slot_det) if j >= 0}, {j: int(k) for j, k in enumerate(det_slot[:m]) if k >= 0}, int(total),
            w[:m].tolist())


def host_solve(w):
    """the host build's procedure on a table of weights (rows of 64) -> (slot_det, det_slot, total)"""
    m = len(w)
    a = np.ascontiguousarray(np.array(w, np.int32).reshape(m, 64)) if m else np.zeros((1, 64), np.int32)
    slot_det, det_slot = np.full(64, -7, np.int32), np.full(max(m, 1), -7, np.int32)
    total = assign_host().yfi_assign_solve_host(a.ctypes.data, m, slot_det.ctypes.data, det_slot.ctypes.data)
    return {k: int(j) for k, j in enumerate(slot_det) if j >= 0}, {j: int(k) for j, k in enumerate(det_slot[:m]) if k >= 0}, int(total)


def greedy_total(w):
    """the total weight of the global greedy match on a table of weights (ties: the lower detection, then the lower slot)"""
    pairs = sorted((-w[i][j], i, j) for i in range(len(w)) for j in range(64) if w[i][j] > 0)
    rows, cols, total = set(), set(), 0
    for neg, i, j in pairs:
        if i not in rows and j not in cols:
            rows.add(i), cols.add(j)
            total -= neg
    return total


# ---- the minimal scene: at match_iou 0.3 greedy takes A-d0 (0.6) and strands d1; optimal takes B-d0 and A-d1 (0.504 each) ----
A, B, D0, D1 = (0, 0, 99, 99), (58, 0, 157, 99), (25, 0, 124, 99), (-33, 0, 66, 99)
M_PARAMS = (0.3, 1, 5)


def minimal_frames():
    """one stream: A and B are born in slots 0 and 1 (ids 1 and 2), then d0 and d1 arrive"""
    return [[([A, B], None), ([D0, D1], None)]]


# ---- two faces of 100 x 100 passing each other over 12 steps ----
C_STEPS, C_CAP = 12, 4


def crossing_frames():
    """stream 0: P moves right by 40 a step, Q left by 5, a little jitter; they overlap from step 5 on, and the frame lists Q first on odd
    steps.  Stream 1: the minimal scene's motion kept up -- two neighbours that both move left by 33 a step (a pan), where the greedy
    match strands a detection step after step without a motion model."""
    cross, pan = [], []
    for t in range(C_STEPS):
        px, qx = -150 + 40 * t + (3 if t % 3 == 0 else 0), 150 - 5 * t
        boxes = [(px, 0, px + 99, 99), (qx, 3, qx + 99, 102)]
        cross.append((boxes if t % 2 == 0 else boxes[::-1], None))
        ax, bx = -33 * t, 58 - 33 * t
        pan.append(([(bx, 0, bx + 99, 99), (ax, 0, ax + 99, 99)] if t % 4 == 3 else [(ax, 0, ax + 99, 99), (bx, 0, bx + 99, 99)], None))
    return [cross, pan]


# ---- 64 tracks and 64 detections, every pair eligible with the same weight: 2080 rounds of the search ----
def all_equal_scene():
    """-> (boxes {slot: box}, dets): 64 identical boxes and 64 identical detections of them"""
    return {k: (10, 10, 49, 59) for k in range(64)}, [(12, 10, 51, 59)] * 64


def all_equal_state():
    """the scene as a state of one stream (64 tracks at the same box, ids 1 .. 64) -> (state0, frames of two steps)"""
    st = ms.empty_state(1)
    for k in range(64):
        st["slot"]["base"][0, k] = (k + 1, 2, 0, 3, (7, 1, 2, 3, 4, ts.conf_bits(k), 10, 10, 49, 59))
        st["slot"]["pos"][0, k] = (2560, 2560, 256 * 49, 256 * 59)
    st["issued"] = 64
    return st, [[([(12, 10, 51, 59)] * 64, None), ([(11, 10, 50, 59)] * 64, None)]]


# ---- a staircase: w[i][j] maximal for j <= i and 0 for j > i ----
STAIR_IOU = 0.01


def staircase_scene():
    """slot j is the tile x in [10 j, 10 j + 9] of a row of 64 disjoint tiles; detection i is the strip over the tiles 0 .. i: its IoU with
    each of them is 1 / (i + 1) and it shares no pixel with the others, so at match_iou 0.01 row i of the table is 1 + 2^30 // (i + 1) in
    the columns j <= i and 0 beyond.  The detections are listed in DESCENDING i: every row ties on column 0, every search walks through
    all the columns assigned so far (2080 rounds in all), and the last row -- the strip over tile 0 alone -- moves every earlier
    detection one column up: an augmenting path through all 64 columns."""
    boxes = {j: (10 * j, 0, 10 * j + 9, 9) for j in range(64)}
    return boxes, [(0, 0, 10 * i + 9, 9) for i in range(63, -1, -1)]


def scene_state(boxes, issued=None):
    """a scene's boxes as the state of one stream: slot k a track of id k + 1 at its box, at rest"""
    st = ms.empty_state(1)
    for k, box in boxes.items():
        st["slot"]["base"][0, k] = (k + 1, 2, 0, 3, (7, 1, 2, 3, 4, ts.conf_bits(k), *box))
        st["slot"]["pos"][0, k] = tuple(256 * v for v in box)
    st["issued"] = max(boxes) + 1 if issued is None and boxes else (issued or 0)
    return st


# ---- sequences on which no detection and no slot has two eligible partners ----
def sparse_frames(streams=3, steps=6):
    """boxes of a coarse grid (pitch 60, side 20 to 30) that drift by at most 3 pixels a step, drop out and come back: a box meets its own
    track only"""
    rng = np.random.default_rng(7100)
    frames = []
    for s in range(streams):
        objects = [[60 * (k % 5) + int(rng.integers(0, 8)), 60 * (k // 5) + int(rng.integers(0, 8)), int(rng.integers(20, 31)), int(rng.integers(20, 31))]
                   for k in range(3 + 2 * s)]
        clip = []
        for t in range(steps):
            for o in objects:
                o[0] += int(rng.integers(-3, 4))
                o[1] += int(rng.integers(-3, 4))
            boxes = [(o[0], o[1], o[0] + o[2] - 1, o[1] + o[3] - 1) for o in objects if rng.random() > 0.2]
            clip.append(([boxes[int(k)] for k in rng.permutation(len(boxes))], None))
        frames.append(clip)
    return frames


def max_degree(dets, counts, streams, steps, layout, cap, params, state0):
    """the largest number of eligible partners any detection or slot has in any frame of the call, by the statement (greedy and optimal
    agree while it is <= 1, so the states of either serve)"""
    ptq = ts._mod("ptq")
    worst = 0
    for s in range(streams):
        st = ms.state_to_py(state0[s])
        for t in range(steps):
            f = ts.frame_of(s, t, streams, steps, layout)
            m = min(max(int(counts[f]), 0), cap, 64)
            recs = dets[f].tolist()[:m]
            boxes = {k: (0,) * 6 + tuple(ptq.motion_box(ptq.motion_sat(p) + ptq.motion_sat(v)) for p, v in zip(sl[6], sl[7]))
                     for k, sl in enumerate(st["slots"]) if sl[0] != 0}
            w = ptq.track_assign_weights(boxes, recs, float(params[0]))
            if w:
                worst = max(worst, max(sum(x > 0 for x in row) for row in w), max(sum(row[j] > 0 for row in w) for j in range(64)))
            st = ptq.track_motion_step(st, recs, params, count=m, cap=cap, frame=f)[0]
    return worst


def junk_call(layout):
    """a state of random bytes (two streams, the second's table full), met by records at the boxes its slots predict"""
    junk = ms.junk_state(2, seed=7200, full=(1,))
    boxes = [ms.predicted_box(junk, s, k) for s in (0, 1) for k in (3, 17)]
    near = [(10, 10, 40, 40), (100, 100, 140, 140), (12, 9, 41, 42)]
    frames = [[(boxes + near[:1], None), (boxes[:2] + near[1:], None), (near, None)], [(near[1:2] + boxes, None), (near[::-1], None), ([], None)]]
    dets, counts = ts.lay_out(frames, 6, layout)
    return dets, counts, junk
