"""What the tests of the score of tracks against labelled identities share (test_track_score_*): the ground-truth, state and summary
layouts as numpy dtypes, the expectation of a call -- `ptq.track_score_step`, the plain-Python statement of csrc/yf_images_score.h, run
stream by stream and step by step --, the host build's prototypes with a runner that puts guard bytes in front of and behind every array a
call may write, the designed scenes and the seeded random ones.  The record and info layouts, the guards and the layouts of a call are
tests/track_support.py's; the tracker's scenes are tests/assign_support.py's.

A scene is `frames[s][t] = (truths, hyps, gt_count, out_count)`: the labelled objects (id, x1, y1, x2, y2) and the reported tracks
(id, x1, y1, x2, y2) of stream s at step t in the order they lie, and the two counts (None: the lengths).  `lay_out` makes the arrays of a
call from it in either layout; the places of a row that hold nothing are 0xA5 bytes."""
import ctypes
import functools
import os
import re
from collections import namedtuple

import numpy as np

import assign_support as asg
import motion_support as ms
import track_support as ts
from conftest import ROOT
from images_support import host_lib

GT = np.dtype([("id", "<u4"), ("x1", "<i4"), ("y1", "<i4"), ("x2", "<i4"), ("y2", "<i4")])
COUNTERS = ("frames", "gt", "hyp", "matches", "misses", "false_positives", "switches", "overlap")
STATE = np.dtype([(name, "<u8") for name in COUNTERS] + [("last", "<u4", (256,)), ("present", "<i4", (256,)), ("tracked", "<i4", (256,))])
SUMMARY = np.dtype([(name, "<u8") for name in COUNTERS] + [("objects", "<i8"), ("mostly_tracked", "<i8"), ("mostly_lost", "<i8"),
                                                            ("mota", "<f8"), ("motp", "<f8")])
assert (GT.itemsize, STATE.itemsize, SUMMARY.itemsize) == (20, 3136, 104)
GT_CLIPPED, HYP_CLIPPED, GT_VOID, HYP_VOID = 1, 2, 4, 8
TOP = asg.TOP
U32MAX, U64MAX = 2 ** 32 - 1, 2 ** 64 - 1

Case = namedtuple("Case", "name frames gt_cap out_cap score_iou state0")
Result = namedtuple("Result", "rc state match status")


def same(a, b):
    """two results equal in every byte: the return value, the whole state, the matches and the status"""
    return a.rc == b.rc and all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:]))


def lay_out(frames, gt_cap, out_cap, layout):
    """frames[s][t] = (truths, hyps, gt_count, out_count) -> (out RAW [n, out_cap], info INFO [n, out_cap], out_counts, gt GT [n, gt_cap],
    gt_counts) of a call in `layout`"""
    streams, steps = len(frames), len(frames[0]) if frames else 0
    n = max(streams * steps, 1)
    out = np.frombuffer(bytes([0xA5]) * (n * out_cap * 28), ts.RAW).reshape(n, out_cap).copy()
    info = np.frombuffer(bytes([0xA5]) * (n * out_cap * 16), ts.INFO).reshape(n, out_cap).copy()
    gt = np.frombuffer(bytes([0xA5]) * (n * gt_cap * 20), GT).reshape(n, gt_cap).copy()
    out_counts, gt_counts = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for s in range(streams):
        assert len(frames[s]) == steps
        for t in range(steps):
            truths, hyps, gt_count, out_count = frames[s][t]
            f = ts.frame_of(s, t, streams, steps, layout)
            assert len(truths) <= gt_cap and len(hyps) <= out_cap
            gt_counts[f] = len(truths) if gt_count is None else gt_count
            out_counts[f] = len(hyps) if out_count is None else out_count
            for i, row in enumerate(truths):
                gt[f, i] = row
            for j, (hid, *box) in enumerate(hyps):
                out[f, j] = (f, s % 3, t % 7, j % 7, 5, ts.conf_bits(j), *box)
                info[f, j] = (hid, 1 + t, 0, 1 + t)
    return out, info, out_counts, gt, gt_counts


def empty_state(streams):
    return np.zeros(max(streams, 1), STATE)


def state_to_py(rec):
    return {"counters": [int(rec[name]) for name in COUNTERS], "last": rec["last"].tolist(), "present": rec["present"].tolist(),
            "tracked": rec["tracked"].tolist()}


def py_to_state(st):
    rec = np.zeros((), STATE)
    for name, v in zip(COUNTERS, st["counters"]):
        rec[name] = v
    rec["last"], rec["present"], rec["tracked"] = st["last"], st["present"], st["tracked"]
    return rec


def sentinels(n, gt_cap):
    """match int32 [n, gt_cap], status int32 [n], every byte 0xA5"""
    n = max(n, 1)
    return np.full((n, gt_cap), ts.SENTINEL32, np.int32), np.full(n, ts.SENTINEL32, np.int32)


def rows_of(arr, f, count, cap, fields):
    return [tuple(int(arr[f, k][name]) for name in fields) for k in range(min(max(int(count), 0), cap, 64))]


def expected(call, streams, steps, layout, gt_cap, out_cap, score_iou, state0, stats=None):
    """the call by the Python statement -> Result; nothing of the inputs is changed"""
    ptq = ts._mod("ptq")
    out, info, out_counts, gt, gt_counts = call
    n = streams * steps
    match, status = sentinels(n, gt_cap)
    state = state0[:max(streams, 1)].copy()
    for s in range(streams):
        st = state_to_py(state[s])
        for t in range(steps):
            f = ts.frame_of(s, t, streams, steps, layout)
            truths = rows_of(gt, f, gt_counts[f], gt_cap, GT.names)
            boxes = rows_of(out, f, out_counts[f], out_cap, ("x1", "y1", "x2", "y2"))
            hyps = [(int(info[f, j]["id"]),) + box for j, box in enumerate(boxes)]
            st, m, bits = ptq.track_score_step(st, truths, hyps, score_iou, gt_count=int(gt_counts[f]), gt_cap=gt_cap,
                                               out_count=int(out_counts[f]), out_cap=out_cap, stats=stats)
            match[f, :len(m)], status[f] = m, bits
        state[s] = py_to_state(st)
    return Result(n, state, match, status)


# ---- the host build ----
@functools.lru_cache(maxsize=None)
def score_host():
    """libyf_images_host.so with the prototypes of csrc/yf_images_score.h's host build added"""
    lib = asg.assign_host()
    vp, ci, cl, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_double
    lib.yf_images_score_tracks_host.restype = cl
    lib.yf_images_score_tracks_host.argtypes = [vp, vp, vp, ci, vp, vp, ci, cl, cl, ci, cd, vp, vp, vp, vp]
    lib.yfi_score_check_host.restype = ci
    lib.yfi_score_check_host.argtypes = [vp, vp, vp, ci, vp, vp, ci, cl, cl, ci, cd, vp, vp, vp, ctypes.c_char_p, ci]
    lib.yf_images_score_state_bytes_host.restype = ctypes.c_size_t
    lib.yf_images_score_state_bytes_host.argtypes = [cl]
    lib.yf_images_score_summary_host.restype = ci
    lib.yf_images_score_summary_host.argtypes = [vp, cl, vp]
    return lib


def run_with(fn, call, streams, steps, layout, gt_cap, out_cap, score_iou, state0, with_match=True, with_status=True, upload=None,
             download=None):
    """`fn(out, info, out_counts, out_cap, gt, gt_counts, gt_cap, streams, steps, layout, score_iou, state, match, status)` on addresses,
    every written array between guard bytes -> Result.  upload / download: the buffers' way to the device and back (the GPU tests)."""
    n = streams * steps
    arrays = [state0[:max(streams, 1)].copy(), *sentinels(n, gt_cap)]
    bufs = [ts.guarded(a)[0] for a in arrays]
    ins = [np.ascontiguousarray(a) for a in call]
    if upload is not None:
        bufs, ins = [upload(b) for b in bufs], [upload(a.view(np.uint8).reshape(-1)) for a in ins]
        addr = lambda b: b.data_ptr()
    else:
        addr = lambda b: b.ctypes.data
    p = [addr(b) + ts.GUARD for b in bufs]
    rc = fn(addr(ins[0]), addr(ins[1]), addr(ins[2]), out_cap, addr(ins[3]), addr(ins[4]), gt_cap, streams, steps, layout, score_iou, p[0],
            p[1] if with_match else None, p[2] if with_status else None)
    if download is not None:
        bufs = [download(b) for b in bufs]
    assert all(ts.guards_intact(b) for b in bufs), "a byte outside an array was written"
    got = [b[ts.GUARD:-ts.GUARD].view(a.dtype).reshape(a.shape) for a, b in zip(arrays, bufs)]
    return Result(rc, *got)


def host_run(call, streams, steps, layout, gt_cap, out_cap, score_iou, state0, with_match=True, with_status=True):
    lib = score_host()
    fn = lambda *a: lib.yf_images_score_tracks_host(*a, None)
    return run_with(fn, call, streams, steps, layout, gt_cap, out_cap, score_iou, state0, with_match, with_status)


VALID = dict(out=8, info=8, out_counts=8, out_cap=4, gt=8, gt_counts=8, gt_cap=4, streams=2, steps=3, layout=ts.TIME, score_iou=0.5, state=8,
             match=8, status=0)
NAMES = tuple(VALID)
POINTERS = ("out", "info", "out_counts", "gt", "gt_counts", "state", "match", "status")


def host_check(**kw):
    """yfi_score_check on made-up addresses -> the text of the first fault, '' for none"""
    a = dict(VALID, **kw)
    text = ctypes.create_string_buffer(256)
    rc = score_host().yfi_score_check_host(*(a[k] for k in NAMES), text, 256)
    assert rc == (text.value != b"")
    return text.value.decode()


# one case per check, as keyword changes of `host_check`'s valid call, with a part of the text
FAULTS = [(dict(out=0), "is NULL"), (dict(info=0), "is NULL"), (dict(out_counts=0), "is NULL"), (dict(gt=0), "is NULL"),
          (dict(gt_counts=0), "is NULL"), (dict(state=0), "is NULL"),
          (dict(out=10), "4-byte aligned"), (dict(info=7), "4-byte aligned"), (dict(out_counts=5), "4-byte aligned"), (dict(gt=6), "4-byte aligned"),
          (dict(gt_counts=9), "4-byte aligned"), (dict(match=2), "4-byte aligned"), (dict(status=6), "4-byte aligned"),
          (dict(state=12), "8-byte aligned"), (dict(out_cap=0), "out_cap"), (dict(out_cap=-4), "out_cap"),
          (dict(gt_cap=0), "gt_cap must be in [1, 64]"), (dict(gt_cap=65), "gt_cap must be in [1, 64]"), (dict(score_iou=float("nan")), "score_iou is NaN"),
          (dict(layout=2), "layout"), (dict(layout=-1), "layout"), (dict(streams=-1), "streams and steps"), (dict(steps=-1), "streams and steps"),
          (dict(streams=2 ** 31, steps=1), "streams * steps"), (dict(streams=65536, steps=32768), "streams * steps")]


# ---- the summary ----
def host_summary(states):
    """yf_images_score_summary's body in the host build on STATE [k] -> a dict of its fields, the doubles as they are"""
    raw = np.ascontiguousarray(states).view(np.uint8).reshape(-1)
    out = np.zeros(1, SUMMARY)
    rc = score_host().yf_images_score_summary_host(raw.ctypes.data if raw.size else None, raw.size // STATE.itemsize, out.ctypes.data)
    assert rc == 0
    return {name: (float if name in ("mota", "motp") else int)(out[0][name]) for name in SUMMARY.names}


def py_summary(states):
    return ts._mod("ptq").track_score_summary([state_to_py(states[s]) for s in range(len(states))])


def same_summary(a, b):
    """two summaries equal, the doubles bit for bit"""
    return a.keys() == b.keys() and all(np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes() if k in ("mota", "motp") else a[k] == b[k]
                                        for k in a)


# ---- the designed scenes ----
A, B = (0, 0, 99, 99), (200, 0, 299, 99)


def crafted(last=(), present=(), tracked=(), **counters):
    """a state of one stream: last / present / tracked = {ground-truth id: value}"""
    st = empty_state(1)
    for name, v in counters.items():
        st[name] = v
    for table, entries in (("last", last), ("present", present), ("tracked", tracked)):
        for o, v in dict(entries).items():
            st[table][0, o - 1] = v
    return st


def swap_frames():
    """the hand-counted minimal case: objects 1 and 2 keep hypotheses 7 and 9 for three frames, on the fourth the hypothesis ids are
    exchanged and on the fifth they stay exchanged: 2 switches, both on the fourth frame"""
    kept, swapped = [(7, *A), (9, *B)], [(9, *A), (7, *B)]
    truth = [(1, *A), (2, *B)]
    return [[(truth, kept, None, None)] * 3 + [(truth, swapped, None, None)] * 2]


# continuity against the optimum at score_iou 0.5: the kept pairs have IoU 67 / 133 each, the exchanged partners 93 / 107 each
C_T1, C_T2, C_H5, C_H6 = (0, 0, 99, 99), (40, 0, 139, 99), (33, 0, 132, 99), (7, 0, 106, 99)


def continuity_frames():
    first = ([(1, *C_T1), (2, *C_T2)], [(5, *C_T1), (6, *C_T2)], None, None)
    second = ([(1, *C_T1), (2, *C_T2)], [(5, *C_H5), (6, *C_H6)], None, None)
    return [[first, second]]


@functools.lru_cache(maxsize=None)
def designed():
    """the designed scenes, each at the smallest size that can go wrong -> [Case]"""
    cases = [Case("swap", swap_frames(), 2, 2, 0.5, None), Case("continuity", continuity_frames(), 2, 2, 0.5, None)]
    # the second frame of `continuity` from the empty state: nothing is kept, the optimum exchanges the partners
    cases.append(Case("optimum", [continuity_frames()[0][1:]], 2, 2, 0.5, None))
    # objects 1 and 2 were both last matched to hypothesis 5: the lower row keeps it, the other goes to the search (and switches to 6)
    near = [(1, 0, 0, 99, 99), (2, 10, 0, 109, 99)]
    cases.append(Case("same_last", [[(near, [(6, 8, 0, 107, 99), (5, 4, 0, 103, 99)], None, None)]], 3, 3, 0.5, crafted(last={1: 5, 2: 5})))
    # an object absent for two frames returns under another id (stream 0: one switch) or under the same (stream 1: none)
    seen, gone = ([(1, *A)], [(3, *A)], None, None), ([], [], None, None)
    cases.append(Case("returns", [[seen, seen, gone, gone, ([(1, *A)], [(4, *A)], None, None)], [seen, seen, gone, gone, seen]], 2, 2, 0.5, None))
    # void rows (id 0, 257, UINT32_MAX, a repeat), a record of id 0, counts above the caps, counts below 0: one frame per status bit,
    # one with all of them, one with none
    rows = [(0, *A), (257, *A), (U32MAX, *A), (5, *B), (5, *A), (6, *A)]
    hyps = [(11, *A), (12, *B)]
    cases.append(Case("voids", [[(rows, hyps, None, None), ([(5, *B), (6, *A)], [(0, *A), (12, *B)], None, None),
                                 ([(5, *B), (6, *A)] + [(7 + k, 400, 0, 420, 20) for k in range(4)], hyps, 9, None), ([(5, *B), (6, *A)], hyps + [(13, *A)], None, 5),
                                 (rows, [(0, *B), (11, *A), (12, *B)], 2 ** 31 - 1, 70), (rows, hyps, -1, ts.I32MIN), ([(5, *B), (6, *A)], hyps, None, None)]],
                      6, 3, 0.5, None))
    # no hypotheses, no ground truth, neither
    cases.append(Case("empty", [[([(1, *A), (2, *B)], [], None, None), ([], [(7, *A), (9, *B)], None, None), ([], [], None, None),
                                 ([(1, *A)], [(7, *A)], 0, None), ([(1, *A)], [(7, *A)], None, 0)]], 2, 2, 0.5, None))
    # score_iou 0: one shared pixel matches, a disjoint box does not; score_iou 1: the same box matches, a shifted one does not
    cases.append(Case("iou0", [[([(1, 0, 0, 9, 9), (2, 30, 0, 39, 9)], [(7, 9, 9, 18, 18), (8, 40, 0, 49, 9)], None, None)]], 2, 2, 0.0, None))
    cases.append(Case("iou1", [[([(1, 0, 0, 9, 9), (2, 30, 0, 39, 9)], [(7, 0, 0, 9, 9), (8, 30, 0, 39, 10)], None, None)]], 2, 2, 1.0, None))
    # int32 extremes, empty and inverted boxes on both sides: never eligible
    odd = [(ts.I32MIN, ts.I32MIN, ts.I32MAX, ts.I32MAX), (ts.I32MAX, ts.I32MAX, ts.I32MIN, ts.I32MIN), (5, 5, 4, 9), (ts.I32MAX - 1, 0, ts.I32MAX, ts.I32MAX),
           (0, 0, 0, 0)]
    cases.append(Case("extremes", [[([(k + 1, *b) for k, b in enumerate(odd)], [(k + 20, *b) for k, b in enumerate(odd[::-1])], None, None)] * 2],
                      5, 5, 0.3, None))
    return cases


def laid_out(case, layout):
    """-> (call, streams, steps, state0) of a designed case"""
    streams, steps = len(case.frames), len(case.frames[0])
    return lay_out(case.frames, case.gt_cap, case.out_cap, layout), streams, steps, (empty_state(streams) if case.state0 is None else case.state0)


# ---- sizes: every number of rows against every number of columns ----
@functools.lru_cache(maxsize=None)
def sweep_frames():
    """15 streams of two steps at caps 64: stream 3 a + b has (0, 1, 2, 63, 64)[a] labelled objects against (0, 1, 64)[b] reported tracks,
    boxes of side 20 .. 80 thrown into a square of 150 so that most pairs overlap; the second step shows the same ids with every box
    moved a little, in another order: continuity meets the search"""
    rng = np.random.default_rng(8100)

    def box():
        x, y, w, h = (int(v) for v in (rng.integers(0, 150), rng.integers(0, 150), rng.integers(20, 81), rng.integers(20, 81)))
        return (x, y, x + w - 1, y + h - 1)

    def moved(row):
        d = [int(v) for v in rng.integers(-6, 7, 4)]
        return (row[0], row[1] + d[0], row[2] + d[1], row[3] + d[0] + d[2] // 3, row[4] + d[1] + d[3] // 3)
    frames = []
    for g in (0, 1, 2, 63, 64):
        for h in (0, 1, 64):
            truths = [(int(o), *box()) for o in rng.choice(256, g, replace=False) + 1]
            hyps = [(int(k), *(truths[j][1:] if j < g and rng.random() < 0.5 else box())) for j, k in enumerate(rng.choice(5000, h, replace=False) + 1)]
            second = ([moved(truths[int(k)]) for k in rng.permutation(g)], [moved(hyps[int(k)]) for k in rng.permutation(h)], None, None)
            frames.append([(truths, hyps, None, None), second])
    return frames


def equal_frames():
    """64 labelled objects and 64 tracks at one box, every pair eligible with the same weight: 2080 rounds of the search; then the same
    tracks in reversed order, every pair kept by its id"""
    boxes, dets = asg.all_equal_scene()
    truths = [(i + 1, *dets[i]) for i in range(64)]
    hyps = [(101 + j, *boxes[j]) for j in range(64)]
    return [[(truths, hyps, None, None), (truths, hyps[::-1], None, None)]]


def staircase_frames():
    """tests/assign_support.py's staircase with the strips as labelled objects (rows, listed in descending length) and the tiles as tracks
    (columns): every search walks through all the columns assigned so far and the last augmenting path runs through all 64 columns; then
    the first 40 strips again over the tiles shifted by one place"""
    boxes, strips = asg.staircase_scene()
    truths = [(i + 1, *b) for i, b in enumerate(strips)]
    hyps = [(201 + j, *boxes[j]) for j in range(64)]
    return [[(truths, hyps, None, None), (truths[:40], hyps[1:] + hyps[:1], None, None)]]


# ---- seeded random clips ----
@functools.lru_cache(maxsize=None)
def drift_frames(streams, steps, seed=8200):
    """`streams` x `steps` small frames for the shape sweeps (at most 8 labelled objects and 6 tracks a frame): two to six objects that
    drift; the tracks are their boxes jittered under ids of their own, about a fifth missing, now and then two ids exchanged, a track
    without an object, a repeated row or a row of id 0; the order of both rows shuffled"""
    rng = np.random.default_rng(seed + 1000 * streams + steps)
    frames = []
    for s in range(streams):
        objects = [[int(rng.integers(0, 200)), int(rng.integers(0, 200)), int(rng.integers(20, 60)), int(rng.integers(20, 60))]
                   for _ in range(int(rng.integers(2, 7)))]
        ids = [int(v) for v in rng.choice(256, len(objects), replace=False) + 1]
        hid = [int(v) for v in rng.choice(900, len(objects), replace=False) + 1]
        clip = []
        for t in range(steps):
            for o in objects:
                o[0] += int(rng.integers(-5, 6))
                o[1] += int(rng.integers(-5, 6))
            if len(objects) > 1 and rng.random() < 0.2:
                a, b = (int(v) for v in rng.choice(len(objects), 2, replace=False))
                hid[a], hid[b] = hid[b], hid[a]
            truths = [(ids[k], o[0], o[1], o[0] + o[2] - 1, o[1] + o[3] - 1) for k, o in enumerate(objects)]
            hyps = [(hid[k], o[0] + int(rng.integers(-3, 4)), o[1] + int(rng.integers(-3, 4)), o[0] + o[2] - 1, o[1] + o[3] - 1)
                    for k, o in enumerate(objects) if rng.random() > 0.2][:5]
            if rng.random() < 0.2:
                hyps.append((1000 + t, 500, 500 + s, 540, 540))
            if rng.random() < 0.15:
                truths.append((truths[0][0], *truths[-1][1:]) if rng.random() < 0.5 else (0, *truths[0][1:]))
            clip.append(([truths[int(k)] for k in rng.permutation(len(truths))], [hyps[int(k)] for k in rng.permutation(len(hyps))], None, None))
        frames.append(clip)
    return frames


D_GT_CAP, D_OUT_CAP = 8, 6


def junk_state(streams, seed=8300, extremes=True):
    """states of random bytes; with `extremes` the first stream's counters at UINT64_MAX and every other entry of its present and tracked
    at INT32_MAX"""
    rng = np.random.default_rng(seed)
    st = np.frombuffer(rng.integers(0, 256, streams * STATE.itemsize, dtype=np.uint8).tobytes(), STATE).copy()
    if extremes:
        for name in COUNTERS:
            st[name][0] = U64MAX
        st["present"][0, ::2] = ts.I32MAX
        st["tracked"][0, ::2] = ts.I32MAX
    return st


def split_calls(run, call, streams, steps, gt_cap, out_cap, score_iou, state0):
    """`steps` calls of one step each on time-major arrays, the state carried -> the Result one call of `steps` steps must give"""
    state, parts = state0, []
    for t in range(steps):
        part = tuple(a[t * streams:(t + 1) * streams] for a in call)
        r = run(part, streams, 1, ts.TIME, gt_cap, out_cap, score_iou, state)
        assert r.rc == streams
        state = r.state
        parts.append(r)
    return Result(streams * steps, state, *(np.concatenate([getattr(p, name) for p in parts]) for name in ("match", "status")))


def per_cu():
    """the workgroups of the score kernel that a CU holds at once, the measure of the launcher's grid: the constant the launcher itself
    takes, read from csrc/yf_images_score.hip.h"""
    text = open(os.path.join(ROOT, "stm32h7-yolo_amd", "csrc", "yf_images_score.hip.h")).read()
    return int(re.search(r"\bkPerCuScore = (\d+)", text).group(1))


# ---- a tracker's output scored: the pan and crossing streams of tests/assign_support.py ----
SCORE_IOU, TRACKER = 0.5, asg.M_PARAMS


def clip_truth():
    """the labelled identities of `asg.crossing_frames`: stream 0 the faces P (id 1) and Q (id 2) that pass each other, stream 1 the
    neighbours A (id 1) and B (id 2) of the pan -> truth[s][t] = [(id, x1, y1, x2, y2), ...]"""
    cross, pan = [], []
    for t in range(asg.C_STEPS):
        px, qx = -150 + 40 * t + (3 if t % 3 == 0 else 0), 150 - 5 * t
        cross.append([(1, px, 0, px + 99, 99), (2, qx, 3, qx + 99, 102)])
        ax, bx = -33 * t, 58 - 33 * t
        pan.append([(1, ax, 0, ax + 99, 99), (2, bx, 0, bx + 99, 99)])
    truth = [cross, pan]
    for s, clip in enumerate(asg.crossing_frames()):
        assert all(sorted(r[1:] for r in truth[s][t]) == sorted(boxes) for t, (boxes, _) in enumerate(clip))
    return truth


def truth_arrays(truth, gt_cap, layout):
    """truth[s][t] -> (gt GT [n, gt_cap], gt_counts) of a call in `layout`"""
    frames = [[(rows, [], None, None) for rows in clip] for clip in truth]
    return lay_out(frames, gt_cap, 1, layout)[3:]


def tracked_on_host(frames, cap, gains, assign, out_cap=8, params=TRACKER):
    """the tracker's host build over a whole scene (tracker frames[s][t] = (boxes, count)), time-major -> ts.Result"""
    streams, steps = len(frames), len(frames[0])
    dets, counts = ts.lay_out(frames, cap, ts.TIME)
    return asg.host_run(dets, counts, streams, steps, ts.TIME, cap, tuple(params) + tuple(gains), assign, ms.empty_state(streams), out_cap)
