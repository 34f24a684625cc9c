"""What the tests of the tracker share (test_track_*): the record, state and info layouts as numpy dtypes, the designed sequences, the
seeded random sequences, the expectation of a call -- `ptq.track_step`, the plain-Python statement of csrc/yf_images_track.h, run stream by
stream and step by step over arrays whose every byte starts as a sentinel --, and the host build's prototypes with a runner that puts
guard bytes in front of and behind every array.

A sequence is `frames[s][t] = (boxes, count)`: the boxes (x1, y1, x2, y2) of stream s at step t in the order they lie, and the frame's
count (None: len(boxes)).  `lay_out` makes the record and count arrays of a call from it in either layout; places of a row that hold no box
are 0xA5 bytes (and count, if the count says so).  The conf of a record is kept as its 32 bits (RAW), so that every byte travels exactly."""
import ctypes
import functools
import importlib
import os
import re
from collections import namedtuple

import numpy as np

from conftest import ROOT
from images_support import host_lib


def _mod(name):
    return importlib.import_module("stm32h7-yolo_amd." + name)


RAW = np.dtype([("frame", "<i4"), ("anchor", "u1"), ("row", "u1"), ("col", "u1"), ("q_conf", "i1"), ("conf", "<u4"), ("x1", "<i4"),
                ("y1", "<i4"), ("x2", "<i4"), ("y2", "<i4")])
SLOT = np.dtype([("id", "<u4"), ("hits", "<i4"), ("misses", "<i4"), ("age", "<i4"), ("det", RAW)])
STATE = np.dtype([("issued", "<u4"), ("reserved", "<u4"), ("slot", SLOT, (64,))])
INFO = np.dtype([("id", "<u4"), ("hits", "<i4"), ("misses", "<i4"), ("age", "<i4")])
assert (RAW.itemsize, SLOT.itemsize, STATE.itemsize, INFO.itemsize) == (28, 44, 2824, 16)
TIME, STREAM = 0, 1
LAYOUTS = (TIME, STREAM)
SENTINEL32 = -1515870811                    # 0xA5A5A5A5
GUARD = 64                                  # bytes in front of and behind every array a call may write
I32MIN, I32MAX = -2 ** 31, 2 ** 31 - 1
DEFAULT = (0.3, 1, 5)


class Params(ctypes.Structure):
    _fields_ = [("match_iou", ctypes.c_double), ("min_hits", ctypes.c_int32), ("max_misses", ctypes.c_int32)]


Case = namedtuple("Case", "name frames cap out_cap params state0")


def frame_of(s, t, streams, steps, layout):
    return t * streams + s if layout == TIME else s * steps + t


def conf_bits(j):
    return int(np.float32(0.99 - 0.005 * j).view(np.uint32))


def lay_out(frames, cap, layout):
    """frames[s][t] = (boxes, count) -> (dets RAW [n, cap], counts int32 [n]) of a call in `layout`"""
    streams, steps = len(frames), len(frames[0]) if frames else 0
    n = streams * steps
    dets = np.frombuffer(bytes([0xA5]) * (max(n, 1) * cap * 28), RAW).reshape(max(n, 1), cap).copy()
    counts = np.zeros(max(n, 1), np.int32)
    for s in range(streams):
        assert len(frames[s]) == steps
        for t in range(steps):
            boxes, count = frames[s][t]
            f = frame_of(s, t, streams, steps, layout)
            assert len(boxes) <= cap
            counts[f] = len(boxes) if count is None else count
            for j, box in enumerate(boxes):
                dets[f, j] = (-9, s % 3, t % 7, j % 7, 5, conf_bits(j), *box)
    return dets, counts


def empty_state(streams):
    return np.zeros(max(streams, 1), STATE)


def state_to_py(rec):
    return {"issued": int(rec["issued"]), "reserved": int(rec["reserved"]), "slots": [list(s) for s in rec["slot"].tolist()]}


def py_to_state(st):
    rec = np.zeros((), STATE)
    rec["issued"], rec["reserved"] = st["issued"], st["reserved"]
    for k, (i, hits, misses, age, det) in enumerate(st["slots"]):
        rec["slot"][k] = (i, hits, misses, age, tuple(int(v) for v in det))
    return rec


def sentinels(n, out_cap):
    """out RAW [n, out_cap], info INFO [n, out_cap], out_counts int32 [n], status int32 [n], every byte 0xA5"""
    n = max(n, 1)
    return (np.frombuffer(bytes([0xA5]) * (n * out_cap * 28), RAW).reshape(n, out_cap).copy(),
            np.frombuffer(bytes([0xA5]) * (n * out_cap * 16), INFO).reshape(n, out_cap).copy(),
            np.full(n, SENTINEL32, np.int32), np.full(n, SENTINEL32, np.int32))


Result = namedtuple("Result", "rc state out info out_counts status")


def same(a, b):
    """two results equal in every byte: the return value, the whole state, records, infos, counts and status"""
    return a.rc == b.rc and all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:]))


def expected(dets, counts, streams, steps, layout, cap, params, state0, out_cap, stats=None):
    """the call by the Python statement -> Result; nothing of the inputs is changed"""
    ptq = _mod("ptq")
    n = streams * steps
    out, info, out_counts, status = sentinels(n, out_cap)
    state = state0.copy()
    for s in range(streams):
        st = state_to_py(state[s])
        for t in range(steps):
            f = frame_of(s, t, streams, steps, layout)
            st, emitted, bits = ptq.track_step(st, dets[f].tolist(), params, count=int(counts[f]), cap=cap, frame=f, stats=stats)
            out_counts[f], status[f] = len(emitted), bits
            for r, (rec, inf) in enumerate(emitted[:out_cap]):
                out[f, r], info[f, r] = rec, inf
        state[s] = py_to_state(st)
    return Result(n, state, out, info, out_counts, status)


# ---- the host build ----
@functools.lru_cache(maxsize=None)
def track_host():
    """libyf_images_host.so with the prototypes of csrc/yf_images_track.h's host build added"""
    lib = host_lib()
    vp, ci, cl = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    lib.yf_images_track_host.restype = cl
    lib.yf_images_track_host.argtypes = [vp, vp, cl, cl, ci, ci, vp, vp, vp, vp, vp, ci, vp, vp]
    lib.yfi_track_check_host.restype = ci
    lib.yfi_track_check_host.argtypes = [vp, vp, cl, cl, ci, ci, vp, vp, vp, vp, vp, ci, vp, ctypes.c_char_p, ci]
    lib.yf_images_track_state_bytes_host.restype = ctypes.c_size_t
    lib.yf_images_track_state_bytes_host.argtypes = [cl]
    return lib


def guarded(interior):
    """a copy of `interior` (any array) with GUARD bytes of 0xA5 on both sides -> (whole uint8 buffer, byte offset of the interior)"""
    whole = np.full(interior.nbytes + 2 * GUARD, 0xA5, np.uint8)
    whole[GUARD:GUARD + interior.nbytes] = np.ascontiguousarray(interior).view(np.uint8).reshape(-1)
    return whole, GUARD


def guards_intact(whole):
    return bool((whole[:GUARD] == 0xA5).all() and (whole[-GUARD:] == 0xA5).all())


def run_with(call, dets, counts, streams, steps, layout, cap, params, state0, out_cap, with_status=True, upload=None, download=None):
    """`call(dets, counts, streams, steps, layout, cap, params, state, out, info, out_counts, out_cap, status)` on addresses, every written
    array between guard bytes -> Result.  upload / download: the buffers' way to the device and back (the GPU tests)."""
    n = streams * steps
    arrays = [state0[:max(streams, 1)].copy(), *sentinels(n, out_cap)]
    bufs = [guarded(a)[0] for a in arrays]
    ins = [np.ascontiguousarray(dets), np.ascontiguousarray(counts)]
    if upload is not None:
        bufs, ins = [upload(b) for b in bufs], [upload(a.view(np.uint8).reshape(-1)) for a in ins]
        addr = lambda b: b.data_ptr()
    else:
        addr = lambda b: b.ctypes.data
    p = [addr(b) + GUARD for b in bufs]
    rc = call(addr(ins[0]), addr(ins[1]), streams, steps, layout, cap, params, p[0], p[1], p[2], p[3], out_cap, p[4] if with_status else None)
    if download is not None:
        bufs = [download(b) for b in bufs]
    assert all(guards_intact(b) for b in bufs), "a byte outside an array was written"
    got = [b[GUARD:-GUARD].view(a.dtype).reshape(a.shape) for a, b in zip(arrays, bufs)]
    return Result(rc, *got)


def host_run(dets, counts, streams, steps, layout, cap, params, state0, out_cap, with_status=True):
    lib = track_host()

    def call(d, c, streams, steps, layout, cap, params, state, out, info, oc, out_cap, status):
        p = Params(*params)
        return lib.yf_images_track_host(d, c, streams, steps, layout, cap, ctypes.byref(p), state, out, info, oc, out_cap, status, None)
    return run_with(call, dets, counts, streams, steps, layout, cap, params, state0, out_cap, with_status)


def host_check(dets=8, counts=8, streams=2, steps=3, layout=TIME, cap=8, params=DEFAULT, state=8, out=8, info=8, out_counts=8, out_cap=4,
               status=0):
    """yfi_track_check on made-up addresses -> the text of the first fault, '' for none"""
    text = ctypes.create_string_buffer(256)
    p = None if params is None else ctypes.byref(Params(*params))
    rc = track_host().yfi_track_check_host(dets, counts, streams, steps, layout, cap, p, state, out, info, out_counts, out_cap, status, text, 256)
    assert rc == (text.value != b"")
    return text.value.decode()


def by_frame(r, streams, steps, layout):
    """a result's per-frame arrays in (stream, step) order, with the frame fields of the records taken out"""
    order = [frame_of(s, t, streams, steps, layout) for s in range(streams) for t in range(steps)]
    out = r.out[order].copy()
    written = np.arange(out.shape[1])[None, :] < np.minimum(r.out_counts[order], out.shape[1])[:, None]
    assert (out["frame"][written] == np.repeat(order, out.shape[1]).reshape(out.shape)[written]).all()
    out["frame"] = 0
    return out.tobytes(), r.info[order].tobytes(), r.out_counts[order].tobytes(), r.status[order].tobytes(), r.state.tobytes()


def split_calls(run, dets, counts, streams, steps, cap, params, state0, out_cap):
    """`steps` calls of one step each on time-major records, the state carried -> the Result one call of `steps` steps must give"""
    state, parts = state0, []
    for t in range(steps):
        r = run(dets[t * streams:(t + 1) * streams], counts[t * streams:(t + 1) * streams], streams, 1, TIME, cap, params, state, out_cap)
        assert r.rc == streams
        written = np.arange(out_cap)[None, :] < r.out_counts[:, None]
        r.out["frame"][written] += t * streams                                       # a call numbers its frames from 0
        state = r.state
        parts.append(r)
    return Result(streams * steps, state, *(np.concatenate([getattr(p, name) for p in parts]) for name in ("out", "info", "out_counts", "status")))


# the faults every entry refuses, as keyword changes of `host_check`'s valid call, with a part of the text
FAULTS = [(dict(streams=-1), "streams and steps"), (dict(steps=-1), "streams and steps"), (dict(streams=2 ** 31, steps=1), "streams * steps"),
          (dict(streams=65536, steps=32768), "streams * steps"), (dict(layout=2), "layout"), (dict(layout=-1), "layout"),
          (dict(cap=0), "cap must"), (dict(cap=1201), "cap must"), (dict(out_cap=0), "out_cap"), (dict(out_cap=-4), "out_cap"),
          (dict(params=None), "params is NULL"), (dict(params=(float("nan"), 1, 5)), "match_iou is NaN"),
          (dict(params=(0.3, 0, 5)), "min_hits"), (dict(params=(0.3, 1, -1)), "max_misses"),
          (dict(dets=0), "is NULL"), (dict(counts=0), "is NULL"), (dict(state=0), "is NULL"), (dict(out=0), "is NULL"),
          (dict(info=0), "is NULL"), (dict(out_counts=0), "is NULL"),
          (dict(dets=10), "4-byte aligned"), (dict(counts=9), "4-byte aligned"), (dict(out=6), "4-byte aligned"), (dict(info=7), "4-byte aligned"),
          (dict(out_counts=5), "4-byte aligned"), (dict(status=6), "4-byte aligned"), (dict(state=12), "8-byte aligned")]


# ---- the designed sequences ----
def _crafted(slots, issued=0, reserved=0):
    """a state of one stream: slots = {k: (id, hits, misses, age, box)}"""
    st = empty_state(1)
    st["issued"], st["reserved"] = issued, reserved
    for k, (i, hits, misses, age, box) in slots.items():
        st["slot"][0, k] = (i, hits, misses, age, (7, 1, 2, 3, 4, conf_bits(k), *box))
    return st


def _grid(k, side=10, pitch=12, per_row=10):
    """box k of a grid of disjoint boxes"""
    x, y = (k % per_row) * pitch, (k // per_row) * pitch
    return (x, y, x + side - 1, y + side - 1)


@functools.lru_cache(maxsize=None)
def designed():
    """the designed sequences, each at the smallest size that can go wrong -> [Case]"""
    A, B, C = (10, 10, 29, 29), (100, 10, 119, 39), (60, 60, 79, 79)
    cases = []
    # birth, confirmation at min_hits = 3, hold-over for max_misses = 2 frames, removal on the next miss; B stays, so A's slot 0 is the
    # lowest free one when C appears in the step that removes A: C gets slot 0 and id 3 (2 is B's; A's id 1 is not reissued)
    life = [([A, B], None), ([A, B], None), ([B, A], None), ([B], None), ([B], None), ([B, C], None), ([C, B], None), ([B, C], None), ([], None)]
    cases.append(Case("lifecycle", [life], 4, 4, (0.3, 3, 2), None))
    # two tracks and two detections, mirror-symmetric: all four pairs have the same IoU; the tie rule gives detection 0 to slot 0
    T0, T1, D0, D1 = (0, 0, 9, 9), (12, 0, 21, 9), (6, 2, 15, 11), (6, -2, 15, 7)
    # (and again, mirrored the other way, with the detections in the other order)
    F0, F1 = (2, 0, 11, 9), (10, 0, 19, 9)
    cases.append(Case("tie", [[([T0, T1], None), ([D0, D1], None), ([F1, F0], None)]], 3, 3, (0.1, 1, 1), None))
    # the global greedy and a per-detection greedy differ: detection 0 prefers slot 0 (0.33 against 0.25 with slot 1), but detection 1
    # and slot 0 are the best pair of all (0.82), so detection 0 gets slot 1
    G0, G1, E0, E1 = (0, 0, 19, 9), (22, 0, 41, 9), (10, 0, 29, 9), (2, 0, 21, 9)
    cases.append(Case("global_greedy", [[([G0, G1], None), ([E0, E1], None)]], 2, 2, (0.2, 1, 1), None))
    # 64 full slots and one more detection: 63 of them seen again, a new one in front of them finds no slot
    full = [_grid(k) for k in range(64)]
    cases.append(Case("full", [[(full, None), ([(500, 500, 520, 520)] + full[:63], None), (full[:5], None)]], 70, 64, (0.3, 1, 3), None))
    # counts above cap (all cap records count), above 64 (64 count, bit 0), below 0 and 0 over places that hold records
    many = [_grid(k, side=6, pitch=7, per_row=9) for k in range(70)]
    cases.append(Case("counts", [[(many[:10], 15), (many[:10], -3), (many[:10], 0), (many[:10], 7)],
                                 [(many[10:20], 10), (many[10:20], 2 ** 31 - 1), (many[10:20], I32MIN), (many[10:20], 10)]], 10, 12, (0.3, 1, 1), None))
    cases.append(Case("counts64", [[(many, None), (many[:66], 66), (many[::-1], 65)]], 70, 64, (0.3, 1, 1), None))
    # out_cap below the emitted count: five tracks, two places
    cases.append(Case("out_cap", [[(full[:5], None), (full[1:5], None)]], 5, 2, (0.3, 1, 2), None))
    # int32 extremes, empty and inverted boxes: the improper ones are born, never match and age out
    odd = [(I32MIN, I32MIN, I32MAX, I32MAX), (I32MAX, I32MAX, I32MIN, I32MIN), (I32MIN, 0, I32MIN, 0), (I32MAX, 5, I32MAX, 5),
           (5, 5, 4, 9), (5, 5, 9, 4), (9, 9, 0, 0), (0, 0, 0, 0), (I32MIN, I32MIN, I32MIN + 1, I32MIN + 1), (I32MAX - 1, 0, I32MAX, I32MAX)]
    cases.append(Case("extremes", [[(odd, None), (odd, None), (odd[::-1], None), ([], None), ([], None)]], 10, 64, (0.3, 1, 1), None))
    # match_iou 0: one shared pixel matches, a disjoint box does not; match_iou 1: the same box matches, a shifted one does not
    cases.append(Case("iou0", [[([(0, 0, 9, 9), (30, 0, 39, 9)], None), ([(9, 9, 18, 18), (40, 0, 49, 9)], None)]], 2, 8, (0.0, 1, 0), None))
    cases.append(Case("iou1", [[([(0, 0, 9, 9), (30, 0, 39, 9)], None), ([(0, 0, 9, 9), (30, 0, 39, 10)], None)]], 2, 8, (1.0, 1, 0), None))
    # issued about to wrap: the ids 0xFFFFFFFF and 1 (0 is skipped), emitted in unsigned order
    cases.append(Case("wrap", [[([A, B, C], None), ([A, B, C], None)]], 3, 8, (0.3, 1, 1), _crafted({}, issued=0xFFFFFFFE, reserved=0xDEADBEEF)))
    cases.append(Case("wrap_at_max", [[([A, B], None)]], 3, 8, (0.3, 1, 1), _crafted({5: (9, 1, 0, 1, C)}, issued=0xFFFFFFFF)))
    # hits and age at INT32_MAX stay there; misses at INT32_MAX too (and the track goes)
    sat = _crafted({0: (4, I32MAX, 0, I32MAX, A), 1: (5, I32MAX - 1, 0, I32MAX - 1, B), 2: (6, 3, I32MAX, I32MAX, C)}, issued=6)
    cases.append(Case("saturate", [[([A, B], None), ([A, B], None)]], 2, 8, (0.3, 1, 5), sat))
    cases.append(Case("saturate_kept", [[([A], None)]], 2, 8, (0.3, 1, I32MAX), sat))
    # misses negative (counts up from there) and above max_misses (matched: back to 0; missed: removed); hits negative: not emitted
    neg = _crafted({0: (4, 2, -5, 9, A), 1: (5, 2, 100, 9, B), 2: (6, 2, 100, 9, C), 3: (7, -4, 0, 2, (200, 200, 220, 220))}, issued=3)
    cases.append(Case("misses", [[([B], None), ([B], None), ([], None)]], 2, 8, (0.3, 1, 2), neg))
    # a free slot (id 0) whose other bytes are not zero stays as it is until a track is born there; equal ids come out by slot
    dirty = _crafted({0: (0, 5, 6, 7, A), 2: (9, 1, 0, 1, B), 3: (9, 1, 0, 1, C), 4: (0, -1, -1, -1, (1, 2, 3, 4))}, issued=20)
    cases.append(Case("dirty", [[([C, B], None), ([(300, 300, 310, 310), B, C], None)]], 3, 8, (0.3, 1, 2), dirty))
    # a state of random bytes, two streams; every id of the second made non-zero: its table is full
    rng = np.random.default_rng(5700)
    junk = np.frombuffer(rng.integers(0, 256, 2 * STATE.itemsize, dtype=np.uint8).tobytes(), STATE).copy()
    junk["slot"]["id"][1] |= 1
    boxes = [tuple(int(junk["slot"]["det"][s, k][e]) for e in ("x1", "y1", "x2", "y2")) for s in (0, 1) for k in (3, 17)]
    cases.append(Case("junk", [[(boxes + [A], None), (boxes[:2], None), ([A], None)], [([B] + boxes, None), (boxes[2:], None), ([], None)]],
                      6, 64, (0.3, 2, 1), junk))
    return cases


def laid_out(case, layout):
    """-> (dets, counts, streams, steps, state0) of a designed case"""
    streams, steps = len(case.frames), len(case.frames[0])
    dets, counts = lay_out(case.frames, case.cap, layout)
    return dets, counts, streams, steps, (empty_state(streams) if case.state0 is None else case.state0)


# ---- the seeded random sequences ----
RANDOM_SEED = 5800
R_STREAMS, R_STEPS, R_CAP, R_OUT_CAP = 3, 40, 70, 48
R_PARAMS = (0.3, 2, 3)


@functools.lru_cache(maxsize=None)
def random_frames(seed=RANDOM_SEED):
    """3 streams x 40 steps, up to 70 records per frame: boxes that drift by a few pixels, drop out for a frame or for good, cross each
    other and appear; stream 1 is crowded for some steps (its table fills up); now and then a mirror-symmetric pair of boxes is
    followed by one box between them (equal IoUs: a tie)"""
    rng = np.random.default_rng(seed)
    frames = []
    for s in range(R_STREAMS):
        objects = []                                            # [x, y, w, h, dx, dy]

        def spawn():
            objects.append([int(rng.integers(0, 380)), int(rng.integers(0, 330)), int(rng.integers(8, 60)), int(rng.integers(8, 60)),
                            int(rng.integers(-4, 5)), int(rng.integers(-4, 5))])
        for _ in range(int(rng.integers(3, 9))):
            spawn()
        clip = []
        for t in range(R_STEPS):
            for o in objects:
                o[0] += o[4] + int(rng.integers(-1, 2))
                o[1] += o[5] + int(rng.integers(-1, 2))
            objects[:] = [o for o in objects if rng.random() > 0.04]                    # gone for good
            if rng.random() < 0.35:
                spawn()
            boxes = [(o[0], o[1], o[0] + o[2] - 1, o[1] + o[3] - 1) for o in objects if rng.random() > 0.15]      # ... or for a frame
            if s == 1 and 12 <= t < 20:                         # the crowd: 70 small boxes, every step a few new ones
                crowd = [_grid(k, side=6, pitch=7, per_row=9) for k in range(70)]
                for k in rng.choice(70, 6, replace=False):
                    x, y = 600 + 9 * int(k), 400 + 9 * t
                    crowd[int(k)] = (x, y, x + 5, y + 5)
                boxes = (crowd + boxes)[:R_CAP]
            if t % 10 == 4:
                boxes = [(1000, 0, 1009, 9), (1008, 0, 1017, 9)] + boxes
            elif t % 10 == 5:
                boxes = [(1004, 0, 1013, 9)] + boxes                   # IoU 60 / 140 with both
            order = rng.permutation(len(boxes))
            clip.append(([boxes[int(k)] for k in order][:R_CAP], None))
        frames.append(clip)
    return frames


@functools.lru_cache(maxsize=None)
def drift_frames(streams, steps, seed=5900):
    """`streams` x `steps` small frames for the shape sweeps: two to five boxes per stream that drift and drop out, one that appears"""
    rng = np.random.default_rng(seed + 1000 * streams + steps)
    frames = []
    for s in range(streams):
        objects = [[int(rng.integers(0, 300)), int(rng.integers(0, 300)), int(rng.integers(10, 50)), int(rng.integers(10, 50))]
                   for _ in range(int(rng.integers(2, 6)))]
        clip = []
        for t in range(steps):
            for o in objects:
                o[0] += int(rng.integers(-5, 6))
                o[1] += int(rng.integers(-5, 6))
            if t == steps // 2:
                objects.append([400, 400 + s, 20, 20])
            clip.append(([(o[0], o[1], o[0] + o[2] - 1, o[1] + o[3] - 1) for o in objects if rng.random() > 0.25], None))
        frames.append(clip)
    return frames


def per_cu(kernel):
    """the workgroups of the 'Track', 'Motion' or 'Assign' kernel that a CU holds at once, the measure of the launcher's grid: the constant
    the launcher itself takes, read from csrc/yf_images_step.hip.h"""
    text = open(os.path.join(ROOT, "stm32h7-yolo_amd", "csrc", "yf_images_step.hip.h")).read()
    return int(re.search(r"\bkPerCu%s = (\d+)" % kernel, text).group(1))


def beyond_the_grid(device, host, workgroups, params, state0):
    """three streams more than the launch has workgroups, so that some workgroups take a second stream (state reloaded into the registers,
    the assign kernel's table reused), two steps at cap 4 with 0 to 4 records a frame; then the same again in the other layout on the
    state the first call left, part occupied and part empty: `device` against `host`, both `host_run`'s signature, in every byte"""
    streams, steps, cap, out_cap = workgroups + 3, 2, 4, 4
    frames = [[(boxes[:cap], None) for boxes, _ in clip] for clip in drift_frames(streams, steps)]
    state = state0(streams)
    for layout in LAYOUTS:
        dets, counts = lay_out(frames, cap, layout)
        want = host(dets, counts, streams, steps, layout, cap, params, state, out_cap)
        got = device(dets, counts, streams, steps, layout, cap, params, state, out_cap)
        assert want.rc == streams * steps and same(got, want), layout
        assert (want.state["issued"] > 0).mean() > 0.9 and (want.out_counts > 0).any()             # tracks nearly everywhere
        state = got.state
    return got


@functools.lru_cache(maxsize=None)
def random_call(layout=TIME):
    """-> (dets, counts, expectation) of the random sequences in one call; the statement's counters must all have counted"""
    dets, counts = lay_out(random_frames(), R_CAP, layout)
    stats = {}
    want = expected(dets, counts, R_STREAMS, R_STEPS, layout, R_CAP, R_PARAMS, empty_state(R_STREAMS), R_OUT_CAP, stats)
    for name in ("matches", "births", "removals", "held", "ties", "dropped"):
        assert stats.get(name, 0) >= 1, (name, stats)
    assert (counts > 64).any() and (want.status == 3).any() and (want.out_counts > R_OUT_CAP).any(), stats
    for a in (dets, counts):
        a.setflags(write=False)
    return dets, counts, want
