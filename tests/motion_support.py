"""What the tests of the tracker with a motion model share (test_track_motion_*): the state layout as numpy dtypes, the scenario of a moving
box with a gap in its detections and its expected results, seeded random sequences of moving boxes, the expectation of a call --
`ptq.track_motion_step`, the plain-Python statement of csrc/yf_images_motion.h, over arrays whose every byte starts as a sentinel --, and the
host build's prototypes.  The record layouts, the sequences' form (`frames[s][t] = (boxes, count)`), the guarded runner and the designed
sequences are tests/track_support.py's.

A call's params here are the seven numbers (match_iou, min_hits, max_misses, alpha, beta, damp, smooth)."""
import ctypes
import functools

import numpy as np

import track_support as ts

MSLOT = np.dtype([("base", ts.SLOT), ("pad", "<i4"), ("pos", "<i8", (4,)), ("vel", "<i8", (4,))])
MSTATE = np.dtype([("issued", "<u4"), ("reserved", "<u4"), ("slot", MSLOT, (64,))])
assert (MSLOT.itemsize, MSTATE.itemsize) == (112, 7176)
I64MIN, I64MAX = -2 ** 63, 2 ** 63 - 1
LIMIT = 2 ** 40
SUGGESTED = (192, 128, 256)                 # (alpha, beta, damp): the library's suggestion
BASE_LIKE = (256, 0, 256)                   # the base tracker
DIFFERENCE = (256, 256, 256)                # predicts with the last frame-to-frame difference
GAIN_SETS = (BASE_LIKE, DIFFERENCE, SUGGESTED)


class Params(ctypes.Structure):
    _fields_ = [("base", ts.Params), ("alpha", ctypes.c_int32), ("beta", ctypes.c_int32), ("damp", ctypes.c_int32), ("smooth", ctypes.c_int32)]


assert ctypes.sizeof(Params) == 32


def c_params(params):
    return Params(ts.Params(*params[:3]), *params[3:7])


def empty_state(streams):
    return np.zeros(max(streams, 1), MSTATE)


def lift(state0):
    """a base tracker's state as this tracker's: every slot's base as it is, pos = 256 * its box, vel = 0, pad = 0"""
    st = empty_state(len(state0))
    st["issued"], st["reserved"] = state0["issued"], state0["reserved"]
    st["slot"]["base"] = state0["slot"]
    for e, name in enumerate(("x1", "y1", "x2", "y2")):
        st["slot"]["pos"][..., e] = 256 * state0["slot"]["det"][name].astype(np.int64)
    return st


def state_to_py(rec):
    return {"issued": int(rec["issued"]), "reserved": int(rec["reserved"]),
            "slots": [[*base, pad, list(pos), list(vel)] for base, pad, pos, vel in rec["slot"].tolist()]}


def py_to_state(st):
    rec = np.zeros((), MSTATE)
    rec["issued"], rec["reserved"] = st["issued"], st["reserved"]
    for k, (i, hits, misses, age, det, pad, pos, vel) in enumerate(st["slots"]):
        rec["slot"][k] = ((i, hits, misses, age, tuple(int(v) for v in det)), pad, tuple(pos), tuple(vel))
    return rec


def expected(dets, counts, streams, steps, layout, cap, params, state0, out_cap, stats=None):
    """the call by the Python statement -> ts.Result; nothing of the inputs is changed"""
    ptq = ts._mod("ptq")
    n = streams * steps
    out, info, out_counts, status = ts.sentinels(n, out_cap)
    state = state0.copy()
    for s in range(streams):
        st = state_to_py(state[s])
        for t in range(steps):
            f = ts.frame_of(s, t, streams, steps, layout)
            st, emitted, bits = ptq.track_motion_step(st, dets[f].tolist(), params, count=int(counts[f]), cap=cap, frame=f, stats=stats)
            out_counts[f], status[f] = len(emitted), bits
            for r, (rec, inf) in enumerate(emitted[:out_cap]):
                out[f, r], info[f, r] = rec, inf
        state[s] = py_to_state(st)
    return ts.Result(n, state, out, info, out_counts, status)


# ---- the host build ----
@functools.lru_cache(maxsize=None)
def motion_host():
    """libyf_images_host.so with the prototypes of csrc/yf_images_motion.h's host build added"""
    lib = ts.track_host()
    vp, ci, cl, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_int64
    lib.yf_images_track_motion_host.restype = cl
    lib.yf_images_track_motion_host.argtypes = [vp, vp, cl, cl, ci, ci, vp, vp, vp, vp, vp, ci, vp, vp]
    lib.yfi_motion_check_host.restype = ci
    lib.yfi_motion_check_host.argtypes = [vp, vp, cl, cl, ci, ci, vp, vp, vp, vp, vp, ci, vp, ctypes.c_char_p, ci]
    lib.yf_images_track_motion_state_bytes_host.restype = ctypes.c_size_t
    lib.yf_images_track_motion_state_bytes_host.argtypes = [cl]
    lib.yfi_motion_mul_host.restype, lib.yfi_motion_mul_host.argtypes = i64, [ctypes.c_int32, i64]
    lib.yfi_motion_box_host.restype, lib.yfi_motion_box_host.argtypes = ctypes.c_int32, [i64]
    lib.yfi_motion_sat_host.restype, lib.yfi_motion_sat_host.argtypes = i64, [i64]
    return lib


def host_run(dets, counts, streams, steps, layout, cap, params, state0, out_cap, with_status=True):
    lib = motion_host()

    def call(d, c, streams, steps, layout, cap, params, state, out, info, oc, out_cap, status):
        p = c_params(params)
        return lib.yf_images_track_motion_host(d, c, streams, steps, layout, cap, ctypes.byref(p), state, out, info, oc, out_cap, status, None)
    return ts.run_with(call, dets, counts, streams, steps, layout, cap, params, state0, out_cap, with_status)


VALID = dict(dets=8, counts=8, streams=2, steps=3, layout=ts.TIME, cap=8, params=ts.DEFAULT + SUGGESTED + (0,), state=8, out=8, info=8,
             out_counts=8, out_cap=4, status=0)


def host_check(**kw):
    """yfi_motion_check on made-up addresses -> the text of the first fault, '' for none"""
    a = dict(VALID, **kw)
    text = ctypes.create_string_buffer(256)
    p = None if a["params"] is None else ctypes.byref(c_params(a["params"]))
    rc = motion_host().yfi_motion_check_host(a["dets"], a["counts"], a["streams"], a["steps"], a["layout"], a["cap"], p, a["state"], a["out"],
                                             a["info"], a["out_counts"], a["out_cap"], a["status"], text, 256)
    assert rc == (text.value != b"")
    return text.value.decode()


def _faults():
    """ts.FAULTS with their params made seven numbers, then the refusals of the gains"""
    faults = []
    for kw, text in ts.FAULTS:
        if kw.get("params") is not None:
            kw = dict(kw, params=tuple(kw["params"]) + SUGGESTED + (0,))
        faults.append((kw, text))
    for at, name in ((3, "alpha"), (4, "beta"), (5, "damp")):
        for bad in (-1, 257, ts.I32MIN, ts.I32MAX):
            p = list(VALID["params"])
            p[at] = bad
            faults.append((dict(params=tuple(p)), name + " must be in [0, 256]"))
    for bad in (-1, 2, ts.I32MAX):
        faults.append((dict(params=VALID["params"][:6] + (bad,)), "smooth must be 0 or 1"))
    return faults


FAULTS = _faults()


# ---- the scenario: a box of 40 x 50 that moves (12, 4) pixels per frame, not detected at steps 6, 7 and 8 ----
S_STEPS, S_CAP, S_GAP, S_BASE = 12, 4, (6, 7, 8), (0.3, 1, 5)


def s_box(t):
    return (10 + 12 * t, 20 + 4 * t, 49 + 12 * t, 69 + 4 * t)


def scenario():
    """-> frames[1][12] of the scenario"""
    return [[([] if t in S_GAP else [s_box(t)], None) for t in range(S_STEPS)]]


# per gains: the id of the track that carries the detection per step (None: no detection), and the held-over boxes at steps 6, 7, 8
S_EXPECTED = {
    BASE_LIKE: ([1] * 6 + [None] * 3 + [2] * 3, [(70, 40, 109, 89)] * 3),
    DIFFERENCE: ([1] * 6 + [None] * 3 + [1] * 3, [(82, 44, 121, 93), (94, 48, 133, 97), (106, 52, 145, 101)]),
    SUGGESTED: ([1] * 6 + [None] * 3 + [1] * 3, [(83, 44, 122, 93), (95, 48, 134, 97), (107, 52, 146, 101)]),
}


def boxes_of(r, f):
    """the (id, x1, y1, x2, y2, misses) of frame f of a result"""
    k = int(r.out_counts[f])
    return [(int(i["id"]), int(d["x1"]), int(d["y1"]), int(d["x2"]), int(d["y2"]), int(i["misses"])) for d, i in zip(r.out[f, :k], r.info[f, :k])]


# ---- seeded random sequences: 5 streams x 7 steps, up to 6 records ----
R_STREAMS, R_STEPS, R_CAP, R_OUT_CAP = 5, 7, 6, 5
R_BASE = (0.3, 1, 2)
R_GAINS = (SUGGESTED + (0,), SUGGESTED + (1,), DIFFERENCE + (0,), (128, 64, 200, 1), (256, 13, 0, 0), (0, 256, 255, 1), (77, 201, 128, 0))


@functools.lru_cache(maxsize=None)
def random_frames(seed=6100):
    """boxes with a velocity of their own (up to 9 pixels per step, some fast enough to lose a track without a motion model) and some
    jitter, that drop out for a step or two, leave, and appear; stream 3 holds more boxes than a frame has places for a while"""
    rng = np.random.default_rng(seed)
    frames = []
    for s in range(R_STREAMS):
        objects = []

        def spawn():
            objects.append([int(rng.integers(-20, 300)), int(rng.integers(-20, 300)), int(rng.integers(8, 50)), int(rng.integers(8, 50)),
                            int(rng.integers(-9, 10)), int(rng.integers(-9, 10))])
        for _ in range(int(rng.integers(2, 6)) + (3 if s == 3 else 0)):
            spawn()
        clip = []
        for t in range(R_STEPS):
            for o in objects:
                o[0] += o[4] + int(rng.integers(-1, 2))
                o[1] += o[5] + int(rng.integers(-1, 2))
            objects[:] = [o for o in objects if rng.random() > 0.05]
            if rng.random() < 0.3:
                spawn()
            boxes = [(o[0], o[1], o[0] + o[2] - 1, o[1] + o[3] - 1) for o in objects if rng.random() > 0.3]
            order = rng.permutation(len(boxes))
            boxes = [boxes[int(k)] for k in order]
            clip.append((boxes[:R_CAP], len(boxes)))               # a count above cap where the stream is crowded
        frames.append(clip)
    return frames


@functools.lru_cache(maxsize=None)
def random_call(layout, gains):
    """-> (dets, counts, expectation) of the random sequences in one call at R_BASE + gains"""
    dets, counts = ts.lay_out(random_frames(), R_CAP, layout)
    want = expected(dets, counts, R_STREAMS, R_STEPS, layout, R_CAP, R_BASE + tuple(gains), empty_state(R_STREAMS), R_OUT_CAP)
    for a in (dets, counts):
        a.setflags(write=False)
    return dets, counts, want


def junk_state(streams, seed=6200, full=()):
    """states of random bytes; the streams in `full` with every id non-zero"""
    rng = np.random.default_rng(seed)
    st = np.frombuffer(rng.integers(0, 256, streams * MSTATE.itemsize, dtype=np.uint8).tobytes(), MSTATE).copy()
    for s in full:
        st["slot"]["base"]["id"][s] |= 1
    return st


def predicted_box(state, s, k):
    """the box slot k of stream s will be matched by at the next step: a record there meets whatever the slot's bytes hold"""
    ptq = ts._mod("ptq")
    slot = state["slot"][s, k]
    return tuple(ptq.motion_box(ptq.motion_sat(int(p)) + ptq.motion_sat(int(v))) for p, v in zip(slot["pos"], slot["vel"]))


def extreme_state():
    """one stream: slots whose pos and vel sit at the int64 extremes, at and just beyond the clamp, around boxes the records meet"""
    st = empty_state(1)
    values = (I64MIN, I64MAX, I64MIN + 1, I64MAX - 1, LIMIT, -LIMIT, LIMIT + 1, -LIMIT - 1, LIMIT - 1, 0, 256 * 30, -1)
    for k in range(24):
        st["slot"]["base"][0, k] = (k + 1, 2, k % 3, 5, (7, 1, 2, 3, 4, ts.conf_bits(k), 10, 10, 40, 40))
        st["slot"]["pad"][0, k] = 0x5A5A5A5A
        for e in range(4):
            st["slot"]["pos"][0, k, e] = values[(k + e) % len(values)]
            st["slot"]["vel"][0, k, e] = values[(k + 2 * e + 5) % len(values)]
    # two slots a record can meet: positions in range, velocities beyond the clamp in opposite directions
    st["slot"]["pos"][0, 0] = (256 * 10, 256 * 10, 256 * 40, 256 * 40)
    st["slot"]["vel"][0, 0] = (0, 0, 0, 0)
    st["slot"]["pos"][0, 1] = (256 * 100, 256 * 100, 256 * 140, 256 * 140)
    st["slot"]["vel"][0, 1] = (I64MAX, I64MIN, I64MAX, I64MIN)
    st["issued"] = 24
    return st
