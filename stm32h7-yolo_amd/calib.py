"""ctypes binding of libyf_calib.so (include/yf_calib.h): calibration of a FLOAT model of the network on the GPU, and with it the whole way from
retrained float weights to a model the int8 engine runs:

    float weights -> .yfw (model_file.write_yfw) -> Calibration.observe(frames) -> ranges() -> ptq.quantize_model -> .yfm
                  -> Network.init_model / Interpreter(model_content=...)

The evaluation is float32 with the arithmetic csrc/yf_calib_arith.h defines ("Calibration arithmetic"); `host_run` is the same
arithmetic on the CPU (libyf_calib_host.so), bit for bit.  Unlike libyf_images.so the library needs no network: it links the HIP runtime only.

Where a quantised model lost precision: Calibration.compare sets the int8 tensors of a run of the engine (Network.run_device with a dump, the
heads) against the float32 tensors of the same frames, per tensor, with the arithmetic csrc/yf_calib_compare.h defines (DESIGN.md,
"Comparison arithmetic"); host_compare is the same on the CPU, bit for bit; quantisation_report makes the table of a .yfw / .yfm pair.

Acting on that table: Calibration.histogram counts every tensor's values over the frames in equal bins of its range (csrc/yf_calib_hist.h,
DESIGN.md "Histogram arithmetic"; host_histogram is the same on the CPU, count for count), ptq.clip_ranges chooses a clipped range from the
counts by percentile or by least modelled error, and quantize_on_device(..., ranges="percentile" / "mse") does all of it.  The default stays
min/max.

What ONE tensor's quantisation costs the logits: Calibration.simulate runs the float32 evaluation with the tensors of a table's enabled
entries put on their int8 grids (csrc/yf_calib_sim.h, DESIGN.md "Simulation arithmetic"; host_simulate is the same on the CPU, bit for bit);
simulation_table makes the table of a .yfm, sensitivity the table of rows -- every tensor alone, every convolution's weights alone, all
activations, all weights, everything -- and quantize_on_device(..., ranges="head") chooses each tensor's range among the min/max, percentile
and mse candidates by the head error its quantisation alone causes.

Changing a number the engine runs with: Calibration.channel_sums gives, per output channel of each of the 24 convolutions, the sum of the
convolution's raw output over the frames, in the float evaluation or under a simulation table (csrc/yf_calib_chan.h, DESIGN.md "Channel-sum
arithmetic"; host_channel_sums is the same on the CPU, bit for bit); correct_biases folds the difference of the simulated and the float means
into the biases (empirical bias correction), and quantize_on_device(..., bias_correction="sequential" / "once") applies it to the model it
returns.

Frames of another size: every function here that takes frames takes [n, h, w, 3] with h and w multiples of 8 up to 160 (160x160 is the
engine's other size) and infers the size from the shape; such frames go through the library's _hw entries, whose kernels keep a frame's
activations in global memory ("Calibration at h x w").  A flat or [n, 56, 56, 3] input means 56x56 and takes the 56x56 entries;
general=True sends 56x56 frames through the _hw entries too, which give the same bits.
"""
import collections
import ctypes
import math
import os

import numpy as np

from . import binding, libs

N_RANGES = 47
FRAME_BYTES = 56 * 56 * 3
LOGITS = 7 * 7 * 18
MAX_ENTRIES = N_RANGES - 1
HIST_MAX_BINS = 4096
MAX_SIDE = 160                  # the _hw entries: h and w are multiples of 8 from 8 to this
# the records of a comparison (csrc/yf_calib_compare.h): per frame and entry, and per entry over the frames.  error = dequantised - float
FRAME_STATS = np.dtype([("sum_err", "<f8"), ("sum_sq_err", "<f8"), ("sum_sq_ref", "<f8"), ("max_abs_err", "<f4"), ("saturated", "<i4")])
TOTALS = np.dtype([("sum_err", "<f8"), ("sum_sq_err", "<f8"), ("sum_sq_ref", "<f8"), ("max_abs_err", "<f4"), ("reserved", "<u4"),
                   ("saturated", "<i8"), ("elements", "<i8")])
assert FRAME_STATS.itemsize == 32 and TOTALS.itemsize == 48

# The table of a simulation (csrc/yf_calib_sim.h): 50 entries {scale, zero_point}; scale 0: the tensor stays float.  Entries 0 .. 46 are the
# range slots in the order of Calibration.ranges() (ascending tensor id), 47 .. 49 the outputs of the graph's QUANTIZE ops.
SIM_ENTRIES = 50
SIM_ENTRY = np.dtype([("scale", "<f4"), ("zero_point", "<i4")])
assert SIM_ENTRY.itemsize == 8
# The channel sums (csrc/yf_calib_chan.h): one double per output channel of every convolution, the convolutions in file order
CHANNELS = 544
N_CONVS = 24
BIAS_MODES = ("sequential", "once")
RANGE_TENSORS = (0, 51, 52, 53, 54, 55, 56, 57, 58, 60, 61, 62, 63, 64, 65, 66, 67, 68, 69, 70, 72, 73, 74, 76, 77, 78, 79, 80, 81, 82, 83, 84, 85, 86,
                 87, 88, 89, 90, 91, 92, 94, 95, 96, 97, 98, 99, 100)

# One tensor of an int8 run: the tflite tensor id, its scale and zero point, and where its values lie -- q: frame 0's first byte (a device tensor
# or address for Calibration.compare, an int8 numpy array for host_compare), frame_stride: bytes from one frame's tensor to the next's.
Entry = collections.namedtuple("Entry", "tensor scale zero_point q frame_stride")


class QTensor(ctypes.Structure):
    """yf_calib_qtensor (include/yf_calib.h)"""
    _fields_ = [("tensor", ctypes.c_int32), ("zero_point", ctypes.c_int32), ("scale", ctypes.c_float), ("reserved", ctypes.c_uint32),
                ("q", ctypes.c_void_p), ("frame_stride", ctypes.c_size_t)]


class CalibError(RuntimeError):
    pass


def lib_path():
    """libyf_calib.so in the package's lib/: it shares nothing with libyf_network.so, so a YF_LIB_PATH override of that one does not move it."""
    return os.path.join(libs.LIB_DIR, "libyf_calib.so")


def host_lib_path():
    return os.path.join(libs.LIB_DIR, "libyf_calib_host.so")


def expected_build_id():
    """The id csrc/Makefile bakes into libyf_calib.so (yf_calib_build_id): sha256 over CALIB_SRCS, CALIBFLAGS and the CFLAGS of the parser."""
    return libs.source_id(libs.make_var("CALIB_SRCS").split(), libs.make_var("CALIBFLAGS") + "|" + libs.make_var("CFLAGS") + "\n")


def library_is_current():
    """True when the in-tree libyf_calib.so can be loaded without running make: it is newer than its sources and the Makefile.  Its baked-in
    id is still checked after loading."""
    return libs.newer_than(lib_path(), libs.make_var("CALIB_SRCS").split() + ["Makefile"])


def frame_size(frames, general=False):
    """(h, w, hw) of frames as the functions here take them: a [n, h, w, 3] array or tensor has its shape's size, anything else (flat,
    [n, 9408], ...) means 56x56.  hw: the call goes to the _hw entries -- every size but 56x56, and 56x56 with general=True.  Whether the
    size is admitted is the library's to say: its text names the rule."""
    shape = tuple(frames.shape)
    h, w = (int(shape[1]), int(shape[2])) if len(shape) == 4 and shape[3] == 3 else (56, 56)
    return h, w, bool(general) or (h, w) != (56, 56)


def elements_at(elements, h, w):
    """A tensor's elements per frame at h x w, from its elements at 56x56 (what the graph's shapes give)."""
    return int(elements) * (h // 8) * (w // 8) // 49


def _host_frames(frames, general):
    """-> (contiguous int8 [n, h, w, 3], h, w, hw).  An input that is not [n, h, w, 3] means 56x56 frames, whichever entries it goes to: a
    length that is no multiple of 9408 is refused here."""
    x = np.ascontiguousarray(frames, np.int8)
    h, w, hw = frame_size(x, general)
    if x.ndim != 4 or x.shape[3] != 3:
        if x.size % FRAME_BYTES:
            raise ValueError(f"frames: expected int8 [n, h, w, 3] or whole 56x56 frames of {FRAME_BYTES} bytes, got {x.shape}")
        x = x.reshape(-1, 56, 56, 3)
    return x, h, w, hw


_lib = None
_host = None

_vp, _ci, _cl, _cp, _cz = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_char_p, ctypes.c_size_t
# The entries that come as a 56x56 and an _hw form, each signature once: the _hw form has (int h, int w) inserted behind the handle (device),
# behind the .yfw and its length (host).  Device: what follows the handle; host: what lies between (yfw, bytes) and (threads, err, errlen).
_DEVICE_ENTRIES = {"observe": [_vp, _cl, _vp, _vp], "compare": [_vp, _cl, ctypes.POINTER(QTensor), _ci, _vp, _vp, _vp],
                   "histogram": [_vp, _cl, _vp, _ci, _vp, _vp], "simulate": [_vp, _cl, _vp, _vp, _vp, _vp, _vp, _vp],
                   "channel_sums": [_vp, _cl, _vp, _vp, _vp, _vp, _vp]}
_HOST_ENTRIES = {"run": [_vp, _cl, _vp, _vp, _vp], "compare": [_vp, _cl, ctypes.POINTER(QTensor), _ci, _vp, _vp, _vp],
                 "histogram": [_vp, _cl, _vp, _ci, _vp], "simulate": [_vp, _cl, _vp, _vp, _vp, _vp, _vp], "channel_sums": [_vp, _cl, _vp, _vp, _vp, _vp]}


def declare_device(lib):
    """restype and argtypes of the ten evaluating entries of a libyf_calib.so (this build's, or another build's loaded beside it)"""
    for op, args in _DEVICE_ENTRIES.items():
        for hw in ("", "_hw"):
            fn = getattr(lib, f"yf_calib_{op}{hw}_device")
            fn.restype, fn.argtypes = _cl, [_vp] + ([_ci, _ci] if hw else []) + args


def load():
    """dlopen libyf_calib.so after the HIP runtime PyTorch uses (binding._one_hip_runtime: one runtime per process), rebuilding it when its
    sources are newer; an existing file is used without a build only if it is current and carries the expected id."""
    global _lib
    if _lib is not None:
        return _lib
    lib = libs.open_library(lib_path(), library_is_current, [("yf_calib_build_id", expected_build_id)], preload=binding._one_hip_runtime)
    lib.yf_calib_build_id.restype = ctypes.c_char_p
    lib.yf_calib_build_id.argtypes = []
    vp, ci = _vp, _ci
    lib.yf_calib_create.restype, lib.yf_calib_create.argtypes = vp, [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int]
    declare_device(lib)
    lib.yf_calib_channel_layout.restype, lib.yf_calib_channel_layout.argtypes = ctypes.c_int, [vp, vp, vp]
    lib.yf_calib_workgroups.restype, lib.yf_calib_workgroups.argtypes = ctypes.c_int, [vp, ci, ci]
    lib.yf_calib_scratch_bytes.restype, lib.yf_calib_scratch_bytes.argtypes = ctypes.c_size_t, [vp]
    lib.yf_calib_ranges.restype, lib.yf_calib_ranges.argtypes = ctypes.c_int, [vp, vp, vp]
    lib.yf_calib_reset.restype, lib.yf_calib_reset.argtypes = ctypes.c_int, [vp]
    lib.yf_calib_frames_observed.restype, lib.yf_calib_frames_observed.argtypes = ctypes.c_long, [vp]
    lib.yf_calib_destroy.restype, lib.yf_calib_destroy.argtypes = None, [vp]
    lib.yf_calib_last_error_text.restype, lib.yf_calib_last_error_text.argtypes = ctypes.c_char_p, []
    _lib = lib
    return lib


def load_host():
    """libyf_calib_host.so (no HIP, no GPU) through libs.host_library, which brings it up to date first."""
    global _host
    if _host is None:
        lib = libs.host_library("libyf_calib_host.so")
        for op, args in _HOST_ENTRIES.items():
            for hw in ("", "_hw"):
                fn = getattr(lib, f"yf_calib_host_{op}{hw}")
                fn.restype, fn.argtypes = _cl, [_cp, _cz] + ([_ci, _ci] if hw else []) + args + [_ci, _cp, _cz]
        lib.yf_calib_channel_layout.restype, lib.yf_calib_channel_layout.argtypes = ctypes.c_int, [_vp, _vp, _vp]
        _host = lib
    return _host


def _entry(lib, stem, suffix, hw, h, w, head, tail):
    """One call of an entry that has two forms, `stem + suffix` (56x56) or `stem + "_hw" + suffix` with (h, w) behind `head` -> (what it
    returned, the name of the entry called: what an error text starts with)"""
    name = f"{stem}{'_hw' if hw else ''}{suffix}"
    return getattr(lib, name)(*head, *((h, w) if hw else ()), *tail), name


def _host_call(op, yfw_bytes, x, h, w, hw, args, threads):
    """yf_calib_host_<op>, or with hw its _hw form, over the frames x [n, h, w, 3].  A refusal, or no frame at all, raises CalibError with the
    library's text."""
    n, err = x.shape[0], ctypes.create_string_buffer(400)
    rc, _ = _entry(load_host(), f"yf_calib_host_{op}", "", hw, h, w, (bytes(yfw_bytes), len(yfw_bytes)), (x.ctypes.data, n, *args, int(threads), err, 400))
    if rc != n or n < 1:
        raise CalibError(f"yf_calib_host_{op}: {err.value.decode()} (returned {rc}, expected {n})")


def _address(q):
    if q is None:
        return None
    if hasattr(q, "data_ptr"):
        return q.data_ptr()
    if isinstance(q, np.ndarray):
        return q.ctypes.data
    return int(q)


def _qtensors(entries):
    """[Entry] -> a ctypes array of yf_calib_qtensor.  Nothing is checked here: the library's one validation names what it refuses."""
    arr = (QTensor * max(len(entries), 1))()
    for i, e in enumerate(entries):
        arr[i] = QTensor(int(e.tensor), int(e.zero_point), float(e.scale), 0, _address(e.q), int(e.frame_stride))
    return arr


def host_compare(yfw_bytes, frames, entries, threads=1, want_tensors=False, elements=None, general=False):
    """The comparison on the CPU: int8 frames [n, h, w, 3] (flat: 56x56) and entries whose q are int8 numpy arrays -> (per-frame records, a FRAME_STATS
    array [n, count]; totals, a TOTALS array [count]; and, with want_tensors, the float32 tensors of the listed entries, one [n, elements]
    array per entry -- `elements` then gives each entry's element count at this frame size).  A refused argument raises CalibError with the
    library's text."""
    x, h, w, hw = _host_frames(frames, general)
    n, count = x.shape[0], len(entries)
    stats, totals = np.zeros((n, max(count, 1)), FRAME_STATS), np.zeros(max(count, 1), TOTALS)
    flat = None
    if want_tensors:
        if elements is None or len(elements) != count:
            raise ValueError("want_tensors: `elements` must give every entry's element count")
        flat = np.zeros(n * int(sum(elements)), np.float32)
    _host_call("compare", yfw_bytes, x, h, w, hw, (_qtensors(entries), count, stats.ctypes.data, totals.ctypes.data,
                                               flat.ctypes.data if want_tensors else None), threads)
    stats, totals = stats[:, :count], totals[:count]
    if not want_tensors:
        return stats, totals
    at, tensors = 0, []
    for e in elements:
        tensors.append(flat[at:at + n * e].reshape(n, e))
        at += n * e
    return stats, totals, tensors


def sim_tensors():
    """The tensor id of each of the 50 entries of a simulation table: the 47 range slots, then the outputs of the graph's QUANTIZE ops in
    ascending tensor id."""
    from . import model_file
    g = model_file.load_graph()
    return RANGE_TENSORS + tuple(sorted(o["out"] for o in g["ops"] if o["op"] == model_file.OPCODE["QUANTIZE"]))


def empty_table():
    """A table with every entry disabled."""
    return np.zeros(SIM_ENTRIES, SIM_ENTRY)


def simulation_table(yfm_bytes, tensors=None):
    """The 50 entries of a simulation from a model's own scales and zero points (a SIM_ENTRY array).  `tensors`: the tensor ids to enable
    (None: all); an id that is not one of the 50 raises ValueError."""
    from . import model_file
    ids, T = sim_tensors(), model_file.load_yfm(yfm_bytes)["tensors"]
    want = set(ids) if tensors is None else {int(t) for t in tensors}
    bad = sorted(want - set(ids))
    if bad:
        raise ValueError(f"tensors: {bad} are not among the {SIM_ENTRIES} tensors of a simulation table ({ids})")
    table = empty_table()
    for i, t in enumerate(ids):
        if t in want:
            table[i] = (np.float32(T[t]["scale"][0]), int(T[t]["zp"]))
    return table


def _table(table):
    t = np.ascontiguousarray(table, SIM_ENTRY) if table is not None else None
    if t is not None and t.shape != (SIM_ENTRIES,):
        raise ValueError(f"table: shape {t.shape}, expected [{SIM_ENTRIES}] entries (simulation_table)")
    return t


def host_simulate(yfw_bytes, frames, table, ref_logits=None, threads=1, general=False, want_stats=False):
    """The simulation on the CPU: int8 frames [n, h, w, 3] (flat: 56x56), a table (simulation_table) and, optionally, reference logits
    [n, h / 8, w / 8, 18] -> (float32 logits, totals: a TOTALS array [1] of the head's error against ref_logits, or None without them); with
    want_stats also the per-frame records, a FRAME_STATS array [n] (None without ref_logits).  A refused argument raises CalibError with the
    library's text."""
    x, h, w, hw = _host_frames(frames, general)
    n, t = x.shape[0], _table(table)
    logits = np.zeros((n, max(h // 8, 0), max(w // 8, 0), 18), np.float32)
    ref = stats = totals = None
    if ref_logits is not None:
        ref = np.ascontiguousarray(ref_logits, np.float32)
        if ref.size != logits.size:
            raise ValueError(f"ref_logits: {ref.shape}, expected {logits.shape}")
        stats, totals = np.zeros(max(n, 1), FRAME_STATS), np.zeros(1, TOTALS)
    ptr = lambda a: None if a is None else a.ctypes.data
    _host_call("simulate", yfw_bytes, x, h, w, hw, (ptr(t), ptr(ref), logits.ctypes.data, ptr(stats), ptr(totals)), threads)
    return (logits, totals, None if stats is None else stats[:n]) if want_stats else (logits, totals)


def channel_layout():
    """(first, cout, pixels56): int32 arrays [24] -- channel first[k] + co of the channel sums is channel co of convolution k (file order),
    and pixels56[k] the pixels per frame of its output at 56x56 (elements_at gives another size's).  From whichever of the two libraries is
    loaded already, else the host build."""
    lib = _lib if _lib is not None else load_host()
    first, cout, pixels = (np.zeros(N_CONVS, np.int32) for _ in range(3))
    rc = lib.yf_calib_channel_layout(first.ctypes.data, cout.ctypes.data, pixels.ctypes.data)
    if rc != CHANNELS:
        raise CalibError(f"yf_calib_channel_layout: returned {rc}, expected {CHANNELS}")
    return first, cout, pixels


def channel_pixels(h, w):
    """float64 [544]: the pixels per frame each channel's sum runs over at h x w -- what a sum over n frames is divided by, times n, for a mean"""
    first, cout, pixels = channel_layout()
    return np.repeat([float(elements_at(p, h, w)) for p in pixels], cout)


def host_channel_sums(yfw_bytes, frames, table=None, threads=1, general=False, want_frames=False, logits=False):
    """The channel sums on the CPU: int8 frames [n, h, w, 3] (flat: 56x56) and a table (simulation_table; None: every entry disabled, the float
    evaluation) -> float64 [544], the sums over all frames; with want_frames (sums, the per-frame sums float64 [n, 544]); with logits the
    float32 logits [n, h / 8, w / 8, 18] as the last item.  A refused argument raises CalibError with the library's text."""
    x, h, w, hw = _host_frames(frames, general)
    n, t = x.shape[0], _table(empty_table() if table is None else table)
    rows, sums = np.zeros((max(n, 1), CHANNELS), np.float64), np.zeros(CHANNELS, np.float64)
    lg = np.zeros((n, max(h // 8, 0), max(w // 8, 0), 18), np.float32) if logits else None
    _host_call("channel_sums", yfw_bytes, x, h, w, hw, (t.ctypes.data, rows.ctypes.data, sums.ctypes.data, lg.ctypes.data if logits else None), threads)
    out = (sums,) + ((rows[:n],) if want_frames else ()) + ((lg,) if logits else ())
    return out[0] if len(out) == 1 else out


def _ranges_dict(minmax, ids):
    return {int(t): (float(minmax[i, 0]), float(minmax[i, 1])) for i, t in enumerate(ids)}


def host_run(yfw_bytes, frames, threads=1, want_logits=True, general=False):
    """The evaluation on the CPU: int8 frames [n, h, w, 3] (flat: 56x56) -> ({tensor id: (min, max)} of these frames, float32 logits
    [n, h / 8, w / 8, 18] or None).  A refused .yfw or frame size raises CalibError with the library's text."""
    x, h, w, hw = _host_frames(frames, general)
    n = x.shape[0]
    minmax, ids = np.zeros((N_RANGES, 2), np.float32), np.zeros(N_RANGES, np.int32)
    logits = np.zeros((n, max(h // 8, 0), max(w // 8, 0), 18), np.float32) if want_logits else None
    _host_call("run", yfw_bytes, x, h, w, hw, (minmax.ctypes.data, ids.ctypes.data, logits.ctypes.data if want_logits else None), threads)
    return _ranges_dict(minmax, ids), logits


def _minmax_array(ranges):
    """{tensor id: (min, max)} -> float32 [47, 2] in the slot order of yf_calib_ranges (ascending tensor id).  Only the count is checked
    here: the library names a row it refuses."""
    ids = sorted(ranges)
    if len(ids) != N_RANGES:
        raise ValueError(f"ranges: {len(ids)} tensors, expected the {N_RANGES} of Calibration.ranges()")
    return np.ascontiguousarray([ranges[t] for t in ids], np.float32)


def host_histogram(yfw_bytes, frames, ranges, bins=2048, threads=1, counts=None, general=False):
    """The histograms on the CPU: int8 frames [n, h, w, 3] (flat: 56x56) and the ranges {tensor id: (min, max)} that give every tensor its axis -> a
    uint64 array [47, bins], rows in the order of sorted(ranges).  `counts` (such an array) is added to and returned.  A refused argument
    raises CalibError with the library's text."""
    x, h, w, hw = _host_frames(frames, general)
    minmax = _minmax_array(ranges)
    if counts is None:
        counts = np.zeros((N_RANGES, max(int(bins), 1)), np.uint64)
    elif counts.dtype != np.uint64 or counts.shape != (N_RANGES, bins) or not counts.flags.c_contiguous:
        raise ValueError(f"counts: expected a contiguous uint64 array [{N_RANGES}, {bins}]")
    _host_call("histogram", yfw_bytes, x, h, w, hw, (minmax.ctypes.data, int(bins), counts.ctypes.data), threads)
    return counts


class Calibration:
    """A calibration of the float model `yfw_bytes` on GPU `device` (None: torch's current device).

    observe(frames)  frames: an int8 device tensor [n, 56, 56, 3] (or a numpy array, which is uploaded).  Asynchronous on torch's current
                     stream (or `stream`, a raw hipStream_t); folds the frames' extremes into the ranges so far.
                     Frames [n, h, w, 3] of another size (h, w multiples of 8 up to 160) take the library's _hw entries (general=True:
                     56x56 frames too); ranges and frames_observed accumulate across sizes.  The first general call at a size larger than
                     any before it allocates the handle's scratch and synchronises the device (workgroups(h, w), scratch_bytes).
    ranges()         synchronises: {tflite tensor id: (min, max)} over everything observed since creation or reset() -- the input, every
                     convolution, LeakyReLU and ADD output and the two pool outputs: what ptq.quantize_model takes.
    logits           the float32 logits [n, h / 8, w / 8, 18] of the last observe (a device tensor; None before the first, or with
                     logits=False)."""

    def __init__(self, yfw_bytes, device=None):
        import torch
        self._lib = load()
        torch.cuda.init()
        if device is None:
            self.device = torch.cuda.current_device()
        else:
            self.device = torch.device("cuda", device).index if isinstance(device, int) else torch.device(device).index
        self.handle = self._lib.yf_calib_create(bytes(yfw_bytes), len(yfw_bytes), self.device)
        if not self.handle:
            raise CalibError(f"yf_calib_create: {self._text()}")
        self.logits = None
        self._keep = None

    def _text(self):
        return (self._lib.yf_calib_last_error_text() or b"").decode()

    def _frames(self, frames, general, at_least_one=False):
        """-> (contiguous int8 device tensor, n, h, w, hw) of frames as observe takes them (frame_size)"""
        import torch
        if not isinstance(frames, torch.Tensor):
            frames = torch.from_numpy(np.ascontiguousarray(frames, np.int8))
        h, w, hw = frame_size(frames, general)
        shaped = len(frames.shape) == 4 and frames.shape[3] == 3           # anything else means whole 56x56 frames, whichever entries it goes to
        if frames.dtype != torch.int8 or (not shaped and frames.numel() % FRAME_BYTES) or (at_least_one and frames.numel() == 0):
            raise ValueError(f"frames: expected int8 [n, h, w, 3]{' with n >= 1' if at_least_one else ''} (flat: 56x56), got {frames.dtype} "
                             f"{tuple(frames.shape)}")
        frames = frames.to(torch.device("cuda", self.device)).contiguous()
        return frames, (frames.shape[0] if shaped else frames.numel() // FRAME_BYTES), h, w, hw

    def _call(self, op, hw, h, w, tail):
        """yf_calib_<op>_device, or with hw yf_calib_<op>_hw_device at (h, w) -> (what it returned, the entry's name)"""
        return _entry(self._lib, f"yf_calib_{op}", "_device", hw, h, w, (self.handle,), tail)

    def workgroups(self, h, w):
        """The workgroups a general launch at (h, w) uses, which is the number of scratch slabs of 800 * (h / 8) * (w / 8) floats each."""
        k = self._lib.yf_calib_workgroups(self.handle, int(h), int(w))
        if k < 1:
            raise CalibError(f"yf_calib_workgroups: {self._text()} (returned {k})")
        return k

    @property
    def scratch_bytes(self):
        return self._lib.yf_calib_scratch_bytes(self.handle)

    def observe(self, frames, logits=True, stream=None, general=False):
        import torch
        frames, n, h, w, hw = self._frames(frames, general, at_least_one=True)
        dev = frames.device
        out = torch.empty((n, h // 8, w // 8, 18), dtype=torch.float32, device=dev) if logits else None
        s = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        rc, name = self._call("observe", hw, h, w, (frames.data_ptr(), n, out.data_ptr() if logits else None, s))
        if rc != n:
            raise CalibError(f"{name}: {self._text()} (returned {rc}, expected {n})")
        self._keep, self.logits = frames, out       # the launch is asynchronous: the frames stay alive until the next call
        return n

    def compare(self, frames, entries, stream=None, general=False):
        """The per-tensor error of an int8 run against the float32 evaluation of the same `frames` (as observe takes them).  entries: a list of
        Entry whose q are int8 device tensors (or device addresses).  Returns (the per-frame records, a uint8 device tensor [n, count, 32]:
        FRAME_STATS, see frame_stats_array; the totals, a TOTALS numpy array [count]).  Launches on torch's current stream (or `stream`, a raw
        hipStream_t) and synchronises the device for the totals.  The handle's ranges and frames_observed are not touched."""
        import torch
        frames, n, h, w, hw = self._frames(frames, general)
        dev, count = frames.device, len(entries)
        d_stats = torch.zeros((n, max(count, 1), FRAME_STATS.itemsize), dtype=torch.uint8, device=dev)
        d_totals = torch.zeros((max(count, 1), TOTALS.itemsize), dtype=torch.uint8, device=dev)
        s = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        if stream is not None:
            torch.cuda.synchronize(dev)                                              # the zeroed outputs were made on torch's stream
        tail = (frames.data_ptr() if n else None, n, _qtensors(entries), count, d_stats.data_ptr(), d_totals.data_ptr(), s)
        rc, name = self._call("compare", hw, h, w, tail)
        if rc != n or n < 1:
            raise CalibError(f"{name}: {self._text()} (returned {rc}, expected {n})")
        torch.cuda.synchronize(dev)                                                  # frames and the entries' tensors are no longer read
        return d_stats[:, :count], d_totals[:count].cpu().numpy().view(TOTALS).reshape(count)

    def histogram(self, frames, ranges=None, bins=2048, counts=None, stream=None, general=False):
        """A second pass over `frames` (as observe takes them): every value of the 47 tensors counted in one of `bins` equal bins of its
        tensor's range -- `ranges` {tensor id: (min, max)}, None: self.ranges().  Returns a uint64 device tensor [47, bins], rows in the
        order of sorted(ranges); passing it back as `counts` accumulates further frames into it.  Asynchronous: the launch goes to torch's
        current stream, or to `stream` (a raw hipStream_t), which is first made to wait, on the device, for what torch's current stream holds
        at this moment -- the upload or copy of `frames`, the zeroing of new counts, earlier histogram calls on the current stream.  Work on
        `counts` or `frames` that the caller queued on any OTHER stream is the caller's to order.  The handle's ranges and frames_observed are
        not touched."""
        import torch
        frames, n, h, w, hw = self._frames(frames, general)
        dev, minmax = frames.device, _minmax_array(self.ranges() if ranges is None else ranges)
        if counts is None:
            counts = torch.zeros((N_RANGES, max(int(bins), 1)), dtype=torch.int64, device=dev).view(torch.uint64)
        elif counts.dtype != torch.uint64 or tuple(counts.shape) != (N_RANGES, bins) or counts.device != dev or not counts.is_contiguous():
            raise ValueError(f"counts: expected a contiguous uint64 tensor [{N_RANGES}, {bins}] on {dev}")
        current = torch.cuda.current_stream(dev)
        s = current.cuda_stream if stream is None else stream
        if s != current.cuda_stream:                                                 # frames and counts were made ready on torch's stream
            torch.cuda.ExternalStream(s, device=dev).wait_event(current.record_event())
        tail = (frames.data_ptr() if n else None, n, minmax.ctypes.data, int(bins), counts.data_ptr(), s)
        rc, name = self._call("histogram", hw, h, w, tail)
        if rc != n or n < 1:
            raise CalibError(f"{name}: {self._text()} (returned {rc}, expected {n})")
        self._keep_hist = frames                    # the launch is asynchronous: the frames stay alive until the next call
        return counts

    def simulate(self, frames, table, ref_logits=None, stream=None, general=False, want_stats=False):
        """The float32 evaluation of `frames` (as observe takes them) with the tensors of the table's enabled entries (simulation_table) on
        their int8 grids.  Returns (the simulated logits, a float32 device tensor [n, h / 8, w / 8, 18]; the totals of the head's error against
        `ref_logits`, a TOTALS numpy array [1] whose `saturated` counts the clipped values over all enabled entries -- None without
        ref_logits, a float32 device tensor or array of the logits' shape); with want_stats also the per-frame records, a uint8 device tensor
        [n, 1, 32] (frame_stats_array), or None.  Launches on torch's current stream (or `stream`, a raw hipStream_t) and synchronises the
        device, as compare does.  The handle's ranges and frames_observed are not touched."""
        import torch
        frames, n, h, w, hw = self._frames(frames, general)
        dev, t = frames.device, _table(table)
        out = torch.empty((n, h // 8, w // 8, 18), dtype=torch.float32, device=dev)
        ref = d_stats = d_totals = None
        if ref_logits is not None:
            ref = ref_logits if isinstance(ref_logits, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(ref_logits, np.float32))
            if ref.dtype != torch.float32 or ref.numel() != out.numel():
                raise ValueError(f"ref_logits: {ref.dtype} {tuple(ref.shape)}, expected float32 {tuple(out.shape)}")
            ref = ref.to(dev).contiguous()
            d_stats = torch.zeros((max(n, 1), 1, FRAME_STATS.itemsize), dtype=torch.uint8, device=dev)
            d_totals = torch.zeros((1, TOTALS.itemsize), dtype=torch.uint8, device=dev)
        s = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        if stream is not None:
            torch.cuda.synchronize(dev)                                              # the outputs and uploads were made on torch's stream
        ptr = lambda v: None if v is None else v.data_ptr()
        tail = (frames.data_ptr() if n else None, n, None if t is None else t.ctypes.data, ptr(ref), out.data_ptr() if n else None, ptr(d_stats),
                ptr(d_totals), s)
        rc, name = self._call("simulate", hw, h, w, tail)
        if rc != n or n < 1:
            raise CalibError(f"{name}: {self._text()} (returned {rc}, expected {n})")
        torch.cuda.synchronize(dev)                                                  # frames and ref_logits are no longer read
        totals = None if ref is None else d_totals.cpu().numpy().view(TOTALS).reshape(1)
        return (out, totals, None if ref is None else d_stats[:n]) if want_stats else (out, totals)

    def channel_sums(self, frames, table=None, general=False, want_frames=False, logits=False, stream=None):
        """Per output channel of each of the 24 convolutions (channel_layout) the sum over `frames` (as observe takes them) of the convolution's
        raw output y = acc + bias, in the float evaluation (table None: every entry disabled) or under a simulation table, where it is the value
        before the convolution's own entry quantises it.  Returns float64 [544] (numpy); with want_frames (sums, the per-frame sums: a float64
        device tensor [n, 544]); with logits the float32 logits, a device tensor [n, h / 8, w / 8, 18], as the last item: simulate's bits for the
        same table.  Launches on torch's current stream (or `stream`, a raw hipStream_t) and synchronises the device for the sums.  The
        handle's ranges and frames_observed are not touched."""
        import torch
        frames, n, h, w, hw = self._frames(frames, general)
        dev, t = frames.device, _table(empty_table() if table is None else table)
        d_rows = torch.empty((max(n, 1), CHANNELS), dtype=torch.float64, device=dev)
        d_sums = torch.empty((CHANNELS,), dtype=torch.float64, device=dev)
        out = torch.empty((n, h // 8, w // 8, 18), dtype=torch.float32, device=dev) if logits else None
        s = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        if stream is not None:
            torch.cuda.synchronize(dev)                                              # the upload was made on torch's stream
        tail = (frames.data_ptr() if n else None, n, t.ctypes.data, d_rows.data_ptr(), d_sums.data_ptr(), out.data_ptr() if logits and n else None, s)
        rc, name = self._call("channel_sums", hw, h, w, tail)
        if rc != n or n < 1:
            raise CalibError(f"{name}: {self._text()} (returned {rc}, expected {n})")
        torch.cuda.synchronize(dev)                                                  # frames are no longer read
        res = (d_sums.cpu().numpy(),) + ((d_rows[:n],) if want_frames else ()) + ((out,) if logits else ())
        return res[0] if len(res) == 1 else res

    @property
    def frames_observed(self):
        return self._lib.yf_calib_frames_observed(self.handle)

    def ranges(self):
        minmax, ids = np.zeros((N_RANGES, 2), np.float32), np.zeros(N_RANGES, np.int32)
        rc = self._lib.yf_calib_ranges(self.handle, minmax.ctypes.data, ids.ctypes.data)
        if rc != N_RANGES:
            raise CalibError(f"yf_calib_ranges: {self._text()} (returned {rc})")
        return _ranges_dict(minmax, ids)

    def reset(self):
        if self._lib.yf_calib_reset(self.handle) != 0:
            raise CalibError(f"yf_calib_reset: {self._text()}")
        self.logits = None

    def destroy(self):
        if self.handle:
            self._lib.yf_calib_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def quantize_on_device(yfw_bytes, frames, device=None, ranges="minmax", percentile=0.9999, bins=2048, keep=(0,), bias_correction=None):
    """Float weights (.yfw bytes) and calibration frames -> the bytes of a .yfm image for Network.init_model: the frames are evaluated on the
    GPU, the ranges go through ptq.quantize_model.  `frames`: an int8 DEVICE tensor [n, 56, 56, 3] of the network's frames (pixel - 128,
    RGB), or [n, h, w, 3] with h and w multiples of 8 up to 160: a model meant for the engine's 160x160 configuration is calibrated on
    [n, 160, 160, 3] frames, so that its ranges are those the int8 network meets at that size (a .yfm carries no size).  Decoded images of
    any size become such frames through images.prepare_device(..., out_hw=160) (or out_hw=56) / prepare_ragged_device first, then this; this
    function does not wrap that step.
    ranges: "minmax" (the default) gives every tensor the extremes observed; "percentile" and "mse" clip them (ptq.clip_ranges with
    `percentile` and `keep`) on histograms of `bins` bins taken in a second pass over the same frames; "head" gives every tensor but those
    of `keep` the one of its min/max, percentile and mse ranges whose quantisation, alone in an otherwise float evaluation of the same
    frames, leaves the least squared error on the logits (head_ranges: some 140 further passes).
    bias_correction: None (the default: the model is quantize_model's of the ranges, byte for byte), or "sequential" / "once": the biases are
    corrected on the same frames after the ranges are chosen, whichever method chose them (correct_biases)."""
    from . import ptq
    if ranges not in ptq.CLIP_METHODS + ("head",):
        raise ValueError(f"ranges: {ranges!r}, expected one of {ptq.CLIP_METHODS + ('head',)}")
    if bias_correction is not None and bias_correction not in BIAS_MODES:
        raise ValueError(f"bias_correction: {bias_correction!r}, expected None or one of {BIAS_MODES}")
    cal = Calibration(yfw_bytes, device)
    try:
        frames = cal._frames(frames, False, at_least_one=True)[0]        # (on the device once, for every pass below)
        cal.observe(frames, logits=False)
        chosen = cal.ranges()
        if ranges != "minmax":
            observed = chosen
            counts = cal.histogram(frames, observed, bins).cpu().numpy()
            if ranges == "head":
                cands = range_candidates(counts, observed, percentile, keep)
                chosen = head_ranges(cands, lambda table, ref: cal.simulate(frames, table, ref), keep)
            else:
                chosen = ptq.clip_ranges(counts, observed, ranges, percentile, keep)
        device = cal.device
    finally:
        cal.destroy()
    if bias_correction is None:
        return ptq.quantize_model(yfw_bytes, chosen)
    return correct_biases(yfw_bytes, chosen, frames, device, bias_correction)[0]


def _frame_count(frames):
    return int(frames.shape[0]) if len(frames.shape) == 4 and frames.shape[3] == 3 else int(np.prod(tuple(frames.shape))) // FRAME_BYTES


def correct_biases(yfw_bytes, ranges, frames, device=None, mode="sequential", channel_sums=None):
    """Empirical bias correction: float weights (.yfw bytes), the ranges chosen for them ({tensor id: (min, max)}: they are used as given, not
    derived again) and calibration frames (as observe takes them) -> (the bytes of a .yfm image, report).  Per output channel of each
    convolution the mean of the raw output y = acc + bias over the frames is measured in the float evaluation of `yfw_bytes` (mean_float: one
    pass with every entry disabled; a mean is the channel's sum divided by n * pixels, in Python floats) and in the full simulation of the
    quantised model (mean_sim: its dequantised weights, ptq.dequantized_yfw, under its whole table, simulation_table), and the difference err =
    mean_sim - mean_float is taken out of the bias: the convolution's new float bias is float32(q * s_bias - err), its current quantised bias
    dequantised, in double.  The engine adds the bias into its int32 accumulator: the correction costs nothing at run time.
      "sequential"  for k = 0 .. 23 in graph order: quantise the current weights, one simulated pass, correct convolution k alone.  A
                    convolution's output depends on earlier convolutions only, so convolution k's offset in the final model is what step k left.
      "once"        one simulated pass, every convolution corrected from it.
    report: one dict per convolution -- conv, tensor (the convolution's output), max_err and rms_err: the largest and the root-mean-square
    |err| over its channels before its correction, in units of the output tensor's scale.
    The passes run on GPU `device` (None: torch's current), each weight set on a handle of its own that is destroyed after its pass;
    `channel_sums`, if given, replaces them: channel_sums(yfw_bytes, frames, table) -> float64 [544], e.g. host_channel_sums."""
    from . import model_file, ptq
    if mode not in BIAS_MODES:
        raise ValueError(f"mode: {mode!r}, expected one of {BIAS_MODES}")
    h, w, _ = frame_size(frames)
    n = _frame_count(frames)

    def sums(yfw, table):
        if channel_sums is not None:
            return np.asarray(channel_sums(yfw, frames, table), np.float64).reshape(CHANNELS)
        cal = Calibration(yfw, device)
        try:
            return cal.channel_sums(frames, table)
        finally:
            cal.destroy()

    first, cout, _ = channel_layout()
    count = channel_pixels(h, w) * float(n)
    mean_float = sums(bytes(yfw_bytes), empty_table()) / count
    convs, current, report = model_file.graph_convs(), bytes(yfw_bytes), []
    for step in (range(N_CONVS) if mode == "sequential" else (None,)):
        yfm = ptq.quantize_model(current, ranges)
        err = sums(ptq.dequantized_yfw(current, yfm), simulation_table(yfm)) / count - mean_float
        m = model_file.load_yfm(yfm)
        biases = [None] * N_CONVS
        for k in (range(N_CONVS) if step is None else (step,)):
            op = m["ops"][convs[k]["op"]]
            bt, e = m["tensors"][op["ins"][2]], err[first[k]:first[k] + cout[k]]
            deq = bt["data"].astype(np.float64) * bt["scale"].astype(np.float32).astype(np.float64)
            biases[k] = (deq - e).astype(np.float32)
            lsb = np.abs(e) / float(m["tensors"][op["out"]]["scale"][0])
            report.append(dict(conv=k, tensor=int(op["out"]), max_err=float(lsb.max()), rms_err=float(np.sqrt((lsb * lsb).mean()))))
        current = ptq.with_biases(current, biases)
    return ptq.quantize_model(current, ranges), report


def format_bias_report(report):
    """the report of correct_biases as text, one line per convolution"""
    out = [f"{'conv':>4} {'tensor':>6} {'max |err| / scale':>18} {'rms |err| / scale':>18}"]
    for r in report:
        out.append(f"{r['conv']:>4} {r['tensor']:>6} {r['max_err']:>18.4f} {r['rms_err']:>18.4f}")
    return "\n".join(out)


def frame_stats_array(d_stats):
    """The per-frame records of Calibration.compare (a device tensor) -> a FRAME_STATS numpy array [n, count]."""
    a = d_stats.contiguous().cpu().numpy()
    return a.view(FRAME_STATS).reshape(a.shape[0], a.shape[1])


# the ops whose output the float evaluation holds as a tensor of its own: PAD, QUANTIZE and CONCATENATION only move values
_EVALUATED = ("CONV_2D", "DEPTHWISE_CONV_2D", "LEAKY_RELU", "ADD", "MAX_POOL_2D")


def report_tensors(dump_offset, yfm_bytes):
    """The tensors a run of the engine leaves for a comparison, in op order: [dict(tensor, op, elements (per frame), scale, zero_point,
    offset)].  The ops and shapes come from the graph the library is built for (model_file.load_graph), scale and zero point from the .yfm,
    `offset` from dump_offset(op) (Network.dump_offset): every evaluated op the dump has a record of, and the network's output, whose
    `offset` is None -- its values are the heads, not part of the dump."""
    from . import model_file
    graph, model = model_file.load_graph(), model_file.load_yfm(yfm_bytes)
    codes = {model_file.OPCODE[k] for k in _EVALUATED}
    out = []
    for i, op in enumerate(graph["ops"]):
        off, t = dump_offset(i), op["out"]
        if op["op"] not in codes or (off < 0 and t != graph["output"]):
            continue
        q = model["tensors"][t]
        out.append(dict(tensor=t, op=i, elements=int(np.prod(graph["tensors"][t]["shape"][1:])), scale=np.float32(q["scale"][0]),
                        zero_point=int(q["zp"]), offset=None if t == graph["output"] else int(off)))
    return out


def report_rows(tensors, totals):
    """report_tensors' list and the totals of a comparison of exactly these entries -> the table: one dict per tensor with tensor, op,
    elements (all frames), scale, zero_point, mean_error, max_abs_error, mean_squared_error, rmse_over_scale, sqnr_db and saturated (the share
    of the elements at -128 or 127).  error = dequantised int8 value - float32 value."""
    rows = []
    for t, r in zip(tensors, totals):
        k, scale = int(r["elements"]), float(t["scale"])
        mse, ref, err = float(r["sum_sq_err"]) / k, float(r["sum_sq_ref"]), float(r["sum_sq_err"])
        rows.append(dict(tensor=t["tensor"], op=t["op"], elements=k, scale=scale, zero_point=t["zero_point"], mean_error=float(r["sum_err"]) / k,
                         max_abs_error=float(r["max_abs_err"]), mean_squared_error=mse, rmse_over_scale=math.sqrt(mse) / scale,
                         sqnr_db=10.0 * math.log10(ref / err) if err > 0.0 and ref > 0.0 else (math.inf if ref > 0.0 else -math.inf),
                         saturated=int(r["saturated"]) / k))
    return rows


def _head_report(network, yfw_bytes, yfm_bytes, d_x, h, w):
    """quantisation_report at a size other than 56x56: the head alone (see there)"""
    import torch
    dev, n, logits = d_x.device, d_x.shape[0], (h // 8) * (w // 8) * 18
    d_out = torch.zeros((n, logits), dtype=torch.int8, device=dev)
    network.run_device_hw(h, w, d_x.data_ptr(), d_out.data_ptr(), n, torch.cuda.current_stream(dev).cuda_stream)
    tensors = [t for t in report_tensors(network.dump_offset, yfm_bytes) if t["offset"] is None]
    entries = [Entry(t["tensor"], t["scale"], t["zero_point"], d_out.data_ptr(), logits) for t in tensors]
    cal = Calibration(yfw_bytes, dev.index)
    try:
        _, totals = cal.compare(d_x, entries)
    finally:
        cal.destroy()
    return report_rows(tensors, totals)


def quantisation_report(network, yfw_bytes, yfm_bytes, frames):
    """Where the int8 model `yfm_bytes` loses precision against the float model `yfw_bytes` it was quantised from, over `frames` (int8
    [n, 56, 56, 3], numpy or device): one row per tensor in op order (report_rows), TFLite's quantisation-debugger table for the model that
    runs, under the rounding in force.  `network` is a Network initialised from yfm_bytes (init_model): it runs the frames with a dump of every
    fused stage's tensor, and the dumped tensors and the heads are compared with the float32 evaluation on the GPU.
    Frames [n, h, w, 3] of another size the engine runs (160x160) give the head's row alone (tensor 100, from run_device_hw): the engine's
    per-stage dump exists at 56x56 only (yf_network_run_device_dump), so there is nothing to set the inner tensors against."""
    import torch
    dev = torch.device("cuda", network._device)
    if not isinstance(frames, torch.Tensor):
        frames = torch.from_numpy(np.ascontiguousarray(frames, np.int8))
    h, w, hw = frame_size(frames)
    if hw:
        if frames.dtype != torch.int8 or frames.numel() == 0:
            raise ValueError(f"frames: expected int8 [n, h, w, 3] with n >= 1, got {frames.dtype} {tuple(frames.shape)}")
        return _head_report(network, yfw_bytes, yfm_bytes, frames.to(dev).contiguous(), h, w)
    if frames.dtype != torch.int8 or frames.numel() % FRAME_BYTES or frames.numel() == 0:
        raise ValueError(f"frames: expected int8 [n, 56, 56, 3] with n >= 1, got {frames.dtype} {tuple(frames.shape)}")
    d_x = frames.to(dev).contiguous()
    n, dump_bytes = d_x.numel() // FRAME_BYTES, network.dump_bytes()
    d_out = torch.zeros((n, LOGITS), dtype=torch.int8, device=dev)
    d_dump = torch.zeros((n, dump_bytes), dtype=torch.int8, device=dev)
    network.run_device(d_x.data_ptr(), d_out.data_ptr(), n, torch.cuda.current_stream(dev).cuda_stream, d_dump.data_ptr())
    tensors = report_tensors(network.dump_offset, yfm_bytes)
    entries = [Entry(t["tensor"], t["scale"], t["zero_point"], d_out.data_ptr() if t["offset"] is None else d_dump.data_ptr() + t["offset"],
                     LOGITS if t["offset"] is None else dump_bytes) for t in tensors]
    cal = Calibration(yfw_bytes, dev.index)
    try:
        _, totals = cal.compare(d_x, entries)
    finally:
        cal.destroy()
    return report_rows(tensors, totals)


# ---------------------------------------------------------------------------------------------------------------- sensitivity
def range_candidates(counts, observed, percentile=0.9999, keep=(0,)):
    """{tensor: [its "minmax", "percentile" and "mse" range]} (the order of ptq.CLIP_METHODS) from the histograms `counts` on the axes of the
    ranges `observed`: what ranges="head" chooses among."""
    from . import ptq
    by_method = [ptq.clip_ranges(counts, observed, m, percentile, keep) for m in ptq.CLIP_METHODS]
    return {t: [r[t] for r in by_method] for t in sorted(by_method[0])}


def head_ranges(candidates, simulate, keep=(0,)):
    """The choice of ranges="head": candidates {tensor: [range, ...]} over the 47 range tensors, simulate(table, ref_logits) -> (logits,
    totals) on the calibration frames (Calibration.simulate or host_simulate with the weights and frames bound).  For every tensor not in
    `keep` each candidate's error is the head's sum_sq_err when that tensor alone is quantised with ptq.activation_qparams of the candidate,
    against the logits of the all-float evaluation; a candidate equal to an earlier one of the same tensor takes that one's error.
    ptq.choose_ranges picks.  The tensors of `keep` take their first candidate."""
    from . import ptq
    keep = {int(t) for t in keep}
    ref, _ = simulate(empty_table(), None)
    errors = {}
    for t, cands in candidates.items():
        slot, done = RANGE_TENSORS.index(int(t)), {}
        if int(t) in keep:
            errors[t] = [0.0] * len(cands)
            continue
        errors[t] = []
        for r in cands:
            key = (float(r[0]), float(r[1]))
            if key not in done:
                table = empty_table()
                table[slot] = ptq.activation_qparams(*key)
                done[key] = float(simulate(table, ref)[1][0]["sum_sq_err"])
            errors[t].append(done[key])
    return ptq.choose_ranges(candidates, errors)


def _sim_elements(h, w):
    """elements per frame of each of the 50 entries at h x w"""
    from . import model_file
    shapes = model_file.load_graph()["tensors"]
    return [elements_at(int(np.prod(shapes[t]["shape"][1:])), h, w) for t in sim_tensors()]


def sensitivity_row(name, op, tensor, conv, totals, head_scale, quantised):
    """One row of the sensitivity table from the totals of a simulation against the float logits: head SQNR in dB, rmse and maximum error in
    head LSB (head_scale: the model's output scale), and the share of the `quantised` values (all frames) that were clipped."""
    r = totals[0]
    k, err, ref = int(r["elements"]), float(r["sum_sq_err"]), float(r["sum_sq_ref"])
    return dict(name=name, op=op, tensor=tensor, conv=conv,
                sqnr_db=10.0 * math.log10(ref / err) if err > 0.0 and ref > 0.0 else (math.inf if ref > 0.0 else -math.inf),
                rmse_lsb=math.sqrt(err / k) / head_scale, max_lsb=float(r["max_abs_err"]) / head_scale,
                clipped=int(r["saturated"]) / quantised if quantised else 0.0)


def sensitivity(yfw_bytes, yfm_bytes, frames, device=None, simulate=None):
    """What each tensor's quantisation costs the logits of the float model `yfw_bytes` under the scales and zero points of the int8 model
    `yfm_bytes`, over `frames` (int8 [n, h, w, 3] of any admitted size, numpy or device; flat: 56x56).  The reference is the evaluation with
    every entry disabled.  Rows (sensitivity_row), in this order: one per table entry enabled alone (50, `op` the name of the op that makes
    the tensor, "INPUT" for the input); one per convolution whose weights and bias alone are the model's dequantised numbers
    (ptq.dequantized_yfw; 24, op "WEIGHTS"); "activations" (all 50 entries), "weights" (all 24 convolutions) and "all".
    The evaluations run on GPU `device` (None: torch's current device), each weight set on a handle of its own; `simulate`, if given,
    replaces them: simulate(yfw_bytes, frames, table, ref_logits) -> (logits, totals), e.g. host_simulate."""
    from . import model_file, ptq
    h, w, _ = frame_size(frames)
    n = _frame_count(frames)
    graph, model = model_file.load_graph(), model_file.load_yfm(yfm_bytes)
    head_scale = float(model["tensors"][graph["output"]]["scale"][0])
    names = {v: k for k, v in model_file.OPCODE.items()}
    made_by = {o["out"]: names[o["op"]] for o in graph["ops"]}
    ids, elements, full = sim_tensors(), _sim_elements(h, w), simulation_table(yfm_bytes)
    handles = []

    def on(yfw):
        """a simulate(table, ref) of one weight set: on the device one handle serves all its calls"""
        if simulate is not None:
            return lambda table, ref: simulate(yfw, frames, table, ref)
        cal = Calibration(yfw, device)
        handles.append(cal)
        return lambda table, ref: cal.simulate(frames, table, ref)

    rows = []
    try:
        base = on(yfw_bytes)
        ref, _ = base(empty_table(), None)
        for i, t in enumerate(ids):
            table = empty_table()
            table[i] = full[i]
            rows.append(sensitivity_row(f"tensor {t}", made_by.get(t, "INPUT"), t, None, base(table, ref)[1], head_scale, n * elements[i]))
        for c in range(len(model_file.graph_convs(graph))):
            one = on(ptq.dequantized_yfw(yfw_bytes, yfm_bytes, [c]))
            rows.append(sensitivity_row(f"conv {c}", "WEIGHTS", None, c, one(empty_table(), ref)[1], head_scale, 0))
            if handles:
                handles.pop().destroy()
        rows.append(sensitivity_row("activations", "", None, None, base(full, ref)[1], head_scale, n * sum(elements)))
        deq = on(ptq.dequantized_yfw(yfw_bytes, yfm_bytes))
        rows.append(sensitivity_row("weights", "", None, None, deq(empty_table(), ref)[1], head_scale, 0))
        rows.append(sensitivity_row("all", "", None, None, deq(full, ref)[1], head_scale, n * sum(elements)))
    finally:
        for cal in handles:
            cal.destroy()
    return rows


def format_sensitivity(rows):
    """the table of sensitivity() as text, one line per row"""
    out = [f"{'what':<14} {'op':<18} {'head SQNR dB':>12} {'rmse LSB':>9} {'max LSB':>8} {'clipped':>9}"]
    for r in rows:
        out.append(f"{r['name']:<14} {r['op']:<18} {r['sqnr_db']:>12.2f} {r['rmse_lsb']:>9.4f} {r['max_lsb']:>8.3f} {r['clipped']:>9.6f}")
    return "\n".join(out)
