"""Round 11 re-ordered the lanes of pool_8's horizontal pass in the two-frame fused 56x56 kernels: it takes the ROWS across the lanes (wave k sweeps chunk
k of five outputs, a frame per half-wave, four surplus lanes per half masked).  Same sweep, same buffers; the vertical pass, whose re-ordering was tried with
it, keeps its order.  Heads, detection records and counts of run_decode_device against the oracle on batches that take the one-frame kernel
(2, the control: it keeps the old horizontal pass), the smallest two-frame launch (513), one with an unpaired one-frame last group (515) and one whose
workgroups get a pair of groups or a single one (1030), for the three kernel sets, and run_camera_device on 513 frames; a guard frame behind every output.

The first and last groups of every batch hold the six golden frames and 29 BAND FRAMES: the input zero point everywhere except input rows 4t .. 4t+3
(t = 0 .. 13) of one seeded random frame, the same for input columns 4t .. 4t+3, and one frame with both bands at t = 13.  Input rows 4t .. 4t+3 reach rows
2t-1 .. 2t+3 of pool_8's input and so rows t-2 .. t+3 of its output: the bands walk over both chunk boundaries of the sweeps (outputs 4|5 and 8|9), every
clamped edge and row 27, the row next to the masked lanes.  test_band_frames_move_pool_8_where_they_should states that from the oracle's op dump, no GPU
involved.  The launches run in one child process under a time limit; the comparisons run here."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

BATCHES = (2, 513, 515, 1030)
CAMERA_BATCH = 513
ROUNDINGS = {"tflite_ref": 0, "ties_up": 1, "fp32": 3}         # name: the oracle's variant (oracle/yf_oracle.h)
N_CAM, CAP, GUARD = 24, 4, 0x4D
OP_POOL8_IN, OP_POOL8 = 7, 8                                   # LEAKY_RELU #7 (28x28x18), MAX_POOL_2D #8 (14x14x18) in the model's op list
DET = lambda d: (int(d["anchor"]), int(d["row"]), int(d["col"]), int(d["x1"]), int(d["y1"]), int(d["x2"]), int(d["y2"]))   # noqa: E731
ORACLE_DET = lambda d: (d[1], d[2], d[3], d[6], d[7], d[8], d[9])                                                          # noqa: E731

CHILD = r"""
import sys, importlib, numpy as np, torch
sys.path.insert(0, sys.argv[1])
yf = importlib.import_module('stm32h7-yolo_amd')
z = np.load(sys.argv[2])
cap, guard = int(sys.argv[4]), int(sys.argv[5])
net = yf.Network(device=0).init()
d_in, d_raw = torch.from_numpy(z['x']).cuda(), torch.from_numpy(z['raw']).cuda()
out = {}
def bufs(n):
    return (torch.full((n + 1, 7, 7, 18), guard, dtype=torch.int8, device='cuda'), torch.full((n + 1, cap, 28), guard, dtype=torch.uint8, device='cuda'),
            torch.full((n + 1,), guard, dtype=torch.int32, device='cuda'))
for name, rounding in (('tflite_ref', yf.YF_ROUND_TFLITE_REF), ('ties_up', yf.YF_ROUND_TIES_UP), ('fp32', yf.YF_ROUND_FP32)):
    net.set_requant_rounding(rounding)
    for n in (2, 513, 515, 1030):
        d_h, d_d, d_c = bufs(n)
        net.run_decode_device(d_in.data_ptr(), d_h.data_ptr(), n, d_d.data_ptr(), d_c.data_ptr(), cap, yf.YF_DECODE_PY)
        torch.cuda.synchronize()
        out[f'{name}_{n}_heads'], out[f'{name}_{n}_dets'], out[f'{name}_{n}_counts'] = d_h.cpu().numpy(), d_d.cpu().numpy(), d_c.cpu().numpy()
        out[f'{name}_{n}_kernel'] = np.array(net.kernel_name_for(n))
    n = z['raw'].shape[0]
    d_h, d_d, d_c = bufs(n)
    net.run_camera_device(d_raw.data_ptr(), d_h.data_ptr(), n, d_d.data_ptr(), d_c.data_ptr(), cap, yf.YF_DECODE_FW)
    torch.cuda.synchronize()
    out[f'{name}_cam_heads'], out[f'{name}_cam_dets'], out[f'{name}_cam_counts'] = d_h.cpu().numpy(), d_d.cpu().numpy(), d_c.cpu().numpy()
net.destroy()
np.savez(sys.argv[3], **out)
"""


def band_frames(zp):
    """29 frames: row bands t = 0 .. 13, column bands t = 0 .. 13, both bands at t = 13."""
    val = np.random.default_rng(11).integers(-128, 128, (56, 56, 3), dtype=np.int8)
    blank = np.full((56, 56, 3), zp, np.int8)
    frames = []
    for axis in (0, 1):
        for t in range(14):
            f = blank.copy()
            sl = (np.s_[4 * t:4 * t + 4],) if axis == 0 else (np.s_[:], np.s_[4 * t:4 * t + 4])
            f[sl] = val[sl]
            frames.append(f)
    f = blank.copy()
    f[52:] = val[52:]
    f[:, 52:] = val[:, 52:]
    frames.append(f)
    return np.stack(frames)


@pytest.fixture(scope="module")
def model():
    from oracle.np_restatement import load_yfm
    return load_yfm(os.path.join(ROOT, "oracle", "model", "yoloface_int8.yfm"))


@pytest.fixture(scope="module")
def zero_point(model):
    return int(model["tensors"][model["input"]]["zp"])


@pytest.fixture(scope="module")
def batch(golden, zero_point):
    special = np.concatenate([band_frames(zero_point), golden["inputs"]])
    n = max(BATCHES)
    x = np.random.default_rng(1111).integers(-128, 128, (n, 56, 56, 3), dtype=np.int8)
    k = len(special)
    assert k == 35 and 2 * k < 512
    x[2:2 + k] = special                           # the two-frame launches see them in their first groups (a band frame at an even index is frame 0 of its group),
    x[515 - k:515] = special                       # ... in the last groups of 513 and 515 (515: frame 514, the last golden frame, is a group of its own)
    x[n - k:] = special                            # ... and in the last groups of 1030, at odd indices: every band frame is frame 1 of a group too
    x[0] = special[13]                             # the one-frame launch: the row band and the column band at t = 13
    x[1] = special[27]
    return x


@pytest.fixture(scope="module")
def camera(oracle):
    rng = np.random.default_rng(1112)
    base = rng.integers(0, 256, (N_CAM, 112 * 112 * 2), dtype=np.uint8)
    pick = np.arange(CAMERA_BATCH) * 7 % N_CAM                           # neighbours differ (7 and 24 are coprime)
    return dict(base=base, pick=pick, frames=np.stack([oracle.prepare_rgb565(r) for r in base]))


@pytest.fixture(scope="module")
def reference(oracle, batch, camera):
    return {name: dict(heads=oracle.run(batch, threads=16, variant=variant), cam=oracle.run(camera["frames"], threads=16, variant=variant))
            for name, variant in ROUNDINGS.items()}


@pytest.fixture(scope="module")
def gpu_results(batch, camera, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pool_lanes")
    src, dst = str(tmp / "frames.npz"), str(tmp / "out.npz")
    np.savez(src, x=batch, raw=camera["base"][camera["pick"]])
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, src, dst, str(CAP), str(GUARD)], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return dict(np.load(dst))


def test_band_frames_move_pool_8_where_they_should(oracle, model, zero_point):
    """From the oracle's op dump, under the reference rounding: against the all-zero-point frame a band at t changes pool_8's output (op 8, 14x14x18) only inside
    rows (columns) t-3 .. t+3 -- in every row t-2 .. t+3 that exists (input rows 4t .. 4t+3 reach conv2d_1's rows 2t .. 2t+2, conv2d_3's and so pool_8's input
    rows 2t-1 .. 2t+3, which the windows [2o-3, 2o+4] of the outputs o = t-2 .. t+3 meet) and in every position across the band -- and changes the heads.  The
    dump's op 8 is the 8x8 stride-2 maximum of its op 7, padded by three: what pool_8's two passes compute."""
    sizes = [int(np.prod(model["tensors"][o["out"]]["shape"][1:])) for o in model["ops"]]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    assert sizes[OP_POOL8_IN] == 28 * 28 * 18 and sizes[OP_POOL8] == 14 * 14 * 18
    frames = np.concatenate([np.full((1, 56, 56, 3), zero_point, np.int8), band_frames(zero_point)])
    assert len(frames) == 30
    heads, dump = oracle.run(frames, dump=True, threads=8)
    t4 = dump[:, offs[OP_POOL8_IN]:offs[OP_POOL8_IN] + sizes[OP_POOL8_IN]].reshape(-1, 28, 28, 18)
    p8 = dump[:, offs[OP_POOL8]:offs[OP_POOL8] + sizes[OP_POOL8]].reshape(-1, 14, 14, 18)
    padded = np.full((len(frames), 28 + 7, 28 + 7, 18), -128, np.int8)
    padded[:, 3:31, 3:31] = t4
    want = np.stack([padded[:, dy:dy + 28:2, dx:dx + 28:2] for dy in range(8) for dx in range(8)]).max(axis=0)
    assert np.array_equal(p8, want)
    for axis in (0, 1):
        for t in range(14):
            i = 1 + 14 * axis + t
            moved = (p8[i] != p8[0]).any(axis=2)
            along, across = np.nonzero(moved.any(axis=1 - axis))[0], np.nonzero(moved.any(axis=axis))[0]
            assert along.min() >= t - 3 and along.max() <= t + 3, (axis, t, along)
            assert list(along) == list(range(max(t - 2, 0), min(t + 3, 13) + 1)), (axis, t, along)
            assert list(across) == list(range(14)), (axis, t, across)
            assert 360 <= int((heads[i] != heads[0]).sum()) <= 694, (axis, t)                 # of 882 head bytes
    moved = (p8[29] != p8[0]).any(axis=2)
    assert moved[11:].all() and moved[:, 11:].all() and not moved[:11, :11].any()
    assert not np.array_equal(heads[29], heads[0]) and len({h.tobytes() for h in heads}) == 30


def check(yf, oracle, res, key, n, want, decode):
    heads, dets, counts = res[f"{key}_heads"], res[f"{key}_dets"], res[f"{key}_counts"]
    bad = np.nonzero((heads[:n] != want).reshape(n, -1).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} frames differ, first {bad[:8]}"
    assert (heads[n] == GUARD).all() and (dets[n] == GUARD).all() and counts[n] == GUARD       # nothing behind the batch
    rec = dets.view(yf.DET_DTYPE).reshape(n + 1, CAP)
    for f in range(n):
        ref = decode(heads[f], f)
        assert counts[f] == len(ref), f
        assert [DET(d) for d in rec[f, :min(CAP, counts[f])]] == [ORACLE_DET(d) for d in ref][:CAP], f


@pytest.mark.gpu
@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("rounding", sorted(ROUNDINGS))
def test_heads_and_records_equal_the_oracle(yf, oracle, reference, gpu_results, rounding, n):
    kernel = str(gpu_results[f"{rounding}_{n}_kernel"])
    assert ("<F=1," in kernel) == (n == 2) and ("<F=2," in kernel) == (n > 2), kernel       # 2 frames: the one-frame kernel; the others: two frames per group
    check(yf, oracle, gpu_results, f"{rounding}_{n}", n, reference[rounding]["heads"][:n], oracle.decode_py)


@pytest.mark.gpu
@pytest.mark.parametrize("rounding", sorted(ROUNDINGS))
def test_camera_frames_equal_the_oracle(yf, oracle, reference, gpu_results, camera, rounding):
    check(yf, oracle, gpu_results, f"{rounding}_cam", CAMERA_BATCH, reference[rounding]["cam"][camera["pick"]], oracle.decode_c)
