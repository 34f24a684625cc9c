"""Round 10 moved two LDS layouts of the fused 56x56 kernels: T8 (conv2d_15's input) has a row pitch of 608 bytes, with T9 and T11 512 bytes further up,
and conv2d_1 reads the taps kx = 1, 2 of a kernel row as one 8-byte pair, with its weights' k slots re-ordered in registers to match.  Heads, detection
records and counts of run_decode_device against the oracle on batches that take the one-frame kernel (2), the smallest two-frame launch (513), one with an
unpaired one-frame last group (515) and one whose workgroups get a pair of groups or a single one (1030), for the three kernel sets (reference rounding,
ties upward, float32), and run_camera_device on 513 frames; a guard frame behind every output.

The first and last groups of every batch hold structured frames that are the input zero point except
  (a) ONE pixel in one colour channel: the nine positions of the 3x3 patch of an even and of an odd output column of conv2d_1, the top-left corner, the right
      edge, the bottom edge and the bottom-right corner -- a wrong k slot or a pair shifted by one dword moves or drops exactly these;
  (b) input columns 52-55, input rows 52-55, and both: what reaches column 13 and row 13 of the 14x14 grid, the pixels beside T8's skew bytes and halo ring;
  (c) the six golden frames.
The oracle's heads for (a) and (b) differ from the all-zero-point frame's, frame by frame (test_structured_frames_reach_the_heads: no GPU involved in that
statement).  The launches run in one child process under a time limit; the comparisons run here."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

BATCHES = (2, 513, 515, 1030)
CAMERA_BATCH = 513
ROUNDINGS = {"tflite_ref": 0, "ties_up": 1, "fp32": 3}         # name: the oracle's variant (oracle/yf_oracle.h)
N_CAM, CAP, GUARD = 24, 4, 0x4D
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


def impulse_positions():
    """(row, col) of the single non-zero input pixel of each impulse frame.  conv2d_1's output (oy, ox) reads input rows 2oy-1 .. 2oy+1 and columns
    2ox-1 .. 2ox+1: the 3x3 patches of output (5, 6) (even column) and (6, 7) (odd column), then corner and edges."""
    pos = [(2 * oy - 1 + ky, 2 * ox - 1 + kx) for oy, ox in ((5, 6), (6, 7)) for ky in range(3) for kx in range(3)]
    return pos + [(0, 0), (20, 55), (55, 30), (55, 55)]


def structured_frames(zp):
    hot = 127 if zp < 0 else -128                   # the value furthest from the zero point
    rng = np.random.default_rng(10)
    val = rng.integers(-128, 128, (56, 56, 3), dtype=np.int8)
    val[val == zp] = hot
    frames = []
    for k, (r, c) in enumerate(impulse_positions()):                     # (a)
        f = np.full((56, 56, 3), zp, np.int8)
        f[r, c, k % 3] = hot
        frames.append(f)
    for sl in ((np.s_[:, 52:],), (np.s_[52:, :],), (np.s_[:, 52:], np.s_[52:, :])):     # (b)
        f = np.full((56, 56, 3), zp, np.int8)
        for s in sl:
            f[s] = val[s]
        frames.append(f)
    return np.stack(frames)


@pytest.fixture(scope="module")
def zero_point():
    from oracle.np_restatement import load_yfm
    m = load_yfm(os.path.join(ROOT, "oracle", "model", "yoloface_int8.yfm"))
    return int(m["tensors"][m["input"]]["zp"])


@pytest.fixture(scope="module")
def batch(golden, zero_point):
    special = np.concatenate([structured_frames(zero_point), golden["inputs"]])
    n = max(BATCHES)
    x = np.random.default_rng(1010).integers(-128, 128, (n, 56, 56, 3), dtype=np.int8)
    k = len(special)
    assert k == 31 and 2 * k < 512
    x[2:2 + k] = special                           # the two-frame launches see them in their first groups,
    x[515 - k:515] = special                       # ... in the last groups of 513 and 515 (515: frame 514 is a group of its own)
    x[n - k:] = special                            # ... and in the last groups of 1030
    x[0] = special[4]                              # the one-frame launch: the centre tap of the even column's patch, and rows and columns 52-55
    x[1] = special[24]
    return x


@pytest.fixture(scope="module")
def camera(oracle):
    rng = np.random.default_rng(1011)
    base = rng.integers(0, 256, (N_CAM, 112 * 112 * 2), dtype=np.uint8)
    pick = np.arange(CAMERA_BATCH) * 7 % N_CAM                           # neighbours differ (7 and 24 are coprime)
    return dict(base=base, pick=pick, frames=np.stack([oracle.prepare_rgb565(r) for r in base]))


@pytest.fixture(scope="module")
def reference(oracle, batch, camera):
    return {name: dict(heads=oracle.run(batch, threads=16, variant=variant), cam=oracle.run(camera["frames"], threads=16, variant=variant))
            for name, variant in ROUNDINGS.items()}


@pytest.fixture(scope="module")
def gpu_results(batch, camera, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("lds_pitch")
    src, dst = str(tmp / "frames.npz"), str(tmp / "out.npz")
    np.savez(src, x=batch, raw=camera["base"][camera["pick"]])
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, src, dst, str(CAP), str(GUARD)], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return dict(np.load(dst))


def test_structured_frames_reach_the_heads(oracle, zero_point):
    """Every impulse frame and every edge frame gives heads that differ from the all-zero-point frame's, under each rounding, and no two of them give the
    same heads: the frames exercise what they are placed for."""
    frames = np.concatenate([np.full((1, 56, 56, 3), zero_point, np.int8), structured_frames(zero_point)])
    assert len(frames) == 1 + len(impulse_positions()) + 3
    for name, variant in ROUNDINGS.items():
        heads = oracle.run(frames, threads=8, variant=variant)
        same = [i for i in range(1, len(heads)) if np.array_equal(heads[i], heads[0])]
        assert not same, (name, same)
        assert len({h.tobytes() for h in heads}) == len(heads), name


def test_references_differ_between_the_roundings(reference):
    heads = [reference[name]["heads"] for name in sorted(ROUNDINGS)]
    assert not any(np.array_equal(heads[i], heads[j]) for i in range(3) for j in range(i))


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


@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("rounding", sorted(ROUNDINGS))
def test_heads_and_records_equal_the_oracle(yf, oracle, reference, gpu_results, rounding, n):
    kernel = str(gpu_results[f"{rounding}_{n}_kernel"])
    assert ("<F=1," in kernel) == (n == 2) and ("<F=2," in kernel) == (n > 2), kernel       # 2 frames: the one-frame kernel; the others: two frames per group
    check(yf, oracle, gpu_results, f"{rounding}_{n}", n, reference[rounding]["heads"][:n], oracle.decode_py)


@pytest.mark.parametrize("rounding", sorted(ROUNDINGS))
def test_camera_frames_equal_the_oracle(yf, oracle, reference, gpu_results, camera, rounding):
    check(yf, oracle, gpu_results, f"{rounding}_cam", CAMERA_BATCH, reference[rounding]["cam"][camera["pick"]], oracle.decode_c)
