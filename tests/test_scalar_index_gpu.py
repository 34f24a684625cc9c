"""The fused 56x56 kernel counts groups and frames in 32 bits and addresses global memory as one scalar base plus a 32-bit lane offset (input staging,
constant fetches, the T15 park and its way back, head and record stores).  Network(frames_per_wg=2, waves_per_wg=8) on the product's full grid -- the
512 workgroups of a 256-CU device; the case descriptions below hold there, and the expected results on a grid of any size -- heads, detection records and
counts against the oracle, under the reference rounding and `ties_up`, on the smallest batches at which that index code takes each of its paths:

    2049 frames  1025 groups: workgroup 0 has a pair of groups plus an unpaired last group that holds ONE frame, all others one pair
    1026 frames  513 groups: workgroup 0 has a pair, every other workgroup one unpaired group (nothing is parked)
    1023 frames  an odd last frame on an unpaired group
    1025 camera frames (112x112 RGB565 in, firmware-mode records): the camera-input build of the same kernel

Every batch runs with the fused decode and, the int8 batches, without it as well (the head copy then runs on all waves).  Frames are drawn from 48
distinct ones, so the oracle runs on 48 frames per rounding; neighbours differ, which is what a wrong frame number would show on.  The launches run in one
child process under a time limit; the comparisons run here."""
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

INT8_BATCHES = (2049, 1026, 1023)
CAMERA_BATCH = 1025
ROUNDINGS = {"tflite_ref": 0, "ties_up": 1}                     # name: the oracle's variant
N_BASE, CAP, GUARD = 48, 4, 0x4D
DET = lambda d: (int(d["anchor"]), int(d["row"]), int(d["col"]), int(d["x1"]), int(d["y1"]), int(d["x2"]), int(d["y2"]))   # noqa: E731
ORACLE_DET = lambda d: (d[1], d[2], d[3], d[6], d[7], d[8], d[9])                                                          # noqa: E731

CHILD = r"""
import sys, importlib, numpy as np, torch
sys.path.insert(0, sys.argv[1])
yf = importlib.import_module('stm32h7-yolo_amd')
z = np.load(sys.argv[2])
cap, guard = int(sys.argv[4]), int(sys.argv[5])
net = yf.Network(device=0, frames_per_wg=2, waves_per_wg=8).init()
d_x, d_raw = torch.from_numpy(z['x']).cuda(), torch.from_numpy(z['raw']).cuda()
out = {}
def bufs(n):
    return (torch.full((n + 1, 7, 7, 18), guard, dtype=torch.int8, device='cuda'), torch.full((n + 1, cap, 28), guard, dtype=torch.uint8, device='cuda'),
            torch.full((n + 1,), guard, dtype=torch.int32, device='cuda'))
for name, rounding in (('tflite_ref', yf.YF_ROUND_TFLITE_REF), ('ties_up', yf.YF_ROUND_TIES_UP)):
    net.set_requant_rounding(rounding)
    for n in (2049, 1026, 1023):
        d_h, d_d, d_c = bufs(n)
        net.run_decode_device(d_x.data_ptr(), d_h.data_ptr(), n, d_d.data_ptr(), d_c.data_ptr(), cap, yf.YF_DECODE_PY)
        torch.cuda.synchronize()
        out[f'{name}_{n}_heads'], out[f'{name}_{n}_dets'], out[f'{name}_{n}_counts'] = d_h.cpu().numpy(), d_d.cpu().numpy(), d_c.cpu().numpy()
        out[f'{name}_{n}_kernel'] = np.array(net.kernel_name_for(n))
        d_h.fill_(guard)
        net.run_device(d_x.data_ptr(), d_h.data_ptr(), n)
        torch.cuda.synchronize()
        out[f'{name}_{n}_heads_only'] = d_h.cpu().numpy()
    n = 1025
    d_h, d_d, d_c = bufs(n)
    net.run_camera_device(d_raw.data_ptr(), d_h.data_ptr(), n, d_d.data_ptr(), d_c.data_ptr(), cap, yf.YF_DECODE_FW)
    torch.cuda.synchronize()
    out[f'{name}_cam_heads'], out[f'{name}_cam_dets'], out[f'{name}_cam_counts'] = d_h.cpu().numpy(), d_d.cpu().numpy(), d_c.cpu().numpy()
net.destroy()
np.savez(sys.argv[3], **out)
"""


@pytest.fixture(scope="module")
def frames(golden):
    rng = np.random.default_rng(909)
    base = rng.integers(-128, 128, (N_BASE, 56, 56, 3), dtype=np.int8)
    base[:len(golden["inputs"])] = golden["inputs"]
    cam = rng.integers(0, 256, (N_BASE, 112 * 112 * 2), dtype=np.uint8)
    n = max(INT8_BATCHES)
    pick = rng.integers(0, N_BASE, n)
    pick[1:] += (pick[1:] == pick[:-1])                         # (mostly) no frame equals its predecessor; exactly so after the next line
    pick %= N_BASE
    for i in range(1, n):
        if pick[i] == pick[i - 1]:
            pick[i] = (pick[i] + 1) % N_BASE
    return dict(base=base, cam=cam, pick=pick)


@pytest.fixture(scope="module")
def reference(oracle, frames):
    ref = {}
    for name, variant in ROUNDINGS.items():
        heads = oracle.run(frames["base"], threads=16, variant=variant)
        cam_heads = oracle.run(np.stack([oracle.prepare_rgb565(r) for r in frames["cam"]]), threads=16, variant=variant)
        ref[name] = dict(heads=heads, dets=[[ORACLE_DET(d) for d in oracle.decode_py(h, 0)] for h in heads],
                         cam_heads=cam_heads, cam_dets=[[ORACLE_DET(d) for d in oracle.decode_c(h, 0, 147)] for h in cam_heads])
    return ref


@pytest.fixture(scope="module")
def gpu_results(frames, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("scalar_index")
    src, dst = str(tmp / "frames.npz"), str(tmp / "out.npz")
    np.savez(src, x=frames["base"][frames["pick"]], raw=frames["cam"][frames["pick"][:CAMERA_BATCH]])
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, src, dst, str(CAP), str(GUARD)], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return dict(np.load(dst))


def check(yf, heads, dets, counts, n, want_heads, want_dets, pick):
    bad = np.nonzero((heads[:n] != want_heads[pick[:n]]).reshape(n, -1).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} frames differ, first {bad[:8]}"
    assert (heads[n] == GUARD).all() and (dets[n] == GUARD).all() and counts[n] == GUARD       # nothing behind the batch
    rec = dets.view(yf.DET_DTYPE).reshape(n + 1, CAP)
    assert np.array_equal(counts[:n], np.array([len(want_dets[p]) for p in pick[:n]]))
    for f in range(n):
        k = min(CAP, counts[f])
        assert [DET(d) for d in rec[f, :k]] == want_dets[pick[f]][:CAP], f
        assert (rec[f, :k]["frame"] == f).all(), f
        assert (dets[f, k:] == GUARD).all(), f                                                    # no record past the frame's count


def test_the_references_tell_the_roundings_and_the_frames_apart(reference):
    assert not np.array_equal(reference["tflite_ref"]["heads"], reference["ties_up"]["heads"])
    assert len({h.tobytes() for h in reference["tflite_ref"]["heads"]}) == N_BASE
    assert sum(len(d) for d in reference["tflite_ref"]["dets"]) > 0 and sum(len(d) for d in reference["tflite_ref"]["cam_dets"]) > 0


@pytest.mark.parametrize("n", INT8_BATCHES)
@pytest.mark.parametrize("rounding", sorted(ROUNDINGS))
def test_heads_records_and_counts_equal_the_oracle(yf, frames, reference, gpu_results, rounding, n):
    kernel = str(gpu_results[f"{rounding}_{n}_kernel"])
    assert "<F=2,NW=8" in kernel.replace(" ", ""), kernel
    ref = reference[rounding]
    check(yf, gpu_results[f"{rounding}_{n}_heads"], gpu_results[f"{rounding}_{n}_dets"], gpu_results[f"{rounding}_{n}_counts"], n, ref["heads"], ref["dets"],
          frames["pick"])
    only = gpu_results[f"{rounding}_{n}_heads_only"]
    assert np.array_equal(only[:n], ref["heads"][frames["pick"][:n]]) and (only[n] == GUARD).all()


@pytest.mark.parametrize("rounding", sorted(ROUNDINGS))
def test_camera_frames_equal_the_oracle(yf, frames, reference, gpu_results, rounding):
    ref = reference[rounding]
    check(yf, gpu_results[f"{rounding}_cam_heads"], gpu_results[f"{rounding}_cam_dets"], gpu_results[f"{rounding}_cam_counts"], CAMERA_BATCH,
          ref["cam_heads"], ref["cam_dets"], frames["pick"])
