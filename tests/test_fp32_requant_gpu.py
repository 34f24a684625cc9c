"""YF_ROUND_FP32 on the GPU: the kernel set whose convolutions requantise in float32 (namespaces yfx / yf160x) against the oracle's statement of the
XNNPACK delegate's arithmetic (oracle variant X, YFO_RV_FP32), bit for bit, on every path that runs a convolution."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

FP32 = 0x10
RV_FP32 = 3                     # oracle/yf_oracle.h YFO_RV_FP32
STAGES = [("T1", 2), ("T2", 4), ("T3", 5), ("T4", 7), ("Q21", 21), ("T6", 11), ("T7", 12), ("T8", 14), ("T9", 16),
          ("T11", 18), ("T14", 22), ("T15", 24), ("Q45", 45), ("T17", 28), ("T18", 29), ("T19", 31), ("T20", 33),
          ("T22", 35), ("T23", 37), ("T24", 39), ("T26", 41), ("T30", 46), ("T31", 48), ("T32", 50), ("T33", 52),
          ("P8", 8), ("C17", 17), ("P25", 25), ("C34", 34), ("C40", 40), ("L43", 43)]     # the dump build's records, in order (test_gpu_parity.STAGES)
LAB_LIB = os.path.join(ROOT, "stm32h7-yolo_amd", "lib_lab", "libyf_network.so")
DET = lambda d: (int(d["anchor"]), int(d["row"]), int(d["col"]), int(d["x1"]), int(d["y1"]), int(d["x2"]), int(d["y2"]))   # noqa: E731
ORACLE_DET = lambda d: (d[1], d[2], d[3], d[6], d[7], d[8], d[9])                                                          # noqa: E731


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def rnd(seed, n):
    return np.random.default_rng(seed).integers(-128, 128, (n, 56, 56, 3), dtype=np.int8)


def test_fp32_requantisation_equals_the_oracle_variant(yf, network, oracle, golden, torch_cuda):
    """The six golden frames (== the committed golden_heads_variants.npz["X"]), the reference's 27 sample images and 4096 seeded frames with the fused
    decode; ai_network_run on host arrays; every fused stage through the dump build; a 160x160 block; 131 camera frames with firmware-mode records;
    ragged batches on both shapes.  Switching back to the reference rounding restores its kernels and heads bit for bit."""
    torch = torch_cuda
    real = np.fromfile(os.path.join(ROOT, "tests", "golden", "real_frames_56.bin"), np.int8).reshape(-1, 56, 56, 3)
    x = rnd(1, 4096)
    x[:6] = golden["inputs"]
    x[6:33] = real
    ref0 = oracle.run(x, threads=16)
    want = oracle.run(x, threads=16, variant=RV_FP32)
    assert not np.array_equal(want, ref0)
    assert network.requant_rounding == 0
    try:
        network.set_requant_rounding(yf.YF_ROUND_FP32)
        assert network.requant_rounding == FP32
        assert "fp32 requantisation" in network.kernel_name and "fp32 requantisation" in network.kernel_name_for(5)
        assert network.kernel_name != network.kernel_name_for(5)                            # <2,8> and the small-batch <1,8> of the same set
        d_in = torch.from_numpy(x).cuda()
        d_out = torch.zeros((4096, 7, 7, 18), dtype=torch.int8, device="cuda")
        cap = 4
        d_d = torch.zeros((4096, cap, 28), dtype=torch.uint8, device="cuda")
        d_c = torch.zeros((4096,), dtype=torch.int32, device="cuda")
        network.run_decode_device(d_in.data_ptr(), d_out.data_ptr(), 4096, d_d.data_ptr(), d_c.data_ptr(), cap, 0)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        assert np.array_equal(got, want)
        assert np.array_equal(got[:6], np.load(os.path.join(ROOT, "tests", "golden", "golden_heads_variants.npz"))["X"])     # the committed fixture
        counts, buf = d_c.cpu().numpy(), d_d.cpu().numpy().view(yf.DET_DTYPE).reshape(4096, cap)
        for f in list(range(40)) + list(np.nonzero(counts)[0][:200]):
            py = oracle.decode_py(want[f], f)
            assert counts[f] == len(py)
            assert [DET(d) for d in buf[f, :min(cap, counts[f])]] == [ORACLE_DET(d) for d in py][:cap]
        # the host path (small batches: one frame per workgroup), and every fused stage through the dump build
        assert np.array_equal(network.run(x[:33]), want[:33])
        from oracle.np_restatement import load_yfm
        m = load_yfm(os.path.join(ROOT, "oracle", "model", "yoloface_int8.yfm"))
        sizes = [int(np.prod(m["tensors"][o["out"]]["shape"][1:])) for o in m["ops"]]
        offs = np.concatenate([[0], np.cumsum(sizes)])
        _, dump_ref = oracle.run(x[4:9], dump=True, variant=RV_FP32)
        d_dump = torch.zeros((5, network.dump_bytes()), dtype=torch.int8, device="cuda")
        network.run_device(d_in[4:9].data_ptr(), d_out.data_ptr(), 5, None, d_dump.data_ptr())
        torch.cuda.synchronize()
        dump, off = d_dump.cpu().numpy(), 0
        for name, op in STAGES:
            assert np.array_equal(dump[:, off:off + sizes[op]], dump_ref[:, offs[op]:offs[op] + sizes[op]]), f"stage {name} (tflite op {op})"
            off += sizes[op]
        # 160x160: the banded kernels of the fp32 set
        block = np.random.default_rng(4).integers(-128, 128, (3, 160, 160, 3), dtype=np.int8)
        d_b = torch.from_numpy(block).cuda()
        d_o = torch.zeros((3, 20, 20, 18), dtype=torch.int8, device="cuda")
        network.run_device_hw(160, 160, d_b.data_ptr(), d_o.data_ptr(), 3)
        torch.cuda.synchronize()
        assert np.array_equal(d_o.cpu().numpy(), oracle.run(block, threads=3, variant=RV_FP32))
        # camera frames -> heads + firmware-mode records in one launch
        raw = np.random.default_rng(34).integers(0, 256, (131, 112 * 112 * 2), dtype=np.uint8)
        cam_ref = oracle.run(np.stack([oracle.prepare_rgb565(r) for r in raw]), threads=8, variant=RV_FP32)
        d_raw = torch.from_numpy(raw).cuda()
        d_ch = torch.zeros((131, 7, 7, 18), dtype=torch.int8, device="cuda")
        d_cd = torch.zeros((131, cap, 28), dtype=torch.uint8, device="cuda")
        d_cc = torch.zeros((131,), dtype=torch.int32, device="cuda")
        network.run_camera_device(d_raw.data_ptr(), d_ch.data_ptr(), 131, d_cd.data_ptr(), d_cc.data_ptr(), cap, yf.YF_DECODE_FW)
        torch.cuda.synchronize()
        assert np.array_equal(d_ch.cpu().numpy(), cam_ref)
        cc, cbuf = d_cc.cpu().numpy(), d_cd.cpu().numpy().view(yf.DET_DTYPE).reshape(131, cap)
        for f in range(131):
            fw = oracle.decode_c(cam_ref[f], f)
            assert cc[f] == len(fw) and [DET(d) for d in cbuf[f, :min(cap, cc[f])]] == [ORACLE_DET(d) for d in fw][:cap]
        # ragged batches on both shapes; nothing written behind the batch
        for shape in ((2, 8), (1, 8)):
            network.configure(*shape)
            assert "fp32 requantisation" in network.kernel_name
            for nn in (1, 7, 513, 1027):
                d_r = torch.full((nn + 1, 7, 7, 18), 77, dtype=torch.int8, device="cuda")
                network.run_device(d_in.data_ptr(), d_r.data_ptr(), nn)
                torch.cuda.synchronize()
                r_got = d_r.cpu().numpy()
                assert np.array_equal(r_got[:nn], want[:nn]) and (r_got[nn] == 77).all(), (shape, nn)
        network.configure(-1, -1)
        with pytest.raises(Exception) as ei:
            network.set_requant_rounding(FP32 | yf.YF_ROUND_GENERIC_KERNELS)
        assert ei.value.type == 0x14 and network.requant_rounding == FP32               # AI_ERROR_INVALID_PARAM latched, nothing changed
    finally:
        network.configure(-1, -1)
        network.set_requant_rounding(0)
    assert "fp32" not in network.kernel_name and "fp32" not in network.kernel_name_for(5)
    network.run_device(d_in.data_ptr(), d_out.data_ptr(), 4096)
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), ref0)


def test_fp32_from_the_environment(oracle, golden):
    """$YF_REQUANT_ROUNDING=fp32 steers an unmodified caller (create + init back to back) onto the fp32 set; fp32+generic fails ai_network_init like an
    unknown word.  Fresh processes: the variable is read by ai_network_create."""
    code = ("import sys, importlib, numpy as np\nsys.path.insert(0, %r)\nyf = importlib.import_module('stm32h7-yolo_amd')\n"
            "x = np.fromfile(%r, np.int8).reshape(-1, 56, 56, 3)\n"
            "try:\n    net = yf.Network(device=0).init()\nexcept Exception as e:\n    print('INIT FAILED', e); sys.exit(3)\n"
            "print(net.requant_rounding, net.kernel_name.replace(' ', '_')); sys.stdout.flush(); sys.stdout.buffer.write(net.run(x).tobytes())\n") % (
        ROOT, os.path.join(ROOT, "tests", "golden", "golden_inputs.bin"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, timeout=300, env=dict(os.environ, YF_REQUANT_ROUNDING="fp32"))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    head, _, raw = r.stdout.partition(b"\n")
    value, name = head.split()
    assert int(value) == FP32 and b"fp32_requantisation" in name
    assert np.array_equal(np.frombuffer(raw, np.int8).reshape(-1, 7, 7, 18), oracle.run(golden["inputs"], variant=RV_FP32))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, timeout=300, env=dict(os.environ, YF_REQUANT_ROUNDING="fp32+generic"))
    assert r.returncode == 3 and b"YF_REQUANT_ROUNDING" in r.stdout and b"fp32" in r.stdout, r.stdout + r.stderr


@pytest.mark.skipif(not os.path.exists(LAB_LIB), reason="the lab library is not built (make -C stm32h7-yolo_amd/csrc lab)")
def test_lab_forms_without_an_fp32_build_refuse(golden):
    """The laboratory's layer-by-layer 160x160 form and its production-order dump build exist for the integer epilogues only: under YF_ROUND_FP32 they
    latch an error instead of running kernels that would read the float32 constants as integer ones.  Fresh processes with the lab library."""
    code = ("import sys, importlib, numpy as np, torch\nsys.path.insert(0, %r)\nyf = importlib.import_module('stm32h7-yolo_amd')\n"
            "net = yf.Network(device=0).init(); net.set_requant_rounding(yf.YF_ROUND_FP32)\n"
            "x = torch.zeros((2, 160, 160, 3), dtype=torch.int8, device='cuda'); o = torch.zeros((2, 20, 20, 18), dtype=torch.int8, device='cuda')\n"
            "d = torch.zeros((2, net.dump_bytes()), dtype=torch.int8, device='cuda')\n"
            "try:\n    net.run_device_hw(160, 160, x.data_ptr(), o.data_ptr(), 2) if sys.argv[1] == 'hw' else net.run_device(x.data_ptr(), o.data_ptr(), 2, None, d.data_ptr())\n"
            "except Exception as e:\n    print('REFUSED', e); sys.exit(0)\n"
            "print('RAN'); sys.exit(1)\n") % ROOT
    for form, env in (("hw", {"YF_160_LAYERWISE": "1"}), ("dump", {"YF_LAB_DUMP_PROD_ORDER": "1"})):
        r = subprocess.run([sys.executable, "-c", code, form], capture_output=True, text=True, timeout=300, env=dict(os.environ, YF_LIB_PATH=LAB_LIB, **env))
        assert r.returncode == 0 and "REFUSED" in r.stdout, (form, r.stdout + r.stderr[-2000:])
