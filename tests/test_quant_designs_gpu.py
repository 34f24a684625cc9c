"""The designed quantisations (tests/quant_designs.py) on the GPU: every (design, rounding) the host admits -- reference, ties_up, single and fp32, so
all three kernel sets and both forms of C64 -- against Oracle(design.yfm) in the matching oracle variant, bit for bit: run_device at n = 1, 5 and 67 with a
guard frame, the dump build stage by stage (a failure names the first wrong stage, pixel and channel: a design's target tensor is compared directly, not
through what survives to the heads), the 160x160 band kernels, the camera entry.  The designs with a zero point at an end of int8 also run 1024 frames at
160x160, where every workgroup of the band kernels takes a second job and meets the halo the job before left.  tests/test_quant_designs_host.py shows on
the CPU that each design's bound stands in the tables these kernels read and that the designs are live."""
import numpy as np
import pytest

import model_variants as mv
import quant_designs as qd
from test_model_file_gpu import torch_cuda, frames, bind, assert_network_equals_oracle, _assert_heads      # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
ORACLE_VARIANT = {qd.REF: 0, qd.TIES_UP: 1, qd.SINGLE: 4, qd.FP32: 3}
CASES = [(d.name, r) for d in qd.DESIGNS for r in qd.ROUNDINGS if d.admitted(r)]
REUSE_N = 1024                              # every workgroup of every band kernel takes a second job (tests/test_band160_reuse_gpu.py asserts it of the device)
REUSE_CASES = [(name, r) for name in ("Z0", "Z255", "ZIN127", "ZINm128") for r in (qd.REF, qd.TIES_UP, qd.FP32)]      # once per kernel set


@pytest.fixture(scope="module")
def oracles(tmp_path_factory):
    from oracle.oracle import Oracle
    d = tmp_path_factory.mktemp("designs_gpu")
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Oracle(qd.BY_NAME[name].write(d)) if name != "S" else Oracle()
        return cache[name]
    return get


@pytest.fixture(scope="module")
def frames_160(torch_cuda):
    x = mv.reuse_frames_160(REUSE_N)
    return dict(x=x, d_x=torch_cuda.from_numpy(x).cuda())


@pytest.mark.parametrize("name,rounding", CASES, ids=[f"{n}-{mv.rounding_name(r)}" for n, r in CASES])
def test_design_equals_its_oracle(network, bind, oracles, frames, torch_cuda, name, rounding):
    what = f"design {name} ({qd.BY_NAME[name].bound}), rounding {mv.rounding_name(rounding)}"
    bind("design " + name, rounding, qd.build(name))
    assert ("sign-free" in network.kernel_name) == (rounding in (qd.TIES_UP, qd.SINGLE)), what
    assert_network_equals_oracle(torch_cuda, network, oracles(name), ORACLE_VARIANT[rounding], frames, what, oracles("S"), fp32=rounding == qd.FP32,
                                 stages_first=True)


@pytest.mark.parametrize("name,rounding", REUSE_CASES, ids=[f"{n}-{mv.rounding_name(r)}" for n, r in REUSE_CASES])
def test_zero_point_designs_with_several_band_jobs_per_workgroup(network, bind, oracles, frames_160, torch_cuda, name, rounding):
    """n = 1024 at 160x160 (after the frames' complements on the same stream: tests/model_variants.py, run_160_after_complement): a workgroup's second job
    starts on LDS rows and halo columns its first job left, filled with a zero point of 127 or -128"""
    what = f"design {name}, rounding {mv.rounding_name(rounding)}, {REUSE_N} frames at 160x160"
    bind("design " + name, rounding, qd.build(name))
    ref = oracles(name).run(frames_160["x"], threads=16, variant=ORACLE_VARIANT[rounding])
    got = mv.run_160_after_complement(torch_cuda, network, frames_160["d_x"], REUSE_N)
    _assert_heads(got, ref, what, (20, 20, 18))
