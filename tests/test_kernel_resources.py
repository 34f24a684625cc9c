"""Static resources of the product's fused 56x56 kernel (F = 2, NW = 8) in each of the three kernel sets, read off the built library's disassembly
and code-object metadata (tools/isa_hashes.py): what the vector port executes that is not the network.

  * SGPRs parked in VGPR lanes (v_readlane_b32 / v_writelane_b32) between the group loop's first and last barrier: the parent of round 9 had 132 / 98 / 76
    of them (yf / yfu / yfx); round 9 reaches 17 / 17 / 0.  The survivors are named in profiles/EXPERIMENTS.md (round 9); the bound is the count reached.
  * no 64-bit compare on the vector port: group and frame numbers are 32-bit inside the kernel (the scalar unit has no ordered 64-bit compare).
  * no 64-bit lane arithmetic for addresses (v_lshl_add_u64): every global access is a scalar base plus a 32-bit lane offset.
  * NumVgprs <= 128 and no more scratch than the parent had (8 / 0 / 0 bytes)."""
import os
import re
import sys

import pytest

from conftest import ROOT

LLVM = "/opt/rocm/lib/llvm/bin"
SETS = {"yf": "_ZN2yf16", "yfu": "_ZN3yfu16", "yfx": "_ZN3yfx16"}
LANE_MOVES_IN_LOOP = {"yf": 17, "yfu": 17, "yfx": 0}
SCRATCH = {"yf": 8, "yfu": 0, "yfx": 0}

pytestmark = pytest.mark.skipif(not all(os.path.exists(os.path.join(LLVM, t)) for t in ("llvm-objcopy", "llvm-objdump", "llvm-readelf", "clang-offload-bundler")),
                                reason="needs the ROCm LLVM tools")


@pytest.fixture(scope="module")
def kernels(yf):
    yf.load()                                     # builds the library if it is stale
    sys.path.insert(0, ROOT)
    from tools import isa_hashes
    res = {}
    body = isa_hashes.disassemble(os.path.join(ROOT, "stm32h7-yolo_amd", "lib", "libyf_network.so"), res)
    out = {}
    for name, prefix in SETS.items():
        k = prefix + "yoloface56_fusedILi2ELi8ELb0ELb0EEEvNS_9NetParamsE"
        assert k in body and k in res, k
        out[name] = (body[k], res[k])
    return out


@pytest.mark.parametrize("kset", sorted(SETS))
def test_few_sgprs_parked_in_vgpr_lanes_inside_the_group_loop(kernels, kset):
    ins, _ = kernels[kset]
    bars = [i for i, x in enumerate(ins) if x.startswith("s_barrier")]
    assert len(bars) == 26, len(bars)              # the loop-top barrier and one behind each of the 25 stages of a group
    moves = [x for x in ins[bars[0]:bars[-1]] if x.startswith(("v_readlane_b32", "v_writelane_b32"))]
    assert LANE_MOVES_IN_LOOP[kset] < 20
    assert len(moves) <= LANE_MOVES_IN_LOOP[kset], (len(moves), moves)


@pytest.mark.parametrize("kset", sorted(SETS))
def test_no_64_bit_compares_or_lane_address_arithmetic(kernels, kset):
    ins, _ = kernels[kset]
    assert [x for x in ins if re.match(r"v_cmpx?_\w+_[iu]64", x)] == []
    assert [x for x in ins if x.startswith("v_lshl_add_u64")] == []


@pytest.mark.parametrize("kset", sorted(SETS))
def test_registers_and_scratch(kernels, kset):
    _, res = kernels[kset]
    assert res["vgpr_count"] <= 128
    assert res["private_segment_fixed_size"] <= SCRATCH[kset]
