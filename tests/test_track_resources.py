"""Static resources of the tracker's kernel, read off the built libyf_images.so (tools/isa_hashes.py): the kernel of namespace yftrack
exists, uses no scratch and spills no register, and the step body it shares with the other two trackers' kernels (namespace yfstep of
csrc/yf_images_step.hip.h) exists in the code object only inlined into those three.  Its VGPR count is recorded in profiles/track_bench.txt, not bounded here: what the float64
IoU costs has not been weighed against occupancy."""
import os
import sys

import pytest

from conftest import ROOT
from images_support import images          # noqa: F401 (fixture)

LLVM = "/opt/rocm/lib/llvm/bin"

pytestmark = pytest.mark.skipif(not all(os.path.exists(os.path.join(LLVM, t)) for t in ("llvm-objcopy", "llvm-objdump", "llvm-readelf", "clang-offload-bundler")),
                                reason="needs the ROCm LLVM tools")


def test_the_track_kernel_uses_no_scratch(images):
    images.load()                                 # builds the library if it is stale
    sys.path.insert(0, ROOT)
    from tools import isa_hashes
    res = {}
    code = isa_hashes.disassemble(images.lib_path(), res)
    # the step body the three trackers' kernels share (namespace yfstep) is inlined into them: the code object holds no function of that
    # namespace, and only those kernels name it at all (in the type of their argument)
    assert not [k for k in code if k.startswith("_ZN6yfstep")], sorted(code)
    shared = sorted(k for k in set(code) | set(res) if "yfstep" in k)
    assert len(shared) == 3 and all("step_kernel" in k and k in res for k in shared), shared
    assert [sum(name in k for k in shared) for name in ("yftrack", "yfmotion", "yfassign")] == [1, 1, 1], shared
    ours = [k for k in res if "yftrack" in k]
    assert len(ours) == 1 and "step_kernel" in ours[0], sorted(res)
    # tests/test_crops_resources.py and tests/test_redact_resources.py count their kernels by these names
    assert not any("yfcrop" in k or "yfredact" in k for k in ours)
    for k in ours:
        assert res[k]["private_segment_fixed_size"] == 0, (k, res[k])
        assert res[k]["sgpr_spill_count"] == 0 and res[k]["vgpr_spill_count"] == 0, (k, res[k])
        assert res[k]["group_segment_fixed_size"] == 0, (k, res[k])          # one wave, registers and cross-lane reads only
