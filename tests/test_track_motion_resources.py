"""Static resources of the kernel of the tracker with a motion model, read off the built libyf_images.so (tools/isa_hashes.py): exactly one
kernel of namespace yfmotion exists, it uses no scratch and spills no register, and the base tracker's kernel is still the only one of
namespace yftrack.  Its VGPR count is recorded in profiles/track_motion_bench.txt, not bounded here."""
import os
import sys

import pytest

from conftest import ROOT
from images_support import images          # noqa: F401 (fixture)

LLVM = "/opt/rocm/lib/llvm/bin"

pytestmark = pytest.mark.skipif(not all(os.path.exists(os.path.join(LLVM, t)) for t in ("llvm-objcopy", "llvm-objdump", "llvm-readelf", "clang-offload-bundler")),
                                reason="needs the ROCm LLVM tools")


def test_the_motion_kernel_uses_no_scratch(images):
    images.load()                                 # builds the library if it is stale
    sys.path.insert(0, ROOT)
    from tools import isa_hashes
    res = {}
    isa_hashes.disassemble(images.lib_path(), res)
    ours = [k for k in res if "yfmotion" in k]
    assert len(ours) == 1 and "step_kernel" in ours[0], sorted(res)
    # the other stages' resource tests count their kernels by these names
    assert not any(name in ours[0] for name in ("yftrack", "yfcrop", "yfredact", "yfblur", "yfdraw", "yffit", "yfarea"))
    assert len([k for k in res if "yftrack" in k]) == 1
    k = ours[0]
    assert res[k]["private_segment_fixed_size"] == 0, (k, res[k])
    assert res[k]["sgpr_spill_count"] == 0 and res[k]["vgpr_spill_count"] == 0, (k, res[k])
    assert res[k]["group_segment_fixed_size"] == 0, (k, res[k])              # one wave, registers and cross-lane reads only
