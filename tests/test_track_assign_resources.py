"""Static resources of the kernel of the optimal assignment, read off the built libyf_images.so (tools/isa_hashes.py): exactly one kernel
of namespace yfassign exists, it uses no scratch and spills no register, and its LDS is the 16 KB table of weights (64 detections x 64
slots of int32) and nothing else -- the design has no other table.  The two trackers' kernels are still the only ones of their
namespaces.  Its register counts are recorded in profiles/track_assign_bench.txt, not bounded here."""
import os
import sys

import pytest

from conftest import ROOT
from images_support import images          # noqa: F401 (fixture)

LLVM = "/opt/rocm/lib/llvm/bin"

pytestmark = pytest.mark.skipif(not all(os.path.exists(os.path.join(LLVM, t)) for t in ("llvm-objcopy", "llvm-objdump", "llvm-readelf", "clang-offload-bundler")),
                                reason="needs the ROCm LLVM tools")


def test_the_assign_kernel_uses_no_scratch_and_16_kb_of_lds(images):
    images.load()                                 # builds the library if it is stale
    sys.path.insert(0, ROOT)
    from tools import isa_hashes
    res = {}
    isa_hashes.disassemble(images.lib_path(), res)
    ours = [k for k in res if "yfassign" in k]
    assert len(ours) == 1 and "step_kernel" in ours[0], sorted(res)
    # the other stages' resource tests count their kernels by these names
    assert not any(name in ours[0] for name in ("yftrack", "yfmotion", "yfcrop", "yfredact", "yfblur", "yfdraw", "yffit", "yfarea"))
    assert len([k for k in res if "yftrack" in k]) == 1 and len([k for k in res if "yfmotion" in k]) == 1
    k = ours[0]
    assert res[k]["private_segment_fixed_size"] == 0, (k, res[k])
    assert res[k]["sgpr_spill_count"] == 0 and res[k]["vgpr_spill_count"] == 0, (k, res[k])
    assert 0 < res[k]["group_segment_fixed_size"] <= 16384, (k, res[k])        # the table of weights alone: no small tables beside it
