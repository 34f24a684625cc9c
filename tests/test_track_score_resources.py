"""Static resources of the kernel of the score of tracks, read off the built libyf_images.so (tools/isa_hashes.py): exactly one kernel of
namespace yfscore exists, it uses no scratch and spills no register, and its LDS is at most the 16 KB table of weights (64 rows x 64
columns of int32) and 3 KB of per-object tables.  The three trackers' kernels are still the only ones of their namespaces.  Its register
counts are recorded in profiles/track_score_bench.txt, not bounded here."""
import os
import sys

import pytest

from conftest import ROOT
from images_support import images          # noqa: F401 (fixture)

LLVM = "/opt/rocm/lib/llvm/bin"

pytestmark = pytest.mark.skipif(not all(os.path.exists(os.path.join(LLVM, t)) for t in ("llvm-objcopy", "llvm-objdump", "llvm-readelf", "clang-offload-bundler")),
                                reason="needs the ROCm LLVM tools")


def test_the_score_kernel_uses_no_scratch_and_at_most_19_kb_of_lds(images):
    images.load()                                 # builds the library if it is stale
    sys.path.insert(0, ROOT)
    from tools import isa_hashes
    res = {}
    isa_hashes.disassemble(images.lib_path(), res)
    ours = [k for k in res if "yfscore" in k]
    assert len(ours) == 1 and "clip_kernel" in ours[0], sorted(res)
    # the other stages' resource tests count their kernels by these names
    assert not any(name in ours[0] for name in ("yftrack", "yfmotion", "yfassign", "yfcrop", "yfredact", "yfblur", "yfdraw", "yffit", "yfarea"))
    assert all(len([k for k in res if name in k]) == 1 for name in ("yftrack", "yfmotion", "yfassign"))
    k = ours[0]
    assert res[k]["private_segment_fixed_size"] == 0, (k, res[k])
    assert res[k]["sgpr_spill_count"] == 0 and res[k]["vgpr_spill_count"] == 0, (k, res[k])
    assert 0 < res[k]["group_segment_fixed_size"] <= 16384 + 3072, (k, res[k])
