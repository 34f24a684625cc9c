"""Static resources of the kernels of the appearance descriptors and of the re-identification, read off the built libyf_images.so
(tools/isa_hashes.py): exactly one kernel of namespace yfreid exists and the five of yfdescribe (BGR, RGB, BGRA, RGBA, surfaces); none
uses scratch or spills a register; yfreid's LDS is at most the 16 KB table of distances (64 records x 64 entries of int32) and 4 KB.  The
other stages' namespaces hold as many kernels as before.  The register counts are recorded in profiles/reid_bench.txt, not bounded here."""
import os
import sys

import pytest

from conftest import ROOT
from images_support import images          # noqa: F401 (fixture)

LLVM = "/opt/rocm/lib/llvm/bin"
# the kernels of every other namespace of the library, as they were counted before these two were added
OTHERS = {"yftrack": 1, "yfmotion": 1, "yfassign": 1, "yfscore": 1, "yfcrop": 9, "yfredact": 7, "yfblur": 6, "yfdraw": 4, "yffit": 21, "yfarea": 18}

pytestmark = pytest.mark.skipif(not all(os.path.exists(os.path.join(LLVM, t)) for t in ("llvm-objcopy", "llvm-objdump", "llvm-readelf", "clang-offload-bundler")),
                                reason="needs the ROCm LLVM tools")


def test_the_reid_and_describe_kernels_use_no_scratch_and_the_others_are_as_many_as_before(images):
    images.load()                                 # builds the library if it is stale
    sys.path.insert(0, ROOT)
    from tools import isa_hashes
    res = {}
    isa_hashes.disassemble(images.lib_path(), res)
    reid = [k for k in res if "yfreid" in k]
    describe = [k for k in res if "yfdescribe" in k]
    assert len(reid) == 1 and "stream_kernel" in reid[0], sorted(res)
    assert len(describe) == 5 and all("records_kernel" in k for k in describe), sorted(res)
    # the other stages' resource tests count their kernels by these names
    assert not any(name in k for k in reid + describe for name in OTHERS)
    assert {name: len([k for k in res if name in k]) for name in OTHERS} == OTHERS
    for k in reid + describe:
        assert res[k]["private_segment_fixed_size"] == 0, (k, res[k])
        assert res[k]["sgpr_spill_count"] == 0 and res[k]["vgpr_spill_count"] == 0, (k, res[k])
    assert 0 < res[reid[0]]["group_segment_fixed_size"] <= 16384 + 4096, (reid[0], res[reid[0]])
    assert all(0 < res[k]["group_segment_fixed_size"] <= 1024 for k in describe), [res[k] for k in describe]
