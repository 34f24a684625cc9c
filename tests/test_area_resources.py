"""Static resources of the area kernels, read off the built libyf_images.so (tools/isa_hashes.py): the 18 kernels of namespace yfarea
exist -- one per format (the four packed ones, NV12, NV21) at 56, at 160 and as fp16 frames --, none of them uses scratch or spills a
register, each holds its tile of staged source rows (16 KB at 56, 32 KB at 160) and a pair of output rows in LDS, and no name contains a substring by which the
resource tests of the other stages count their kernels."""
import os
import re
import sys

import pytest

from conftest import ROOT
from images_support import images          # noqa: F401 (fixture)

LLVM = "/opt/rocm/lib/llvm/bin"

pytestmark = pytest.mark.skipif(not all(os.path.exists(os.path.join(LLVM, t)) for t in ("llvm-objcopy", "llvm-objdump", "llvm-readelf", "clang-offload-bundler")),
                                reason="needs the ROCm LLVM tools")


def test_the_area_kernels_use_no_scratch_and_spill_nothing(images):
    images.load()                                 # builds the library if it is stale
    sys.path.insert(0, ROOT)
    from tools import isa_hashes
    res = {}
    isa_hashes.disassemble(images.lib_path(), res)
    ours = sorted(k for k in res if "yfarea" in k)
    found = set()
    for k in ours:
        m = re.match(r"_ZN6yfarea11area_kernelILi(\d+)ELi(\d)E([at])EEvNS_4ArgsE$", k)
        assert m, k
        found.add((int(m.group(1)), int(m.group(2)), m.group(3)))
    assert len(ours) == 18 and found == {(out, fmt, elem) for out, elem in ((56, "a"), (160, "a"), (56, "t")) for fmt in range(6)}, ours
    # the resource tests of the other stages count their kernels by these names
    assert not any(name in k for k in ours for name in ("prepare_", "yfcrop", "yfredact", "yfblur", "yfdraw", "yftrack", "yffit")), ours
    for k in ours:
        print(f"{k}: {res[k]['vgpr_count']} VGPRs, {res[k]['sgpr_count']} SGPRs, {res[k]['group_segment_fixed_size']} B of LDS")
        assert res[k]["private_segment_fixed_size"] == 0, (k, res[k])
        assert res[k]["vgpr_spill_count"] == 0 and res[k]["sgpr_spill_count"] == 0, (k, res[k])
        side = int(re.match(r"_ZN6yfarea11area_kernelILi(\d+)E", k).group(1))
        tile = 16384 if side == 56 else 32768                                            # 256 / 512 threads: 32 waves per CU either way
        assert tile < res[k]["group_segment_fixed_size"] <= tile + tile // 4, (k, res[k])
