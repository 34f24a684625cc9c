"""Static resources of the blur kernels, read off the built libyf_images.so (tools/isa_hashes.py): the six kernels of namespace yfblur
exist -- the means and the paint, each for pixels of 3 and of 4 bytes and for NV12 / NV21 surfaces (one kernel: the blur does not care
which of U and V comes first, and its fill takes the bytes in memory order) --, none of them uses scratch, and each stays within 64 VGPRs
and below 16 KB of LDS, the redaction's bounds."""
import os
import sys

import pytest

from conftest import ROOT
from images_support import images          # noqa: F401 (fixture)

LLVM = "/opt/rocm/lib/llvm/bin"

pytestmark = pytest.mark.skipif(not all(os.path.exists(os.path.join(LLVM, t)) for t in ("llvm-objcopy", "llvm-objdump", "llvm-readelf", "clang-offload-bundler")),
                                reason="needs the ROCm LLVM tools")


def test_the_blur_kernels_use_no_scratch(images):
    images.load()                                 # builds the library if it is stale
    sys.path.insert(0, ROOT)
    from tools import isa_hashes
    res = {}
    isa_hashes.disassemble(images.lib_path(), res)
    ours = [k for k in res if "yfblur" in k]
    count = lambda part: len([k for k in ours if part in k])
    assert len(ours) == 6, sorted(res)
    assert (count("means_kernel"), count("paint_kernel")) == (3, 3), ours
    # the resource tests of the other stages count their kernels by these names
    assert not any(name in k for k in ours for name in ("yfcrop", "yfredact", "yfdraw", "yftrack")), ours
    for k in ours:
        assert res[k]["private_segment_fixed_size"] == 0, (k, res[k])
        assert res[k]["vgpr_count"] <= 64, (k, res[k])            # eight waves per SIMD stay possible (512 VGPRs / 64)
        assert res[k]["group_segment_fixed_size"] < 16384, (k, res[k])
