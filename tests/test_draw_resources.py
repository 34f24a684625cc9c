"""Static resources of the drawing kernels, read off the built libyf_images.so (tools/isa_hashes.py): the four kernels of namespace yfdraw
exist -- the outline for pixels of 3 and of 4 bytes and for NV12 and NV21 surfaces --, none of them uses scratch, each stays within 64
VGPRs and below 16 KB of LDS, the crop and redaction kernels' bounds."""
import os
import sys

import pytest

from conftest import ROOT
from images_support import images          # noqa: F401 (fixture)

LLVM = "/opt/rocm/lib/llvm/bin"

pytestmark = pytest.mark.skipif(not all(os.path.exists(os.path.join(LLVM, t)) for t in ("llvm-objcopy", "llvm-objdump", "llvm-readelf", "clang-offload-bundler")),
                                reason="needs the ROCm LLVM tools")


def test_the_drawing_kernels_use_no_scratch(images):
    images.load()                                 # builds the library if it is stale
    sys.path.insert(0, ROOT)
    from tools import isa_hashes
    res = {}
    isa_hashes.disassemble(images.lib_path(), res)
    ours = [k for k in res if "yfdraw" in k]
    count = lambda part: len([k for k in ours if part in k])
    assert len(ours) == 4, sorted(res)
    assert (count("outline_kernel"), count("outline_yuv_kernel")) == (2, 2), ours
    assert not any("yfcrop" in k or "yfredact" in k for k in ours)   # the crop and redaction tests count their kernels by those names
    for k in ours:
        assert res[k]["private_segment_fixed_size"] == 0, (k, res[k])
        assert res[k]["vgpr_count"] <= 64, (k, res[k])            # eight waves per SIMD stay possible (512 VGPRs / 64)
        assert res[k]["group_segment_fixed_size"] < 16384, (k, res[k])
