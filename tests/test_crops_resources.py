"""Static resources of the face-chip kernels, read off the built libyf_images.so (tools/isa_hashes.py): the eight chip kernels (packed pixels of 3
or 4 bytes in the chip's byte order or its reverse; NV12 and NV21 to either order) and the scan exist, none of them uses scratch, and each stays within 64 VGPRs."""
import os
import sys

import pytest

from conftest import ROOT
from images_support import images          # noqa: F401 (fixture)

LLVM = "/opt/rocm/lib/llvm/bin"

pytestmark = pytest.mark.skipif(not all(os.path.exists(os.path.join(LLVM, t)) for t in ("llvm-objcopy", "llvm-objdump", "llvm-readelf", "clang-offload-bundler")),
                                reason="needs the ROCm LLVM tools")


def test_the_chip_kernels_use_no_scratch(images):
    images.load()                                 # builds the library if it is stale
    sys.path.insert(0, ROOT)
    from tools import isa_hashes
    res = {}
    isa_hashes.disassemble(images.lib_path(), res)
    packed = [k for k in res if "yfcrop" in k and "chips_kernel" in k]
    yuv = [k for k in res if "yfcrop" in k and "chips_yuv_kernel" in k]
    scan = [k for k in res if "yfcrop" in k and "first_kernel" in k]
    assert len(packed) == 4 and len(yuv) == 4 and len(scan) == 1, sorted(res)      # <3 | 4 bytes> x <same | reversed order>; <NV12 | NV21> x <RGB | BGR>
    for k in packed + yuv + scan:
        assert res[k]["private_segment_fixed_size"] == 0, (k, res[k])
        assert res[k]["vgpr_count"] <= 64, (k, res[k])            # eight waves per SIMD stay possible (512 VGPRs / 64)
