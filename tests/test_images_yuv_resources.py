"""Static resources of the NV12 / NV21 prepare kernels, read off the built libyf_images.so (tools/isa_hashes.py): the twelve instantiations
exist and none of them uses scratch."""
import os
import sys

import pytest

from conftest import ROOT
from images_support import images          # noqa: F401 (fixture)

LLVM = "/opt/rocm/lib/llvm/bin"

pytestmark = pytest.mark.skipif(not all(os.path.exists(os.path.join(LLVM, t)) for t in ("llvm-objcopy", "llvm-objdump", "llvm-readelf", "clang-offload-bundler")),
                                reason="needs the ROCm LLVM tools")


def test_the_yuv_kernels_use_no_scratch(images):
    images.load()                                 # builds the library if it is stale
    sys.path.insert(0, ROOT)
    from tools import isa_hashes
    res = {}
    isa_hashes.disassemble(images.lib_path(), res)
    int8 = [k for k in res if "prepare_yuv_kernel" in k]
    f16 = [k for k in res if "prepare_yuv_f16_kernel" in k]
    assert len(int8) == 8 and len(f16) == 4, sorted(res)          # <56 | 160> x <NV12 | NV21> x <uniform | ragged>; fp16 at 56 only
    for k in int8 + f16:
        assert res[k]["private_segment_fixed_size"] == 0, (k, res[k])
        assert res[k]["vgpr_count"] <= 64, (k, res[k])            # eight waves per SIMD stay possible (512 VGPRs / 64)
