"""Static resources of the letterbox kernels, read off the built libyf_images.so (tools/isa_hashes.py): the 21 kernels of namespace yffit
exist -- the prepare for the four packed formats at 56, at 160 and as fp16 frames, for NV12 and NV21 likewise, and the three decodes --,
none of them uses scratch, and no prepare kernel uses more VGPRs or more LDS than the plain prepare kernel for the same format, frame
side and element in the same library, whatever those figures are (of the plain kernel's two instances the ragged one is the like: the
letterbox kernels are ragged only)."""
import os
import re
import sys

import pytest

from conftest import ROOT
from images_support import images          # noqa: F401 (fixture)

LLVM = "/opt/rocm/lib/llvm/bin"

pytestmark = pytest.mark.skipif(not all(os.path.exists(os.path.join(LLVM, t)) for t in ("llvm-objcopy", "llvm-objdump", "llvm-readelf", "clang-offload-bundler")),
                                reason="needs the ROCm LLVM tools")


def plain_name(name):
    """the mangled name of the plain ragged prepare kernel that does a letterbox prepare kernel's work"""
    m = re.match(r"_ZN5yffit13frames_kernelILi(\d+)ELi(\d)ELb(\d)E([at])EEvNS_4ArgsE$", name)
    if m:
        out, c, bgr, elem = m.groups()
        if elem == "t":
            return f"_ZN12_GLOBAL__N_118prepare_f16_kernelILi{c}ELb{bgr}ELb1EEEvNS_8PrepArgsE"
        return f"_ZN12_GLOBAL__N_114prepare_kernelILi{out}ELi{c}ELb{bgr}ELb1EEEvNS_8PrepArgsE"
    m = re.match(r"_ZN5yffit17frames_yuv_kernelILi(\d+)ELb(\d)E([at])EEvNS_4ArgsE$", name)
    if m:
        out, vfirst, elem = m.groups()
        if elem == "t":
            return f"_ZN12_GLOBAL__N_122prepare_yuv_f16_kernelILb{vfirst}ELb1EEEvNS_7YuvArgsE"
        return f"_ZN12_GLOBAL__N_118prepare_yuv_kernelILi{out}ELb{vfirst}ELb1EEEvNS_7YuvArgsE"
    return None


def test_the_fit_kernels_use_no_scratch_and_no_more_than_the_plain_prepare(images):
    images.load()                                 # builds the library if it is stale
    sys.path.insert(0, ROOT)
    from tools import isa_hashes
    res = {}
    isa_hashes.disassemble(images.lib_path(), res)
    ours = [k for k in res if "yffit" in k]
    count = lambda part: len([k for k in ours if part in k])
    assert len(ours) == 21, sorted(res)
    assert (count("frames_kernel"), count("frames_yuv_kernel")) == (12, 6), ours
    assert (count("decode56_kernel"), count("decode160_kernel"), count("decode_f32_kernel")) == (1, 1, 1), ours
    # the resource tests of the other stages count their kernels by these names
    assert not any(name in k for k in ours for name in ("prepare_", "yfcrop", "yfredact", "yfblur", "yfdraw", "yftrack")), ours
    compared = 0
    for k in ours:
        assert res[k]["private_segment_fixed_size"] == 0, (k, res[k])
        assert res[k]["vgpr_spill_count"] == 0 and res[k]["sgpr_spill_count"] == 0, (k, res[k])
        plain = plain_name(k)
        if plain is None:
            continue
        assert plain in res, (k, plain)
        print(f"{k}: {res[k]['vgpr_count']} VGPRs, {res[k]['group_segment_fixed_size']} B of LDS; {plain}: "
              f"{res[plain]['vgpr_count']} VGPRs, {res[plain]['group_segment_fixed_size']} B")
        assert res[k]["vgpr_count"] <= res[plain]["vgpr_count"], (k, res[k], plain, res[plain])
        assert res[k]["group_segment_fixed_size"] <= res[plain]["group_segment_fixed_size"], (k, res[k], plain, res[plain])
        compared += 1
    assert compared == 18
