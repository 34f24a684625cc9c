"""The float32-requantisation kernel set (YF_ROUND_FP32, namespaces yfx / yf160x) is ADDED beside the existing kernels: every kernel of the library before
it -- the 12 frozen ones and the 7 of the sign-free set (yfu, yf160u) -- disassembles to the same instruction stream (profiles/isa_hashes_before_fp32.txt,
tools/isa_hashes.py), and exactly seven new kernels exist: the four 56x56 shapes and the three 160x160 band kernels of the fp32 set."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

LLVM = "/opt/rocm/lib/llvm/bin"


@pytest.mark.skipif(not all(os.path.exists(os.path.join(LLVM, t)) for t in ("llvm-objcopy", "llvm-objdump", "clang-offload-bundler")),
                    reason="needs the ROCm LLVM tools")
def test_existing_kernels_unchanged_and_seven_fp32_kernels_added(yf):
    yf.load()                                     # builds the library if it is stale
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_hashes.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    now = set(ln.strip() for ln in r.stdout.splitlines() if ln.strip())
    before = [ln.strip() for ln in open(os.path.join(ROOT, "profiles", "isa_hashes_before_fp32.txt")) if ln.strip() and not ln.startswith("#")]
    assert len(before) == 19
    assert [ln for ln in before if ln not in now] == []
    new = sorted(ln.split()[2] for ln in now - set(before))
    assert len(new) == 7 and all(n.startswith(("_ZN3yfx", "_ZN6yf160x")) for n in new), new
    assert sum(n.startswith("_ZN3yfx16yoloface56_fused") for n in new) == 4
    assert sum(n.startswith("_ZN6yf160x4band") for n in new) == 3
