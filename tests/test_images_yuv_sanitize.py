"""The host prepare of NV12 / NV21 surfaces under ASan + UBSan: tests/csrc/yuv_sanitize_main.c, a program of its own compiled together with
csrc/yf_images_host.c and run directly -- each plane an allocation of exactly its extent, every shape of the GPU tests, both chroma orders,
int8 and fp16 frames, and the descriptor check on sums that overflow.  No GPU, nothing loaded into Python."""
import os
import subprocess

from conftest import ROOT

PKG = os.path.join(ROOT, "stm32h7-yolo_amd")


def test_host_prepare_of_surfaces_is_clean_under_asan_and_ubsan(tmp_path):
    cc = os.environ.get("CC", "cc")                                  # the compiler csrc/Makefile's $(CC) resolves to; a machine without one fails here
    exe = str(tmp_path / "yuv_sanitize")
    subprocess.check_call([cc, "-O1", "-g", "-std=gnu11", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "csrc", "yuv_sanitize_main.c"),
                           os.path.join(PKG, "csrc", "yf_images_host.c"), "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("yuv: ok"), r.stdout + r.stderr
