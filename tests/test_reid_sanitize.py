"""The host build of the appearance descriptors and of the re-identification under ASan + UBSan: tests/csrc/reid_sanitize_main.c, a
program of its own compiled together with csrc/yf_images_host.c and run directly -- the pixel buffer (its last picture ends with its
last byte), every descriptor, record, count, state, info, kind and status array an allocation of exactly its extent; records and picture
descriptors of random bytes and at the integer extremes, states of random bytes with duplicated aliases and a clock at UINT32_MAX, counts
at the integer extremes, the full frame against the full table; both layouts; d_info_out the input itself; refused calls over freed
memory.  No GPU, nothing loaded into Python."""
import os
import subprocess

from conftest import ROOT

PKG = os.path.join(ROOT, "stm32h7-yolo_amd")


def test_host_describe_and_reid_are_clean_under_asan_and_ubsan(tmp_path):
    cc = os.environ.get("CC", "cc")                                  # the compiler csrc/Makefile's $(CC) resolves to; a machine without one fails here
    exe = str(tmp_path / "reid_sanitize")
    subprocess.check_call([cc, "-O1", "-g", "-std=gnu11", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "csrc", "reid_sanitize_main.c"),
                           os.path.join(PKG, "csrc", "yf_images_host.c"), "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("reid: ok"), r.stdout + r.stderr
