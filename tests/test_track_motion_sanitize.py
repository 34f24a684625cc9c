"""The host build of the tracker with a motion model under ASan + UBSan: tests/csrc/track_motion_sanitize_main.c, a program of its own
compiled together with csrc/yf_images_host.c and run directly -- every state, record row and output array an allocation of exactly its
extent; states of random bytes, counters at the int32 extremes, pos and vel at the int64 extremes (no signed overflow: the clamp of
yfi_motion_sat holds), full tables; records with int32 extremes, empty and inverted boxes; both layouts; refused calls over freed memory.
No GPU, nothing loaded into Python."""
import os
import subprocess

from conftest import ROOT

PKG = os.path.join(ROOT, "stm32h7-yolo_amd")


def test_host_motion_tracker_is_clean_under_asan_and_ubsan(tmp_path):
    cc = os.environ.get("CC", "cc")                                  # the compiler csrc/Makefile's $(CC) resolves to; a machine without one fails here
    exe = str(tmp_path / "track_motion_sanitize")
    subprocess.check_call([cc, "-O1", "-g", "-std=gnu11", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "csrc", "track_motion_sanitize_main.c"),
                           os.path.join(PKG, "csrc", "yf_images_host.c"), "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("motion: ok"), r.stdout + r.stderr
