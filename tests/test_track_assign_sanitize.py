"""The host build of the optimal assignment under ASan + UBSan: tests/csrc/track_assign_sanitize_main.c, a program of its own compiled
together with csrc/yf_images_host.c and run directly -- every state, record row, table of weights and output array an allocation of
exactly its extent; tables of weights all at the maximum, all at the minimum, staircases and random ones (no signed overflow: the bound of
csrc/yf_images_assign.h on the potentials holds); through the entry the 64 x 64 scenes of all-maximum and all-minimum weight, states of
random bytes, counters at the int32 extremes, pos and vel at the int64 extremes, full tables, records with int32 extremes; both layouts,
both values of assign; refused calls over freed memory.  No GPU, nothing loaded into Python."""
import os
import subprocess

from conftest import ROOT

PKG = os.path.join(ROOT, "stm32h7-yolo_amd")


def test_host_optimal_assignment_is_clean_under_asan_and_ubsan(tmp_path):
    cc = os.environ.get("CC", "cc")                                  # the compiler csrc/Makefile's $(CC) resolves to; a machine without one fails here
    exe = str(tmp_path / "track_assign_sanitize")
    subprocess.check_call([cc, "-O1", "-g", "-std=gnu11", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "csrc", "track_assign_sanitize_main.c"),
                           os.path.join(PKG, "csrc", "yf_images_host.c"), "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("assign: ok"), r.stdout + r.stderr
