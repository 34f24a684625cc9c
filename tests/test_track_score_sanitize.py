"""The host build of the score of tracks against labelled identities under ASan + UBSan: tests/csrc/track_score_sanitize_main.c, a
program of its own compiled together with csrc/yf_images_host.c and run directly -- every state, ground-truth row, record row, count,
match and status array an allocation of exactly its extent; states of random bytes and counters at their extremes, ids of random bytes
and at the integer extremes (the state is indexed by ground-truth ids), counts at the integer extremes, dense 64 x 64 tables; both
layouts; refused calls over freed memory.  No GPU, nothing loaded into Python."""
import os
import subprocess

from conftest import ROOT

PKG = os.path.join(ROOT, "stm32h7-yolo_amd")


def test_host_track_score_is_clean_under_asan_and_ubsan(tmp_path):
    cc = os.environ.get("CC", "cc")                                  # the compiler csrc/Makefile's $(CC) resolves to; a machine without one fails here
    exe = str(tmp_path / "track_score_sanitize")
    subprocess.check_call([cc, "-O1", "-g", "-std=gnu11", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "csrc", "track_score_sanitize_main.c"),
                           os.path.join(PKG, "csrc", "yf_images_host.c"), "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("score: ok"), r.stdout + r.stderr
