"""The host build's channel sums under ASan + UBSan: tests/csrc/calib_chan_sanitize_main.c, a program of its own compiled together with
csrc/yf_calib_host.c and the .yfw parser and run directly.  No GPU, nothing loaded into Python."""
import os
import subprocess

from conftest import ROOT
import calib_support as cs

PKG = os.path.join(ROOT, "stm32h7-yolo_amd")


def test_host_channel_sums_are_clean_under_asan_and_ubsan(tmp_path):
    cc = os.environ.get("CC", "cc")                                  # the compiler csrc/Makefile's $(CC) resolves to; a machine without one fails here
    exe, model = str(tmp_path / "calib_chan_sanitize"), str(tmp_path / "model.yfw")
    open(model, "wb").write(cs.yfw_bytes("yfw"))
    subprocess.check_call([cc, "-O1", "-g", "-std=gnu11", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "csrc", "calib_chan_sanitize_main.c"),
                           os.path.join(PKG, "csrc", "yf_calib_host.c"), os.path.join(PKG, "csrc", "yf_yfw.c"), "-lpthread"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, model], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("channel sums: ok"), r.stdout + r.stderr
