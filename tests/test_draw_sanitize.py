"""The host build of the drawing under ASan + UBSan: tests/csrc/draw_sanitize_main.c, a program of its own compiled together with
csrc/yf_images_host.c and run directly -- every picture and plane an allocation of exactly its extent and every frame a picture of its own,
the designed boxes (on and beyond every border, wholly outside at distance half and half + 1, inverted, points and lines, int32 extremes),
records, counts, keys and palettes of random bytes, every format, half 0 to 3, with and without keys, and invalid descriptors over freed
memory.  No GPU, nothing loaded into Python."""
import os
import subprocess

from conftest import ROOT

PKG = os.path.join(ROOT, "stm32h7-yolo_amd")


def test_host_drawing_is_clean_under_asan_and_ubsan(tmp_path):
    cc = os.environ.get("CC", "cc")                                  # the compiler csrc/Makefile's $(CC) resolves to; a machine without one fails here
    exe = str(tmp_path / "draw_sanitize")
    subprocess.check_call([cc, "-O1", "-g", "-std=gnu11", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "csrc", "draw_sanitize_main.c"),
                           os.path.join(PKG, "csrc", "yf_images_host.c"), "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("draw: ok"), r.stdout + r.stderr
