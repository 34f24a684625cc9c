"""The loader every library of the project goes through (stm32h7-yolo_amd/libs.py), without a GPU: the load policy on libyf_images.so and
libyf_calib.so (tests/test_abi.py::test_load_without_a_build_tool_checks_the_build_id is the same on libyf_network.so), and the host builds."""
import importlib
import os
import subprocess
import sys

import pytest

from conftest import ROOT

# the child of test_abi's policy test, for the module named in argv[1]: (LOADED, make calls, warnings, id as expected) or (REFUSED, make calls, says why)
CHILD = (
    "import importlib, os, sys, warnings, subprocess\n"
    "os.environ['PATH'] = '/nonexistent'\n"
    "m = importlib.import_module('stm32h7-yolo_amd.' + sys.argv[1])\n"
    "mode = sys.argv[2]\n"
    "if 'bad' in mode: m.expected_build_id = lambda: '0' * 16\n"
    "if 'stale' in mode: m.library_is_current = lambda: False\n"
    "calls = []\n"
    "real = subprocess.check_call\n"
    "def spy(*a, **k): calls.append(a); return real(*a, **k)\n"
    "subprocess.check_call = spy\n"
    "with warnings.catch_warnings(record=True) as w:\n"
    "    warnings.simplefilter('always')\n"
    "    try:\n"
    "        lib = m.load()\n"
    "        have = getattr(lib, 'yf_' + sys.argv[1] + '_build_id')().decode()\n"
    "        print('LOADED', len(calls), sum('could not run the build' in str(x.message) for x in w), have == m.expected_build_id())\n"
    "    except RuntimeError as e:\n"
    "        print('REFUSED', len(calls), 'build id' in str(e))\n")


@pytest.mark.parametrize("mode, no_build, want", [
    ("good", False, "LOADED 0 0 True"),             # current library: no make, no child process at all
    ("stale", False, "LOADED 1 1 True"),            # has to build, cannot (no make on PATH): warns, checks the id, loads
    ("stale-bad", False, "REFUSED 1 True"),
    ("stale", True, "LOADED 0 0 True"),             # YF_NO_BUILD=1: never starts make ...
    ("stale-bad", True, "REFUSED 0 True"),          # ... and refuses a library built from other sources
])
@pytest.mark.parametrize("module", ["images", "calib"])
def test_companion_libraries_load_under_the_network_librarys_policy(module, mode, no_build, want):
    """images.load() and calib.load() on the five cases of the network library's policy test, each in a fresh process (a library that is loaded
    would decide the next case).  The network library that images.load() opens first is current in every case, so the counted make is its own."""
    env = dict(os.environ, **({"YF_NO_BUILD": "1"} if no_build else {}))
    env.pop("YF_LIB_PATH", None)
    if not no_build:
        env.pop("YF_NO_BUILD", None)
    r = subprocess.run([sys.executable, "-c", CHILD, module, mode], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.stdout.strip() == want, r.stdout + r.stderr


def test_host_library_makes_its_target_and_starts_nothing_under_no_build(monkeypatch):
    """libs.host_library: `make ../lib/<name>` and dlopen; with YF_NO_BUILD=1 no child process, and a file that is not there raises."""
    libs = importlib.import_module("stm32h7-yolo_amd.libs")
    assert hasattr(libs.host_library("libyf_hostprep.so"), "yf_prepare_tables")
    calls = []
    monkeypatch.setattr(subprocess, "check_call", lambda *a, **k: calls.append(a))
    monkeypatch.setenv("YF_NO_BUILD", "1")
    assert hasattr(libs.host_library("libyf_hostprep.so"), "yf_prepare_tables")
    with pytest.raises(OSError):
        libs.host_library("libyf_no_such_library.so")
    assert not calls
