"""How a library of this project is located, judged current, built and opened: the one parser of csrc/Makefile and csrc/flags.mk, the ids and
the mtime test computed from them, the one `make` (under the checkout's build lock), the load policy of the three GPU libraries (binding, images,
calib) and the loader of the host builds beside them (libyf_hostprep.so, libyf_images_host.so, libyf_calib_host.so)."""
import ctypes
import hashlib
import os
import re
import subprocess

_PKG = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_PKG, "csrc")
LIB_DIR = os.path.join(_PKG, "lib")
ALL = ("all", "../lib/libyf_hostprep.so")       # what binding.build makes: every GPU library and the host-logic library of the CPU tests


def make_var(name):
    """The value of `NAME = ...` in csrc/flags.mk or csrc/Makefile."""
    for mk in ("flags.mk", "Makefile"):
        m = re.search(r"^%s\s*=\s*(.*)$" % name, open(os.path.join(CSRC, mk)).read(), re.M)
        if m:
            return m.group(1).strip()
    raise KeyError(f"{name}: not set in csrc/flags.mk or csrc/Makefile")


def source_id(files, tail):
    """sha256 over the contents of `files` (relative to csrc/, in order) and then `tail`, 16 hex digits: the form of every id the Makefile bakes in."""
    h = hashlib.sha256()
    for f in files:
        h.update(open(os.path.join(CSRC, f), "rb").read())
    h.update(tail.encode())
    return h.hexdigest()[:16]


def newer_than(lib_path, deps):
    """True when `lib_path` exists and is at least as new as every file of `deps` (relative to csrc/, or absolute); False on a missing file."""
    try:
        built = os.path.getmtime(lib_path)
        return all(os.path.getmtime(os.path.join(CSRC, f)) <= built for f in deps)
    except OSError:
        return False


def make(*targets, force=False):
    """`make -C csrc <targets>` for gfx950 (hipcc cross-compiles without a GPU), after `make clean` when forced.  One build at a time: the processes
    that share a checkout (the two ranks of bench.py's self-launch, parallel test workers, profiler-wrapped tools) serialise on a lock file beside
    the Makefile -- not in the output directory, which `make clean` empties while a forced build holds the lock."""
    import fcntl
    os.makedirs(LIB_DIR, exist_ok=True)
    with open(os.path.join(CSRC, ".build.lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        if force:
            subprocess.check_call(["make", "-C", CSRC, "clean"], stdout=subprocess.DEVNULL)
        subprocess.check_call(["make", "-C", CSRC, "-j4", *targets], stdout=subprocess.DEVNULL)


def open_library(path, is_current, ids, unchecked_override=False, preload=None):
    """dlopen a GPU library under the project's load policy.  A YF_LIB_PATH override (A/B of differently compiled libraries) is opened as it is
    where `unchecked_override` says so.  Otherwise, with YF_NO_BUILD=1 (the profiler scripts) or when `is_current()` says the file is newer than
    its sources, it is opened without any child process -- under rocprofv3 every child of a GPU-holding process is instrumented by the profiler's
    preloaded tool; else `make` runs first, so that a stale .so is never loaded under fresh sources, and where the build cannot run (no make, no
    hipcc, or it failed) an existing file is used with a warning.  A file that was not just built must carry the ids the sources give: `ids` is
    a list of (symbol of a function returning the id baked into the library, callable giving the expected id); another build is refused.
    `preload`, if given, is called before the dlopen (binding._one_hip_runtime)."""
    check = True
    if unchecked_override and os.environ.get("YF_LIB_PATH"):
        check = False
    elif os.environ.get("YF_NO_BUILD") == "1" or is_current():
        if not os.path.exists(path):
            raise RuntimeError(f"{path} does not exist and is not being built here (YF_NO_BUILD=1): build it first "
                               "(python -c 'import __graft_entry__ as g; g.build()')")
    else:
        try:
            make(*ALL)
            check = False
        except (OSError, subprocess.CalledProcessError) as e:
            if not os.path.exists(path):
                raise
            import warnings
            warnings.warn(f"stm32h7-yolo_amd: could not run the build ({e}); loading the existing {os.path.basename(path)} after checking its build id")
    if preload is not None:
        preload()
    lib = ctypes.CDLL(path)
    for symbol, expected in ids if check else []:
        fn = getattr(lib, symbol)
        fn.restype, fn.argtypes = ctypes.c_char_p, []
        have, want = (fn() or b"").decode(), expected()
        if have != want:
            raise RuntimeError(f"{path} was built from other sources or flags ({symbol}: build id {have}, expected {want}) and is not being rebuilt "
                               "here (no make / YF_NO_BUILD=1)")
    return lib


def host_library(file_name):
    """A host build (no HIP, no GPU) from lib/, without prototypes: `make ../lib/<file_name>` first, which decides whether the file is current;
    with YF_NO_BUILD=1 no child process is started and the file that is there is opened (OSError when there is none)."""
    if os.environ.get("YF_NO_BUILD") != "1":
        make("../lib/" + file_name)
    return ctypes.CDLL(os.path.join(LIB_DIR, file_name))
