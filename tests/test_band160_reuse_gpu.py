"""The 160x160 band kernels (csrc/yf_band160.hip.h) when a workgroup takes SEVERAL band jobs -- bit for bit against the oracle, no tolerance.  Each kernel
is a persistent grid of at most two workgroups per CU; a workgroup keeps its LDS buffers from one job to the next, prefetches the next job's input inside
the current one and maps a job number to (frame, band) in one of two orders.  Up to 102 frames no workgroup of band_k1 / band_k23 sees a second job
(512 for band_k4); the launches here are above that, on frames whose heads are pairwise distinct (tests/test_band160_reuse_host.py shows it, and states
the schedule this module counts on: mv.band_walk).  Every launch follows one of the frames' bitwise complements on the same stream, so that a row of
the per-stream HBM arena that a kernel fails to write holds another frame's values."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import model_variants as mv

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1024
PREFIXES = (1024, 1023, 520, 104, 103)      # XCD order, every workgroup reused | plain order | XCD, partial last round (twice) | plain, 3 workgroups reused
SHIPPED_ROUNDINGS = [0, 1, mv.FP32]         # kernel sets yf160, yf160u, yf160x
BAND_DW = {"band_k1": mv.DW_OPS[0], "band_k23": mv.DW_OPS[2], "band_k4": mv.DW_OPS[3]}      # conv2d_3, conv2d_15, conv2d_27: one depthwise conv per band kernel
FOREIGN = [mv.jitter(1)] + [f(op) for op in BAND_DW.values() for f in (mv.amplify, lambda op: mv.uniform(op, 127), lambda op: mv.uniform(op, -128))]
assert list(BAND_DW.values()) == [3, 15, 27]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def device(torch_cuda):
    """The module's premise, asserted on entry: even band_k4 (one job per frame, at most two workgroups per CU) takes two jobs per workgroup at n = 1024."""
    cus = torch_cuda.cuda.get_device_properties(0).multi_processor_count
    assert 2 * cus * mv.BAND_MAX_WGS_PER_CU <= N * 1, f"{cus} CUs: a grid of {mv.BAND_MAX_WGS_PER_CU * cus} workgroups leaves band_k4 without a second job at n = {N}; this module must not pass without reuse"
    return dict(cus=cus)


@pytest.fixture(scope="module")
def frames(torch_cuda, device):
    x = mv.reuse_frames_160(N)
    perms = [np.random.default_rng(1600 + k).permutation(N) for k in range(2)]
    return dict(x=x, d_x=torch_cuda.from_numpy(x).cuda(), perms=perms, refs={}, seconds=[])


def _oracle_pass(frames, orc, variant, key):
    """one oracle pass over the 1024 frames, kept for the module under `key`"""
    if key not in frames["refs"]:
        t0 = time.perf_counter()
        frames["refs"][key] = orc.run(frames["x"], threads=16, variant=variant)
        frames["seconds"].append(time.perf_counter() - t0)
        print(f"oracle pass over {N} frames at 160x160 ({key}): {frames['seconds'][-1]:.2f} s")
    return frames["refs"][key]


def _where(cus, n, frame, y):
    """the seam a differing head row points at: (band of band_k23, workgroup, round) of that frame at the grid of two workgroups per CU; band_k1 cuts a
    frame into the same five bands of 32 input rows and walks them in the same order, so its band, workgroup and round are the same"""
    band = y // 4                                                # head row y <- rows 2y, 2y + 1 of the 40x40 grid, 8 to a band
    grid = max(mv.band_grids(n, 5, cus))
    wg, rnd = mv.band_locate(n, 5, grid, frame, band)
    prev = mv.band_walk(n, 5, grid)[wg][rnd - 1] if rnd else None
    return (f"band_k1 / band_k23 band {band} of frame {frame}: workgroup {wg}, round {rnd} ({'XCD' if mv.band_xcd_order(n, grid) else 'plain'} order, grid {grid}; "
            f"its previous job: {'none' if prev is None else f'frame {prev[0]} band {prev[1]}'}); band_k4: workgroup {frame % min(n, 2 * cus)}, round {frame // min(n, 2 * cus)}")


def _run(torch, network, device, d_x, n, ref, what):
    got = mv.run_160_after_complement(torch, network, d_x, n)
    d = mv.first_difference(got.reshape(n, -1), ref.reshape(n, -1), (20, 20, 18))
    assert d is None, (f"{what}, n = {n}: head differs first at (frame, y, x, channel) = {d[:4]}: got {d[4]}, oracle {d[5]}; "
                       f"{int((got != ref).any(axis=(1, 2, 3)).sum())} frames differ; " + _where(device["cus"], n, d[0], d[1]))


def _assert_kernel_set(network, rounding, what):
    assert ("fp32 requantisation" in network.kernel_name) == (rounding == mv.FP32), what
    assert rounding == mv.FP32 or ("sign-free" in network.kernel_name) == (rounding in (1, 2, 3)), what


@pytest.mark.parametrize("rounding", SHIPPED_ROUNDINGS, ids=[mv.rounding_name(r) for r in SHIPPED_ROUNDINGS])
def test_shipped_weights_with_several_jobs_per_workgroup(network, oracle, device, frames, torch_cuda, rounding):
    """Each kernel set on the shipped weights: prefixes of the frame set at n = 1024 (XCD order, every workgroup of every kernel takes a second job),
    1023 (plain order with a full grid), 520 and 104 (XCD order, partial last round: the guard on the prefetch), 103 (plain order, three workgroups
    reused); and all 1024 frames in two seeded permutations, so that other frames and bands follow each other on a workgroup."""
    torch = torch_cuda
    what = f"shipped weights, rounding {mv.rounding_name(rounding)}"
    try:
        network.configure(-1, -1)
        if _BOUND["name"] is not None:                           # (run behind a foreign-weights id: the shipped blob again)
            _BOUND["name"] = None
            network.set_requant_rounding(0)
            network.init()
        network.set_requant_rounding(rounding)
        assert network.requant_rounding == rounding
        _assert_kernel_set(network, rounding, what)
        ref = _oracle_pass(frames, oracle, mv.ROUNDINGS[rounding][1], ("shipped", rounding))
        assert len({h.tobytes() for h in ref}) == N
        for n in PREFIXES:
            _run(torch, network, device, frames["d_x"], n, ref[:n], what)
        for k, perm in enumerate(frames["perms"]):
            d_p = frames["d_x"][torch.from_numpy(perm).cuda()]
            _run(torch, network, device, d_p, N, ref[perm], what + f", permutation {k}")
            _assert_kernel_set(network, rounding, what)
    finally:
        network.set_requant_rounding(0)
        network.configure(-1, -1)


# ---- foreign weights (bound as tests/test_model_variants_gpu.py binds them) -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """variant -> (blob, oracle of the .yfm that states the same weights), each built once"""
    from oracle.oracle import Oracle
    d, cache = tmp_path_factory.mktemp("reuse160"), {}

    def get(v):
        if v.name not in cache:
            blob, path = v.build(d)
            cache[v.name] = (np.frombuffer(blob, np.uint8).copy(), Oracle(path))
        return cache[v.name]
    return get


_BOUND = dict(name=None)                                        # the variant the session's network is bound to


@pytest.fixture(scope="module")
def bound(network, built):
    """bind(v, rounding): the session's network initialised from the variant's blob (one ai_network_init per variant: its ids are consecutive), the
    rounding switched on the ready network.  _BOUND is set only after the init succeeded; the module leaves the session's network on the shipped blob,
    the reference rounding and the automatic shape."""
    def bind(v, rounding):
        network.configure(-1, -1)
        if _BOUND["name"] != v.name:
            _BOUND["name"] = None
            network.set_requant_rounding(0)
            network.init(weights=built(v)[0])
            _BOUND["name"] = v.name
        network.set_requant_rounding(rounding)
        assert network.requant_rounding == rounding
        return built(v)[1]
    try:
        yield bind
    finally:
        _BOUND["name"] = None
        network.set_requant_rounding(0)
        network.init()
        network.configure(-1, -1)


# (variant, rounding): the reference rounding and, where the host admits the variant under it, the fp32 requantisation; a variant's ids are consecutive
FOREIGN_CASES = [(v, r) for v in FOREIGN for r in (0, mv.FP32) if v.admitted(r)]


@pytest.mark.parametrize("v,rounding", FOREIGN_CASES, ids=[f"{v.name}-{mv.rounding_name(r)}" for v, r in FOREIGN_CASES])
def test_foreign_weights_with_several_jobs_per_workgroup(network, bound, device, frames, torch_cuda, v, rounding):
    """Other weights than the shipped ones behind the same schedule: every weight and bias moved (jitter), and one depthwise conv per band kernel
    amplified to both clamps or made uniform +127 / -128 (sum(w) at its extremes against the halo fill: the rows that the first and last band of a frame
    fill, and the others leave to the neighbour rows).  n = 1024 (XCD order) and 1023 (plain order) against the oracle of the variant's .yfm."""
    what = f"{v.name}, rounding {mv.rounding_name(rounding)}"
    orc = bound(v, rounding)
    _assert_kernel_set(network, rounding, what)
    ref = _oracle_pass(frames, orc, mv.ROUNDINGS[rounding][1], (v.name, rounding))
    del frames["refs"][(v.name, rounding)]                       # one pass per id: no other id asks for it
    assert len({h.tobytes() for h in ref}) == N, f"{what}: the oracle's heads are not pairwise distinct"
    for n in (1024, 1023):
        _run(torch_cuda, network, device, frames["d_x"], n, ref[:n], what)


# ---- arena chunks -----------------------------------------------------------------------------------------------------------------------
def test_arena_chunks_in_a_fresh_process(torch_cuda, device):
    """YF_160_CHUNK is read when the engine is created, so tests/dev/chunks_160.py runs as a child: 41 frames in chunks of 16 (XCD order twice, then 9
    frames in the plain order; frame and head pointers advance by chunks, every chunk on the same arena), 8 frames in one chunk of 8, and 232 frames in
    chunks of 112 (a chunk whose workgroups take second jobs, then one of 8 frames without), each under the reference rounding and the fp32
    requantisation, against the oracle.  A wrong `done * IN_FRAME_BYTES` / `done * OUT_FRAME_BYTES` offset puts distinct heads into the wrong slots."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "dev", "chunks_160.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("chunks ")]
    assert len(lines) == 6 and all(ln.endswith(" ok") for ln in lines), r.stdout
    for chunk, n, sizes in ((16, 41, "16+16+9"), (8, 8, "8"), (112, 232, "112+112+8")):
        assert sum(f"YF_160_CHUNK={chunk} n={n} ({sizes})" in ln for ln in lines) == 2, r.stdout
