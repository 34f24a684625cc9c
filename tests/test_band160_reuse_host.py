"""What tests/test_band160_reuse_gpu.py relies on, checked without a GPU: the frame set reuse_frames_160() is deterministic and its 1024 heads are pairwise
distinct under the three roundings the kernel sets compute (a frame in the wrong slot or a band from the wrong frame cannot hide), and the plain-Python
restatement of the band kernels' schedule (tests/model_variants.py: band_split_job, band_walk) says which workgroups take a second job, in which order
and with which band behind which, at every frame count that module launches."""
import numpy as np
import pytest

import model_variants as mv

CUS = 256                                                       # the MI355X; the GPU module asserts that its device has no more
N_PREFIXES = (1024, 1023, 520, 104, 103)                        # the launches of the GPU module ...
N_CHUNKS = (16, 9, 8, 112)                                      # ... and the chunks of its arena-chunk cases (16 + 16 + 9, 8, 112 + 112 + 8)
ORACLE_VARIANTS = {"R": 0, "U": 1, "X": 3}                      # reference rounding, ties up on the dense convs, fp32 requantisation


@pytest.fixture(scope="module")
def frames():
    return mv.reuse_frames_160()


def test_the_frame_set_is_deterministic(frames):
    assert frames.shape == (1024, 160, 160, 3) and frames.dtype == np.int8
    assert frames.tobytes() == mv.reuse_frames_160().tobytes()
    assert frames[:41].tobytes() == mv.reuse_frames_160(41).tobytes(), "a shorter set is a prefix: all draws in frame order"
    edges = mv.band_edge_frames_160()
    for k in range(0, 1024, 4):
        assert int((frames[k] != edges[(k // 4) % 39]).any(axis=2).sum()) in range(1, 65), f"frame {k}: one 8x8 patch on its band-edge frame"
    for k in range(1, 1024, 4):
        rows = np.flatnonzero((frames[k] != frames[k, :, :1, :1]).any(axis=(1, 2)))                     # the rows that are not one value throughout
        assert rows.shape[0] == 32 and rows[0] % 32 == 0 and rows[-1] == rows[0] + 31, f"frame {k}: noise inside one 32-row band"
        assert np.unique(np.delete(frames[k], rows, axis=0)).shape[0] == 1, f"frame {k}: one level outside the band"
    assert all(np.abs(frames[k].astype(int)).max() <= 8 for k in range(3, 1024, 4))


@pytest.mark.parametrize("name", list(ORACLE_VARIANTS))
def test_all_heads_are_distinct(oracle, frames, name):
    """A condition on the seed, not a measurement: every one of the 1024 heads differs from every other, and each kind-0 head from the head of the
    unpatched band-edge frame it was made from (whose 39 heads are distinct as well)."""
    variant = ORACLE_VARIANTS[name]
    heads = oracle.run(frames, threads=16, variant=variant)
    assert heads.shape == (1024, 20, 20, 18)
    distinct = len({h.tobytes() for h in heads})
    print(f"oracle variant {name}: {distinct} distinct heads of {heads.shape[0]}")
    assert distinct == 1024
    base = oracle.run(mv.band_edge_frames_160(), threads=16, variant=variant)
    assert len({h.tobytes() for h in base}) == 39
    same = [k for k in range(0, 1024, 4) if np.array_equal(heads[k], base[(k // 4) % 39])]
    assert not same, f"kind-0 frames {same}: the patch does not reach the head"


# ---- the schedule -----------------------------------------------------------------------------------------------------------------------
def _walks(n, grid_of=max):
    """kernel name -> (grid, xcd, walk) at the largest (default) or smallest grid the engine can choose"""
    out = {}
    for name, bands in zip(mv.BAND_KERNELS, mv.BAND_JOBS_PER_FRAME):
        grid = grid_of(mv.band_grids(n, bands, CUS))
        out[name] = (grid, mv.band_xcd_order(n, grid), mv.band_walk(n, bands, grid))
    return out


def _last_round_partial(walk):
    return len(walk[0]) > 1 and len(walk[-1]) == len(walk[0]) - 1


def test_grids_the_engine_can_choose():
    assert mv.band_grids(1024, 5, CUS) == [256, 512] and mv.band_grids(1024, 1, CUS) == [256, 512]
    assert mv.band_grids(104, 1, CUS) == [104] and mv.band_grids(103, 5, CUS) == [256, 512] and mv.band_grids(8, 5, CUS) == [40]
    assert all(g <= 2 * CUS for n in N_PREFIXES + N_CHUNKS for b in mv.BAND_JOBS_PER_FRAME for g in mv.band_grids(n, b, CUS))


@pytest.mark.parametrize("grid_of", [max, min], ids=["two_per_cu", "one_per_cu"])
def test_which_workgroups_take_a_second_job(grid_of):
    """What the GPU module relies on at each n, for either number of resident workgroups per CU."""
    two = grid_of is max
    w = _walks(1024, grid_of)
    for name, (grid, xcd, walk) in w.items():
        assert xcd and grid == (512 if two else 256) and min(len(jobs) for jobs in walk) >= 2, name           # n = 1024: XCD order, every workgroup of every kernel reused
    w = _walks(1023, grid_of)
    assert not any(xcd for _, xcd, _ in w.values())                                                              # n = 1023: plain order
    assert sum(len(jobs) >= 2 for jobs in w["band_k4"][2]) == (511 if two else 256) and all(len(jobs) >= 2 for k in ("band_k1", "band_k23") for jobs in w[k][2])
    for n in (520, 104):                                                                                         # XCD order, partial last round
        w = _walks(n, grid_of)
        assert all(xcd for _, xcd, _ in w.values()), n
        assert _last_round_partial(w["band_k1"][2]) and _last_round_partial(w["band_k23"][2]), n
    assert _last_round_partial(_walks(520, grid_of)["band_k4"][2])
    grid, xcd, walk = _walks(104, grid_of)["band_k4"]                                                            # (band_k4 at n = 104: one job on each of 104 workgroups)
    assert grid == 104 and xcd and all(len(jobs) == 1 for jobs in walk)
    w = _walks(103, grid_of)                                                                                     # n = 103: plain order, 515 jobs = grid + 3 (or 2 grids + 3)
    for k in ("band_k1", "band_k23"):
        grid, xcd, walk = w[k]
        assert not xcd and [len(jobs) for jobs in walk] == [len(walk[-1]) + 1] * 3 + [len(walk[-1])] * (grid - 3) and len(walk[-1]) == (1 if two else 2)
    assert w["band_k4"][0] == 103 and not w["band_k4"][1]
    for n, reused in ((16, False), (9, False), (8, False), (112, True)):                                         # the arena chunks: 112 frames reuse, the others do not
        w = _walks(n, grid_of)
        assert all(xcd == (n % 8 == 0) for _, xcd, _ in w.values()), n
        assert all((max(len(jobs) for jobs in w[k][2]) > 1) == reused for k in ("band_k1", "band_k23")), n
        assert all(len(jobs) == 1 for jobs in w["band_k4"][2]), n


@pytest.mark.parametrize("n", [1024, 1023], ids=["xcd_order", "plain_order"])
def test_band_transitions_on_a_workgroup(n):
    """At grid 512: the plain order puts band b + 2 (mod 5) behind band b, the XCD order band b - 1 (mod 5): job v + 512 is 512 = 5 * 102 + 2 jobs on in
    the plain order, and (v + 512) >> 3 = (v >> 3) + 64 = 5 * 13 - 1 band slots on in the XCD order.  Either way all five (previous -> next) pairs occur, a
    top band (a == 0) and a bottom band each come as a later job of some workgroup, and a later job is always another frame's."""
    for bands in (5, 5):
        walk = mv.band_walk(n, bands, 512)
        xcd = mv.band_xcd_order(n, 512)
        assert xcd == (n == 1024)
        pairs = {(a[1], b[1]) for jobs in walk for a, b in zip(jobs, jobs[1:])}
        assert pairs == {(b, (b - 1) % 5 if xcd else (b + 2) % 5) for b in range(5)}
        later = {b for jobs in walk for _, b in jobs[1:]}
        assert 0 in later and bands - 1 in later
        assert all(a[0] != b[0] for jobs in walk for a, b in zip(jobs, jobs[1:]))
    # grid 256 (one resident workgroup per CU): 256 = 5 * 51 + 1 jobs on, 32 = 5 * 6 + 2 band slots on
    walk = mv.band_walk(n, 5, 256)
    assert {(a[1], b[1]) for jobs in walk for a, b in zip(jobs, jobs[1:])} == {(b, (b + 2) % 5 if n == 1024 else (b + 1) % 5) for b in range(5)}


@pytest.mark.parametrize("n", N_PREFIXES + N_CHUNKS)
def test_every_job_is_one_frame_and_band(n):
    """Every job number maps to exactly one (frame, band) and every (frame, band) is hit once: in the order the kernel takes at each grid the engine can
    choose, in the plain order at every n, and in the XCD order wherever its condition (n and grid multiples of 8) can hold; band_locate inverts it."""
    for bands in mv.BAND_JOBS_PER_FRAME:
        want = sorted((f, b) for f in range(n) for b in range(bands))
        for grid in mv.band_grids(n, bands, CUS):
            orders = {mv.band_xcd_order(n, grid), False} | ({True} if n % 8 == 0 and grid % 8 == 0 else set())
            for xcd in orders:
                walk = mv.band_walk(n, bands, grid, xcd)
                assert len(walk) == grid and sorted(j for jobs in walk for j in jobs) == want, (n, bands, grid, xcd)
            walk = mv.band_walk(n, bands, grid)
            for f, b in ((0, 0), (n - 1, bands - 1), (n // 2, bands // 2), (min(7, n - 1), 0), (min(8, n - 1), bands - 1)):
                wg, rnd = mv.band_locate(n, bands, grid, f, b)
                assert walk[wg][rnd] == (f, b)
    if n % 8:
        assert sorted(mv.band_split_job(v, True, 5) for v in range(5 * n)) != sorted((f, b) for f in range(n) for b in range(5)), "the XCD order needs n % 8 == 0"
