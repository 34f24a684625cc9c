"""tools/lds_bank_model.py: the LDS bank rule (ds_read_b32 / ds_write_b32 serve the two 32-lane halves one after the other, bank = dword mod 32, lanes on the
same address are free of each other, a k-way conflict costs k - 1 extra cycles per half) applied to the lane -> address maps of pool_8's two passes.

The figures below are the RULE'S OUTPUT on the stated maps, not measurements: 432.0 and 194.0 are what it gives for the maps that shipped before round 11 (the
first is also what the counters measured for that pass, profiles/r10_lds_conflicts_by_stage.txt), the others what the tool printed when the new maps were
designed: rows across the lanes for pool8_h (shipped in the two-frame kernels) and columns fastest for pool8_v (evaluated, not taken: pool8_v keeps its
order).  No GPU, no build."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)
from tools import lds_bank_model as lbm        # noqa: E402


def test_the_rule_on_single_instructions():
    assert lbm.inst_cost({l: 4 * l for l in range(64)}) == (2, 0)                      # consecutive dwords: one cycle per half
    assert lbm.inst_cost({l: 128 * l for l in range(32)}) == (32, 31)                  # 32 lanes on bank 0, upper half idle
    assert lbm.inst_cost({l: 64 for l in range(64)}) == (2, 0)                         # one address: a broadcast
    assert lbm.inst_cost({l: 8 * l for l in range(64)}) == (4, 2)                      # even banks only: 2-way in both halves
    assert lbm.inst_cost({}) == (0, 0)
    assert lbm.inst_cost({0: 0, 1: 128, 40: 4}) == (3, 1)                              # halves are served apart


def test_sweep_coordinates_are_the_kernels():
    """pool8_sweep<5, 27>: odd pairs o0 - 2 .. o0 + 5, coordinates 2j + 1 and 2j + 2 clamped into the row."""
    assert lbm.sweep_coords(0) == [0, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12]
    assert lbm.sweep_coords(1) == list(range(7, 23))
    assert lbm.sweep_coords(2) == list(range(15, 28)) + [27, 27, 27]


@pytest.mark.parametrize("nt", (192, 512))
def test_the_item_order_maps(nt):
    """cg fastest, then the chunk (both passes before round 11; pool8_v and the one-frame / staged-order pool8_h still): on the three pool waves of the
    production kernel and on the eight waves of the staged-order build alike."""
    h = lbm.stage_cycles(lbm.pool8_h_items(nt), *lbm.pool8_h_accesses(), frames=2)
    assert (h["read_conflict"], h["store_conflict"], h["conflict"]) == (367.0, 65.0, 432.0)
    v = lbm.stage_cycles(lbm.pool8_v_items("cg,k,ox,f", nt), *lbm.pool8_v_accesses(), frames=2)
    assert (v["read_conflict"], v["store_conflict"], v["conflict"]) == (126.5, 67.5, 194.0)


def test_pool8_h_rows_across_the_lanes():
    waves = lbm.pool8_h_rows()
    assert len(waves) == 15 and all(sorted(w) == list(range(28)) + list(range(32, 60)) for w in waves)
    items = sorted(it for w in waves for it in w.values())
    assert items == sorted((cg, k, y, f) for cg in range(5) for k in range(3) for y in range(28) for f in range(2))    # the items of pool8_h, each once
    h = lbm.stage_cycles(waves, *lbm.pool8_h_accesses(), frames=2)
    assert (h["read_conflict"], h["store_conflict"]) == (0.0, 75.0)
    assert (h["read_pipe"], h["store_pipe"], h["pipe"]) == (240.0, 150.0, 390.0)
    old = lbm.stage_cycles(lbm.pool8_h_items(), *lbm.pool8_h_accesses(), frames=2)
    assert old["pipe"] == 715.5


@pytest.mark.parametrize("nt", (192, 512))
def test_pool8_v_columns_fastest(nt):
    """The candidate order of round 11 (q = 5 ox + cg fastest, then k, f): the same items, fewer conflicts by the rule; it did not show in the timing."""
    old, new = lbm.pool8_v_items("cg,k,ox,f", nt), lbm.pool8_v_items("q,k,f", nt)
    assert sorted(it for w in old for it in w.values()) == sorted(it for w in new for it in w.values())               # only an order
    v = lbm.stage_cycles(new, *lbm.pool8_v_accesses(), frames=2)
    assert (v["read_conflict"], v["store_conflict"], v["conflict"]) == (39.0, 37.5, 76.5)
    assert (v["read_pipe"], v["store_pipe"]) == (151.0, 72.5)


def test_addresses_stay_inside_their_buffers():
    """Every address the maps state lies in T4 (reads of h), HB (stores of h, reads of v) or concat_22's pool half (stores of v)."""
    hl, hs = lbm.pool8_h_accesses()
    vl, vs = lbm.pool8_v_accesses()
    for waves, loads, stores, rd, wr in ((lbm.pool8_h_rows(), hl, hs, (0, 29 * 580), (16832, 16832 + 7840)),
                                         (lbm.pool8_v_items("q,k,f"), vl, vs, (16832, 16832 + 7840), (24672, 24672 + 196 * 48))):
        for w in waves:
            for cg, k, a, f in w.values():
                for fn, (lo, hi) in [(fn, rd) for fn in loads] + [(fn, wr) for fn in stores]:
                    assert lo <= fn(cg, k, a, f) - f * lbm.FRAME_STRIDE < hi


def test_command_line_prints_the_four_maps():
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "lds_bank_model.py")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    rows = {ln[:32].strip(): ln[32:].split() for ln in r.stdout.splitlines()[2:]}
    assert rows["pool8_h items (cg, k, y, f)"][3] == "432.0" and rows["pool8_h rows across the lanes"][3] == "75.0"
    assert rows["pool8_v items (cg, k, ox, f)"][3] == "194.0" and rows["pool8_v items (q, k, f)"][3] == "76.5"
