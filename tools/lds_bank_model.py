#!/usr/bin/env python3
"""The LDS bank rule of profiles/r10_lds_conflicts_by_stage.txt applied to a stage's lane -> address map.  DEV TOOL (no GPU, no build).

The rule: ds_read_b32 / ds_write_b32 serve the two 32-lane halves of a wave one after the other; bank = dword mod 32; lanes on the SAME address are free of
each other; a k-way conflict (k distinct dwords on one bank) costs k - 1 extra cycles for that half.  A half with no active lane costs nothing.  So one
wave-instruction costs  sum over its active halves of k  LDS pipe cycles, of which  sum of (k - 1)  are conflict cycles.

A stage is stated as
    waves   a list of wave-items, each {lane: item} for the active lanes (an item is whatever tuple the address functions take)
    loads   a list of functions item -> byte address, one per ds_read_b32 of the sweep
    stores  the same for the ds_write_b32
and `stage_cycles` returns read / store conflict and pipe cycles.  The maps of pool_8's two passes (yf_kernels.hip.h: pool8_h, pool8_h_rows, pool8_v) are
stated below: the shipped ones, the one pool8_h_rows replaced in the two-frame kernels, and the order "q,k,f" of pool8_v that round 11 evaluated and did
not take (inside the timing scatter, profiles/r11_pool_lanes_ab.txt).  `python tools/lds_bank_model.py` prints them per frame.  The figures are the rule's
output, not measurements: profiles/r11_lds_conflicts_by_stage.txt holds them beside the counters.
"""
import sys

# the LDS plan of the 56x56 kernel (yf_kernels.hip.h): byte offsets inside a frame's arena, two frames of a group FRAME_STRIDE bytes apart
FRAME_STRIDE = 34176
T4_ROWB, T4_S, T4_ORIGIN = 580, 20, 580 + 20      # B_T4: 29 pixels of 20 bytes per row, one halo row and one halo column in front of pixel (0, 0)
HB_OFF, HB_ROWB = 16832, 280                      # B_HB: [28 rows][14] pixels of 20 bytes
T14_OFF, T14_S, T14_ROWB = 24672, 48, 14 * 48     # B_T14 (concat_22): 14 x 14 pixels of 48 bytes
NO, OUT = 5, 14                                   # outputs per sweep, outputs along the pooled axis
CHUNK0 = (0, 5, 9)                                # first output of chunk k: min(k * NO, OUT - NO)


def half_cost(addrs):
    """(pipe cycles, conflict cycles) of one 32-lane half whose active lanes access the byte addresses `addrs` with a b32 instruction."""
    if not addrs:
        return 0, 0
    banks = {}
    for a in addrs:
        assert a % 4 == 0, a
        banks.setdefault((a // 4) % 32, set()).add(a // 4)
    k = max(len(s) for s in banks.values())
    return k, k - 1


def inst_cost(lane_addr):
    """(pipe cycles, conflict cycles) of one wave-instruction; lane_addr = {lane: byte address} of the active lanes."""
    lo, hi = half_cost([a for l, a in lane_addr.items() if l < 32]), half_cost([a for l, a in lane_addr.items() if l >= 32])
    return lo[0] + hi[0], lo[1] + hi[1]


def stage_cycles(waves, loads, stores, frames=1):
    """Conflict and pipe cycles of a stage, divided by `frames`: dict(read_conflict, store_conflict, conflict, read_pipe, store_pipe, pipe, wave_items)."""
    out = dict(read_conflict=0, store_conflict=0, read_pipe=0, store_pipe=0, wave_items=0)
    for items in waves:
        if not items:
            continue
        out["wave_items"] += 1
        for kind, fns in (("read", loads), ("store", stores)):
            for fn in fns:
                pipe, conf = inst_cost({l: fn(*it) for l, it in items.items()})
                out[kind + "_pipe"] += pipe
                out[kind + "_conflict"] += conf
    out["conflict"] = out["read_conflict"] + out["store_conflict"]
    out["pipe"] = out["read_pipe"] + out["store_pipe"]
    return {k: v / frames for k, v in out.items()}


def linear_waves(total, nt, item_of):
    """The wave-items of `for (i = tid; i < total; i += nt)` on nt threads: lane l of wave w takes item_of(w * 64 + l + pass * nt)."""
    out = []
    for base in range(0, total, nt):
        for w in range(nt // 64):
            out.append({l: item_of(base + w * 64 + l) for l in range(64) if base + w * 64 + l < total})
    return out


def sweep_coords(k):
    """The 16 clamped input coordinates that pool8_sweep<5, 27> loads for chunk k, in load order."""
    return [min(max(2 * (CHUNK0[k] - 2 + jj) + h, 0), 27) for jj in range(NO + 3) for h in (1, 2)]


# ---- pool_8 h: T4 -> HB.  item = (cg, k, y, f): channel dword, chunk, row, frame
def pool8_h_accesses():
    loads = [lambda cg, k, y, f, n=n: f * FRAME_STRIDE + T4_ORIGIN + y * T4_ROWB + sweep_coords(k)[n] * T4_S + 4 * cg for n in range(2 * NO + 6)]
    stores = [lambda cg, k, y, f, n=n: f * FRAME_STRIDE + HB_OFF + y * HB_ROWB + (CHUNK0[k] + n) * 20 + 4 * cg for n in range(NO)]
    return loads, stores


def pool8_h_items(nt=192):
    """pool8_h: one item per lane, cg fastest, then k, y, f (the staged-order builds, the one-frame kernels; the two-frame kernels before round 11)."""
    return linear_waves(2 * 28 * 3 * 5, nt, lambda i: (i % 5, (i // 5) % 3, (i // 15) % 28, i // 420))


def pool8_h_rows():
    """pool8_h_rows (round 11): a wave-item is (cg, k); lanes 0-27 take rows 0-27 of frame 0, lanes 32-59 those of frame 1, the other eight are masked."""
    return [{32 * f + y: (cg, k, y, f) for f in range(2) for y in range(28)} for k in range(3) for cg in range(5)]


# ---- pool_8 v: HB -> concat_22.  item = (cg, k, ox, f): channel dword, chunk, column, frame
def pool8_v_accesses():
    loads = [lambda cg, k, ox, f, n=n: f * FRAME_STRIDE + HB_OFF + ox * 20 + 4 * cg + sweep_coords(k)[n] * HB_ROWB for n in range(2 * NO + 6)]
    stores = [lambda cg, k, ox, f, n=n: f * FRAME_STRIDE + T14_OFF + ox * T14_S + 4 * cg + (CHUNK0[k] + n) * T14_ROWB for n in range(NO)]
    return loads, stores


def pool8_v_items(order, nt=192):
    """pool8_v on nt threads.  order "cg,k,ox,f": cg fastest, then the chunk (shipped); "q,k,f": q = 5 ox + cg fastest (round 11's candidate, not taken)."""
    if order == "cg,k,ox,f":
        return linear_waves(420, nt, lambda i: (i % 5, (i // 5) % 3, (i // 15) % 14, i // 210))
    assert order == "q,k,f", order
    return linear_waves(420, nt, lambda i: (i % 70 % 5, (i // 70) % 3, i % 70 // 5, i // 210))


MAPS = {
    "pool8_h items (cg, k, y, f)": lambda: stage_cycles(pool8_h_items(), *pool8_h_accesses(), frames=2),
    "pool8_h rows across the lanes": lambda: stage_cycles(pool8_h_rows(), *pool8_h_accesses(), frames=2),
    "pool8_v items (cg, k, ox, f)": lambda: stage_cycles(pool8_v_items("cg,k,ox,f"), *pool8_v_accesses(), frames=2),
    "pool8_v items (q, k, f)": lambda: stage_cycles(pool8_v_items("q,k,f"), *pool8_v_accesses(), frames=2),
}


def main():
    print("the bank rule on pool_8's lane maps, two-frame kernel, cycles PER FRAME (conflict = read + store; pipe = read + store)")
    print(f"{'map':32s} {'wave-items':>10s} {'read confl':>10s} {'store confl':>11s} {'conflict':>9s} {'read pipe':>10s} {'store pipe':>10s} {'pipe':>7s}")
    for name, fn in MAPS.items():
        if len(sys.argv) > 1 and not any(a in name for a in sys.argv[1:]):
            continue
        r = fn()
        print(f"{name:32s} {r['wave_items']:10.1f} {r['read_conflict']:10.1f} {r['store_conflict']:11.1f} {r['conflict']:9.1f} "
              f"{r['read_pipe']:10.1f} {r['store_pipe']:10.1f} {r['pipe']:7.1f}")


if __name__ == "__main__":
    main()
