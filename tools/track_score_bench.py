#!/usr/bin/env python3
"""The score of tracks against labelled identities on the GPU (GPU TOOL; bench.py is not involved), in two parts, both reported and
neither gated: there is no earlier number for this operation.

TIME.  What one launch of yf_images_score_tracks_device costs beside one launch of yf_images_track_motion_assign_device with
YF_ASSIGN_OPTIMAL on the same records -- the yardstick, since it runs the same search.  The two calls are interleaved in one loop, round
after round the score, then the tracker, device events around every call, warm-up first, the median of the timed calls.

    real      4096 pictures of 410x362 with real content (the 27 real frames of tests/golden upscaled to that size, repeated): the ragged
              run at 56x56 and the suppression at 0.4 leave the records, the tracker (optimal, the suggested gains) the reported tracks,
              and the ground truth of the score is those tracks themselves under ids 1, 2, ... in their order.  4096 streams x 1 step and
              the same frames as 64 streams x 64 steps, the states carried from call to call.
    dense     64 tracks at one box against 64 labelled objects (detections) at one box beside it: every pair eligible with the same
              weight, 2080 rounds of the search per step.  64 streams x 64 steps.  The score's state is emptied and the tracker's
              tables are refilled before every timed call, outside the events, so that every step of both searches the whole table.

Then the kernel's registers, LDS and scratch (tools/isa_hashes.py), and with --parent-lib the libyf_images.so of the parent commit, built
from its sources with the same compiler: every kernel of it must be present with an identical instruction hash.

FIGURES.  The first identity-switch figures, on SYNTHETIC CLIPS, NOT VIDEO: `Tracker` in its four settings -- greedy or optimal, each
with motion=None or the suggested gains -- scored by `TrackScore` on the pan and the crossing streams of
tests/assign_support.crossing_frames and on seeded random clips of drifting faces with detector drop-outs.

    python tools/track_score_bench.py [--iters 30] [--warmup 5] [--parent-lib PATH] [--out profiles/track_score_bench.txt]
"""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 410, 362
SCORE_IOU, TRACKER = 0.5, (0.3, 1, 5)
RANDOM_CLIPS, RANDOM_STEPS, RANDOM_SEED = 8, 40, 9100


def random_clip(rng):
    """one clip: four to seven faces of side 40 .. 90 that drift by up to 12 pixels a step with a little jitter, about 15 % of the
    detections missing, the frame's order shuffled -> (frames[t] = boxes of the detections, truth[t] = [(id, x1, y1, x2, y2)])"""
    faces = [[int(rng.integers(0, 500)), int(rng.integers(0, 300)), int(rng.integers(40, 91)), int(rng.integers(-12, 13)), int(rng.integers(-6, 7))]
             for _ in range(int(rng.integers(4, 8)))]
    frames, truth = [], []
    for _ in range(RANDOM_STEPS):
        for f in faces:
            f[0] += f[3] + int(rng.integers(-2, 3))
            f[1] += f[4] + int(rng.integers(-2, 3))
        boxes = [(f[0], f[1], f[0] + f[2] - 1, f[1] + f[2] - 1) for f in faces]
        truth.append([(k + 1, *b) for k, b in enumerate(boxes)])
        seen = [b for b in boxes if rng.random() > 0.15]
        frames.append([seen[int(k)] for k in rng.permutation(len(seen))])
    return frames, truth


def clips():
    """-> [(name, frames[s][t] = boxes, truth[s][t])]: the crossing, the pan, the random clips as streams of one call"""
    import assign_support as asg
    import score_support as sc
    cross, pan = ([[boxes for boxes, _ in clip]] for clip in asg.crossing_frames())
    truth = sc.clip_truth()
    rng = np.random.default_rng(RANDOM_SEED)
    made = [random_clip(rng) for _ in range(RANDOM_CLIPS)]
    return [("crossing (two faces pass each other, 12 steps)", cross, [truth[0]]), ("pan (two neighbours move by 33 a step, 12 steps)", pan, [truth[1]]),
            (f"random ({RANDOM_CLIPS} clips of 4 to 7 drifting faces, {RANDOM_STEPS} steps, 15 % drop-outs)", [m[0] for m in made], [m[1] for m in made])]


def figures(images, torch, say):
    import track_support as ts
    say("")
    say("# FIGURES: synthetic clips, not video.  No labelled video is at hand; nothing below says how a setting does on real footage.")
    say(f"# score IoU {SCORE_IOU}; tracker (match_iou, min_hits, max_misses) = {TRACKER}; suggested gains (alpha, beta, damp) = {images.MOTION_GAINS}, smooth 0")
    say(f"# {'clip':74s} {'assign':8s} {'motion':10s} {'gt':>5s} {'switches':>8s} {'misses':>7s} {'false+':>7s} {'MOTA':>8s} {'MOTP':>7s}")
    crossing_without_motion = {}
    for name, frames, truth in clips():
        streams, steps = len(frames), len(frames[0])
        cap = max(len(b) for clip in frames for b in clip)
        dets, counts = ts.lay_out([[(b, None) for b in clip] for clip in frames], cap, ts.TIME)
        gt, gt_counts = images.pack_track_truth([truth[s][t] for t in range(steps) for s in range(streams)])
        d_dets = torch.from_numpy(dets.view(np.uint8).reshape(streams * steps, cap, 28).copy()).cuda()
        d_counts = torch.from_numpy(counts.copy()).cuda()
        d_gt = torch.from_numpy(gt.view(np.uint8).reshape(streams * steps, gt.shape[1], 20).copy()).cuda()
        d_gt_counts = torch.from_numpy(gt_counts.copy()).cuda()
        for assign in ("greedy", "optimal"):
            for motion in (None, True):
                tracker = images.Tracker(streams, *TRACKER, motion=motion, assign=assign)
                score = images.TrackScore(streams, SCORE_IOU)
                d_out, d_info, d_oc, _ = tracker.update(d_dets, d_counts, steps, "time")
                score.update(d_out, d_info, d_oc, d_gt, d_gt_counts, steps, "time")
                r = score.summary()
                say(f"  {name:74s} {assign:8s} {'suggested' if motion else 'none':10s} {r['gt']:5d} {r['switches']:8d} {r['misses']:7d} "
                    f"{r['false_positives']:7d} {r['mota']:8.4f} {r['motp']:7.4f}")
                if name.startswith("crossing") and motion is None:
                    crossing_without_motion[assign] = r["switches"]
    if crossing_without_motion["optimal"] > crossing_without_motion["greedy"]:
        say(f"# NOTE: without the motion model the OPTIMAL assignment switches the two crossing faces ({crossing_without_motion['optimal']} "
            f"switches) where the greedy match does not ({crossing_without_motion['greedy']}): maximum total IoU exchanges the partners on the "
            "frame the faces overlap most.  With the motion model neither does.  The tracker is as it was; this is the measurement.")


def resources(images, say, parent_lib):
    from tools import isa_hashes
    res = {}
    isa_hashes.disassemble(images.lib_path(), res)
    say("")
    for k in sorted(res):
        if any(name in k for name in ("yfscore", "yfassign")):
            r = res[k]
            say(f"# {k}: {r['vgpr_count']} VGPRs, {r['sgpr_count']} SGPRs, {r['group_segment_fixed_size']} bytes of LDS, "
                f"{r['private_segment_fixed_size']} bytes of scratch, spills {r['sgpr_spill_count']} + {r['vgpr_spill_count']}")
    if parent_lib:
        ours = {name: (h, n) for name, h, n in isa_hashes.hashes(images.lib_path())}
        theirs = {name: (h, n) for name, h, n in isa_hashes.hashes(parent_lib)}
        changed = sorted(name for name in theirs if ours.get(name) != theirs[name])
        new = sorted(name for name in ours if name not in theirs)
        say(f"# the parent commit's libyf_images.so (its sources, the same compiler): {len(theirs)} kernels, {len(theirs) - len(changed)} of them present "
            f"here with an identical instruction hash, {len(changed)} changed or missing {changed}; new here: {new}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_score_bench.txt"))
    args = ap.parse_args()
    import torch
    yf = importlib.import_module("stm32h7-yolo_amd")
    images = importlib.import_module("stm32h7-yolo_amd.images")
    ptq = importlib.import_module("stm32h7-yolo_amd.ptq")
    binding = importlib.import_module("stm32h7-yolo_amd.binding")
    net = yf.Network(device=0).init()
    lib = images.load()
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    dev = "cuda"
    n, cap, out_cap, gt_cap = 4096, 147, 64, 64
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"# libyf_images build {(lib.yf_images_build_id() or b'').decode()}, network build {net.build_id}; {torch.cuda.get_device_name(0)}")
    say(f"# TIME: {args.iters} timed rounds after {args.warmup} warm-up, the two calls interleaved in every round, median of per-call device events")

    real = np.fromfile(os.path.join(ROOT, "tests", "golden", "real_frames_56.bin"), np.int8).reshape(-1, 56, 56, 3)
    rgb56 = (real.astype(np.int16) + 128).astype(np.uint8)
    photos = [np.ascontiguousarray(ptq.resize_linear_u8(f, W, H)[..., ::-1]) for f in rgb56]
    size = (H * W * 3 + 15) // 16 * 16
    desc = np.zeros(n, images.IMAGE_DTYPE)
    desc["offset"], desc["height"], desc["width"], desc["row_stride"] = np.arange(n, dtype=np.int64) * size, H, W, W * 3
    nbytes = int(desc["offset"][-1]) + H * W * 3
    buf = np.zeros(nbytes, np.uint8)
    for i in range(n):
        o = int(desc["offset"][i])
        buf[o:o + H * W * 3] = photos[i % len(photos)].reshape(-1)
    d_px, d_desc = torch.from_numpy(buf).to(dev), torch.from_numpy(desc.view(np.uint8)).to(dev)
    d_frames = torch.empty((n, 56, 56, 3), dtype=torch.int8, device=dev)
    d_heads = torch.empty((n, 7, 7, 18), dtype=torch.int8, device=dev)
    d_dets = torch.empty((n, cap, 28), dtype=torch.uint8, device=dev)
    d_counts = torch.empty(n, dtype=torch.int32, device=dev)
    d_status = torch.empty(n, dtype=torch.int32, device=dev)
    d_out = torch.empty((n, out_cap, 28), dtype=torch.uint8, device=dev)
    d_info = torch.empty((n, out_cap, 16), dtype=torch.uint8, device=dev)
    d_oc = torch.empty(n, dtype=torch.int32, device=dev)
    images.set_decode_tables(*net.decode_tables())
    images.run_decode_ragged_device(net, d_px.data_ptr(), nbytes, "bgr", d_desc.data_ptr(), n, d_frames.data_ptr(), d_heads.data_ptr(),
                                    d_dets.data_ptr(), d_counts.data_ptr(), cap, d_status.data_ptr(), stream=s)
    images.nms_device(d_dets.data_ptr(), d_counts.data_ptr(), n, cap, 0.4, stream=s)
    torch.cuda.synchronize()
    counts = d_counts.cpu().numpy()
    say(f"real  {n} x {W}x{H}, {int(np.clip(counts, 0, cap).sum())} records after the suppression (at most {int(counts.max())} per frame)")

    gains = images.MOTION_GAINS + (0,)
    d_track_state = torch.zeros((n, images.TRACK_MOTION_STATE_BYTES), dtype=torch.uint8, device=dev)
    d_score_state = torch.zeros((n, images.SCORE_STATE_BYTES), dtype=torch.uint8, device=dev)
    d_gt = torch.zeros((n, gt_cap, 20), dtype=torch.uint8, device=dev)
    d_gt_counts = torch.zeros(n, dtype=torch.int32, device=dev)
    # the tracker's output the score reads, kept apart from the output of the timed tracker calls
    d_hyp, d_hyp_info, d_hyp_counts = torch.empty_like(d_out), torch.empty_like(d_info), torch.empty_like(d_oc)

    def track(streams, steps, base, dd, dc, dcap, outs):
        images.track_motion_assign_device(dd.data_ptr(), dc.data_ptr(), streams, steps, "time", dcap, tuple(base) + gains, "optimal",
                                          d_track_state.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), out_cap,
                                          d_status.data_ptr(), s)

    def score(streams, steps):
        images.score_tracks_device(d_hyp.data_ptr(), d_hyp_info.data_ptr(), d_hyp_counts.data_ptr(), out_cap, d_gt.data_ptr(), d_gt_counts.data_ptr(),
                                   gt_cap, streams, steps, "time", SCORE_IOU, d_score_state.data_ptr(), None, d_status.data_ptr(), s)

    def truth_from_tracks():
        """the ground truth of the timing: the reported tracks themselves, ids 1, 2, ... in their order"""
        torch.cuda.synchronize()
        out = d_hyp.cpu().numpy().view(binding.DET_DTYPE).reshape(n, out_cap)
        gt = np.zeros((n, gt_cap), images.GT_TRACK_DTYPE)
        gt["id"] = np.arange(1, gt_cap + 1)[None, :]
        for e in ("x1", "y1", "x2", "y2"):
            gt[e] = out[e][:, :gt_cap]
        d_gt.copy_(torch.from_numpy(gt.view(np.uint8).reshape(n, gt_cap, 20)))
        d_gt_counts.copy_(torch.clamp(d_hyp_counts, 0, gt_cap))
        return int(np.clip(d_hyp_counts.cpu().numpy(), 0, gt_cap).sum())

    def measure(name, what, streams, steps, base, dd, dc, dcap, before=None):
        """round after round the score, then the tracker; `before()` runs ahead of each pair, outside the events"""
        ev = [[], []]
        for it in range(args.warmup + args.iters):
            if before:
                before()
            for k, fn in enumerate((lambda: score(streams, steps), lambda: track(streams, steps, base, dd, dc, dcap, (d_out, d_info, d_oc)))):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                fn()
                b.record(stream)
                if it >= args.warmup:
                    ev[k].append((a, b))
        torch.cuda.synchronize()
        t = [float(np.median([a.elapsed_time(b) for a, b in e])) * 1e3 for e in ev]
        say(f"{name:5s} {what:56s} score {t[0]:9.2f} us; optimal-assign tracker {t[1]:9.2f} us; ratio {t[0] / t[1]:6.2f}")

    default = TRACKER
    for streams, steps in ((n, 1), (64, 64)):
        d_track_state.zero_()
        d_score_state.zero_()
        track(streams, steps, default, d_dets, d_counts, cap, (d_hyp, d_hyp_info, d_hyp_counts))
        rows = truth_from_tracks()
        measure("real", f"{streams} streams x {steps} step(s), {rows} labelled rows, states carried", streams, steps, default, d_dets, d_counts, cap)
        torch.cuda.synchronize()
        st = images.score_summary(d_score_state[:streams].cpu().numpy())
        say(f"# after the last call: matches {st['matches']} of gt {st['gt']}, switches {st['switches']}, misses {st['misses']}")

    # ---- dense ----  64 tracks born at one box, then 64 detections at one box two pixels beside it: all 4096 pairs eligible, one weight
    wcap = 64
    fill, dets = np.zeros((n, wcap), binding.DET_DTYPE), np.zeros((n, wcap), binding.DET_DTYPE)
    for arr, box in ((fill, (10, 10, 49, 59)), (dets, (12, 10, 51, 59))):
        for e, v in zip(("x1", "y1", "x2", "y2"), box):
            arr[e] = v
        arr["conf"] = 0.9
    d_fill = torch.from_numpy(fill.view(np.uint8).reshape(n, wcap, 28)).to(dev)
    d_wdets = torch.from_numpy(dets.view(np.uint8).reshape(n, wcap, 28)).to(dev)
    d_wcounts = torch.full((n,), wcap, dtype=torch.int32, device=dev)
    never = (0.3, 1, 2 ** 31 - 1)
    streams, steps = 64, 64

    def refill():
        d_track_state.zero_()
        d_score_state.zero_()
        track(streams, 1, never, d_fill, d_wcounts, wcap, (d_out, d_info, d_oc))
    # the hypotheses: 64 tracks per frame at the filled box under ids that change from step to step, so that no pair is kept and every
    # step of the score searches the whole table; the ground truth: 64 objects at the box beside it
    refill()
    track(streams, steps, never, d_fill, d_wcounts, wcap, (d_hyp, d_hyp_info, d_hyp_counts))
    torch.cuda.synchronize()
    info = d_hyp_info.cpu().numpy().view(images.TRACK_INFO_DTYPE).reshape(n, out_cap).copy()
    info["id"][:streams * steps] = 1 + (np.arange(out_cap)[None, :] + 64 * np.arange(streams * steps)[:, None])
    d_hyp_info.copy_(torch.from_numpy(info.view(np.uint8).reshape(n, out_cap, 16)))
    gt = np.zeros((n, gt_cap), images.GT_TRACK_DTYPE)
    gt["id"] = np.arange(1, gt_cap + 1)[None, :]
    for e, v in zip(("x1", "y1", "x2", "y2"), (12, 10, 51, 59)):
        gt[e] = v
    d_gt.copy_(torch.from_numpy(gt.view(np.uint8).reshape(n, gt_cap, 20)))
    d_gt_counts.fill_(gt_cap)
    measure("dense", "64 streams x 64 steps, 64 x 64 equal weights, no pair kept", streams, steps, never, d_wdets, d_wcounts, wcap, before=refill)
    torch.cuda.synchronize()
    st = images.score_summary(d_score_state[:streams].cpu().numpy())
    say(f"# after the last call: matches {st['matches']} of gt {st['gt']}, switches {st['switches']} (every new match after the first step is one)")

    resources(images, say, args.parent_lib)
    figures(images, torch, say)
    net.destroy()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
