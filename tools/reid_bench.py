#!/usr/bin/env python3
"""The appearance descriptors and the re-identification on the GPU (GPU TOOL; bench.py is not involved), in three parts, all reported and
none gated: there is no earlier number for either operation.

TIME, the calls of a pair interleaved in one loop, round after round, device events around every call, warm-up first, the median of the
timed calls, each figure measured once on one MI355X:

    describe  yf_images_describe_records_device (the scan and one workgroup per record) beside yf_images_blur_records_device at grid 8
              (the scan, the means, the paint) on the real-content records: 4096 pictures of 410x362 (the 27 real frames of tests/golden
              upscaled to that size, repeated), the ragged run at 56x56 and the suppression at 0.4.  THE BLUR'S MEANS LAUNCH ALONE CANNOT
              BE TIMED through the C-ABI: the blur figure is that of the parent commit's whole call, and the row says so.
    reid      yf_images_reid_device beside one launch of yf_images_track_motion_device on the same records at 4096 streams x 1 step and
              64 x 64, the states carried from call to call; the descriptors are those of the tracker's boxes.

Then the kernels' registers, LDS and scratch (tools/isa_hashes.py), and with --parent-lib the libyf_images.so of the parent commit, built
from its sources with the same compiler: every kernel of it must be present with an identical instruction hash.

EFFECT, on SYNTHETIC TEXTURED CLIPS, NOT VIDEO: faces as random smooth textures pasted into noise pictures, with a brightness drift and
+- 1 pixel of box jitter; the boxes are fed to the tracker directly, because the network does not detect textures.  Three kinds of clip --
an occlusion longer than max_misses, a face that leaves the picture and returns, a different face that takes a lost one's place --, eight
seeds each: switches and MOTA with and without `ReId`, and the largest same-face and the smallest different-face distance seen, between
which images.REID_MAX_DISTANCE is set.  --distances-only prints that part from the host build alone (no GPU).

    python tools/reid_bench.py [--iters 30] [--warmup 5] [--parent-lib PATH] [--distances-only] [--out profiles/reid_bench.txt]
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
CLIP_W, CLIP_H, FACE, STEPS, SEEDS = 160, 96, 32, 30, 8
TRACKER, SCORE_IOU = (0.3, 1, 5), 0.5
KINDS = ("occlusion", "leaves", "replaced")


def clip(kind, seed):
    """one stream of STEPS BGR pictures of noise with textured faces: face 1 stays on the left; face 2 on the right is hidden on steps
    8 .. 19 (occlusion), or walks out of the picture to the right and back in (leaves); with `replaced` a different face 3 appears in its
    place after the gap.  The brightness drifts by a level every three steps and every reported box jitters by +- 1 pixel.
    -> (pictures, boxes[t], truths[t], faces[t]): faces[t] the face shown in each box"""
    import reid_support as rs
    rng = np.random.default_rng(seed)
    tex = {k: rs.texture(np.random.default_rng(seed * 100 + k), FACE, FACE) for k in (1, 2, 3)}
    pictures, boxes, truths, faces = [], [], [], []
    for t in range(STEPS):
        pic = rs.noise(rng, CLIP_H, CLIP_W, 3)
        shown = [(1, 20, 30)]
        if kind == "leaves":
            x = 100 + 12 * t if t < 8 else 100 + 12 * max(0, 27 - t)
            if x <= CLIP_W - 12 and not 8 <= t < 20:
                shown.append((2, x, 40))
        elif t < 8:
            shown.append((2, 100, 40))
        elif t >= 20:
            shown.append((3 if kind == "replaced" else 2, 100, 40))
        frame_boxes, frame_truth = [], []
        for face, x, y in shown:
            lit = np.clip(tex[face].astype(np.int32) + (t // 3 - 4), 0, 255).astype(np.uint8)
            w = min(FACE, CLIP_W - x)
            pic[y:y + FACE, x:x + w] = lit[:, :w]
            jx, jy = (int(v) for v in rng.integers(-1, 2, 2))
            frame_boxes.append((x + jx, y + jy, x + jx + FACE - 1, y + jy + FACE - 1))
            frame_truth.append((face, x, y, x + FACE - 1, y + FACE - 1))
        pictures.append(pic)
        boxes.append(frame_boxes)
        truths.append(frame_truth)
        faces.append([face for face, _, _ in shown])
    return pictures, boxes, truths, faces


def distances(say):
    """the same-face and different-face distances of the clips, from the host build's descriptors of the reported boxes: for every clip
    the descriptors of a face after the gap against those of the same face before it -- apart where one of the two shows the face cut by
    the picture's border, whose region is clamped and is no longer the face's --, and of face 1 against faces 2 / 3 and face 2 against
    face 3 at all times"""
    import reid_support as rs
    same, cut, other = [], [], []
    dist = rs.ptq().reid_distance
    for kind in KINDS:
        for seed in range(SEEDS):
            pictures, boxes, truths, faces = clip(kind, 9800 + seed)
            got = rs.describe_host_run(rs.Batch("clip", "bgr", pictures, boxes, None, 2))
            d = {}
            for t in range(STEPS):
                for k, face in enumerate(faces[t]):
                    if got.desc["flags"][t, k] & 1:
                        d.setdefault(face, []).append((t, got.desc["v"][t, k], truths[t][k][3] <= CLIP_W - 1))
            for rows in d.values():
                for ta, a, wa in rows:
                    for tb, b, wb in rows:
                        if ta < 8 and tb >= 20:
                            (same if wa and wb else cut).append(dist(a, b))
            other += [dist(a, b) for _, a, _ in d.get(2, []) for _, b, _ in d.get(3, [])]
            other += [dist(a, b) for _, a, _ in d[1][::5] for f in (2, 3) for _, b, _ in d.get(f, [])[::2]]
    say("")
    say("# DISTANCES on the synthetic textured clips (host build; the device computes the same bytes): a face before the gap against the")
    say("# same face after it, and against a different face.  Not video.")
    say(f"  same face, whole in the picture:   {len(same):6d} pairs, largest  {max(same):7d}, median {int(np.median(same)):7d}")
    say(f"  different face:                    {len(other):6d} pairs, smallest {min(other):7d}, median {int(np.median(other)):7d}")
    say(f"  same face, cut by the border:      {len(cut):6d} pairs, largest  {max(cut):7d}, median {int(np.median(cut)):7d}  (the clamped region is not the")
    say("                                     face's: such a return is re-identified only once the face is whole again, if the track is still fresh)")
    return max(same), min(other)


def effect(images, torch, say):
    import reid_support as rs
    import track_support as ts
    say("")
    say("# EFFECT: synthetic textured clips, not video.  No labelled video is at hand; nothing below says how the stage does on real footage.")
    say(f"# {SEEDS} seeds per kind as streams of one call, {STEPS} steps; tracker (match_iou, min_hits, max_misses) = {TRACKER}; score IoU {SCORE_IOU};")
    say(f"# ReId(max_distance={images.REID_MAX_DISTANCE}, max_age={images.REID_MAX_AGE}, blend={images.REID_BLEND})")
    say(f"# {'clip':44s} {'reid':5s} {'gt':>5s} {'switches':>8s} {'misses':>7s} {'false+':>7s} {'MOTA':>8s} {'ids of the right-hand face(s)':>30s}")
    for kind in KINDS:
        made = [clip(kind, 9800 + seed) for seed in range(SEEDS)]
        pictures = [made[s][0][t] for t in range(STEPS) for s in range(SEEDS)]              # time-major
        dets, counts = ts.lay_out([[(b, None) for b in m[1]] for m in made], 4, ts.TIME)
        gt, gt_counts = images.pack_track_truth([made[s][2][t] for t in range(STEPS) for s in range(SEEDS)])
        buf, descs, _, _ = rs.pack(rs.Batch("clips", "bgr", pictures, [[] for _ in pictures], None, 8))
        n = SEEDS * STEPS
        d_dets = torch.from_numpy(dets.view(np.uint8).reshape(n, 4, 28).copy()).cuda()
        d_counts = torch.from_numpy(counts.copy()).cuda()
        d_gt = torch.from_numpy(gt.view(np.uint8).reshape(n, gt.shape[1], 20).copy()).cuda()
        d_gt_counts = torch.from_numpy(gt_counts.copy()).cuda()
        d_px, d_pictures = torch.from_numpy(buf.copy()).cuda(), torch.from_numpy(descs.view(np.uint8).reshape(n, -1).copy()).cuda()
        for with_reid in (False, True):
            tracker, score = images.Tracker(SEEDS, *TRACKER), images.TrackScore(SEEDS, SCORE_IOU)
            d_out, d_info, d_oc, _ = tracker.update(d_dets, d_counts, STEPS, "time", out_cap=8)
            if with_reid:
                images.ReId(SEEDS).update(d_px, buf.size, "bgr", d_pictures, d_out, d_info, d_oc, STEPS, "time")
            score.update(d_out, d_info, d_oc, d_gt, d_gt_counts, STEPS, "time")
            r = score.summary()
            info, oc = d_info.cpu().numpy().view(images.TRACK_INFO_DTYPE).reshape(n, 8), d_oc.cpu().numpy()
            per = [len({int(info[t * SEEDS + s, k]["id"]) for t in range(STEPS) for k in range(1, int(oc[t * SEEDS + s]))}) for s in range(SEEDS)]
            say(f"  {kind:44s} {'yes' if with_reid else 'no':5s} {r['gt']:5d} {r['switches']:8d} {r['misses']:7d} {r['false_positives']:7d} "
                f"{r['mota']:8.4f} {str(per):>30s}")
    say("# (`replaced` shows a DIFFERENT face after the gap: two ids per stream are right there, and a switch would be wrong either way.)")


def resources(images, say, parent_lib):
    from tools import isa_hashes
    res = {}
    isa_hashes.disassemble(images.lib_path(), res)
    say("")
    for k in sorted(res):
        if any(name in k for name in ("yfreid", "yfdescribe")):
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
    else:
        say("# no --parent-lib given: the instruction hashes of the pre-existing kernels were NOT compared in this run")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--distances-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reid_bench.txt"))
    args = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    if args.distances_only:
        distances(say)
        return
    import torch
    yf = importlib.import_module("stm32h7-yolo_amd")
    images = importlib.import_module("stm32h7-yolo_amd.images")
    ptq = importlib.import_module("stm32h7-yolo_amd.ptq")
    net = yf.Network(device=0).init()
    lib = images.load()
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    dev = "cuda"
    n, cap, out_cap = 4096, 147, 64

    say(f"# libyf_images build {(lib.yf_images_build_id() or b'').decode()}, network build {net.build_id}; {torch.cuda.get_device_name(0)}")
    say(f"# TIME: {args.iters} timed rounds after {args.warmup} warm-up, the two calls of a pair interleaved in every round, median of per-call device")
    say("# events; every figure measured once on one MI355X; reported, not gated")

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
    d_first = torch.empty(n + 1, dtype=torch.int32, device=dev)
    images.set_decode_tables(*net.decode_tables())
    images.run_decode_ragged_device(net, d_px.data_ptr(), nbytes, "bgr", d_desc.data_ptr(), n, d_frames.data_ptr(), d_heads.data_ptr(),
                                    d_dets.data_ptr(), d_counts.data_ptr(), cap, d_status.data_ptr(), stream=s)
    images.nms_device(d_dets.data_ptr(), d_counts.data_ptr(), n, cap, 0.4, stream=s)
    torch.cuda.synchronize()
    counts = d_counts.cpu().numpy()
    records = int(np.clip(counts, 0, cap).sum())
    say(f"real  {n} x {W}x{H}, {records} records after the suppression (at most {int(counts.max())} per frame)")

    def timed(fns):
        ev = [[] for _ in fns]
        for it in range(args.warmup + args.iters):
            for k, fn in enumerate(fns):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                fn()
                b.record(stream)
                if it >= args.warmup:
                    ev[k].append((a, b))
        torch.cuda.synchronize()
        return [float(np.median([a.elapsed_time(b) for a, b in e])) * 1e3 for e in ev]

    # ---- describe beside the blur at grid 8 ----  (the blur writes the pictures: it runs on a copy)
    d_px_blur = d_px.clone()
    d_rec_desc = torch.empty((n, cap, 68), dtype=torch.uint8, device=dev)
    room = images.blur_workspace(n * cap, 8)
    d_work = torch.empty(room, dtype=torch.uint8, device=dev)
    t = timed([lambda: images.describe_records_device(d_px.data_ptr(), nbytes, "bgr", d_desc.data_ptr(), d_dets.data_ptr(), d_counts.data_ptr(), n, cap,
                                                      d_rec_desc.data_ptr(), d_first.data_ptr(), d_status.data_ptr(), stream=s),
               lambda: images.blur_records_device(d_px_blur.data_ptr(), nbytes, "bgr", d_desc.data_ptr(), d_dets.data_ptr(), d_counts.data_ptr(), n, cap,
                                                  d_work.data_ptr(), room, n * cap, d_first.data_ptr(), d_status.data_ptr(), grid=8, stream=s)])
    say(f"describe  {records} records: describe (scan + records) {t[0]:9.2f} us; the whole blur call at grid 8 (scan + means + paint) {t[1]:9.2f} us; "
        f"ratio {t[0] / t[1]:5.2f}")
    say("#         the blur's means launch alone: NOT MEASURED (no entry launches it alone); the blur figure above is the parent's whole call")
    valid = int((d_rec_desc.cpu().numpy().view(images.FACE_DESC_DTYPE).reshape(n, cap)["flags"] == 1).sum())
    say(f"#         {valid} of the records have a valid descriptor (a region of at least 8 x 8 pixels)")
    del d_px_blur, d_work

    # ---- reid beside the tracker with a motion model ----
    gains = images.MOTION_GAINS + (0,)
    d_track_state = torch.zeros((n, images.TRACK_MOTION_STATE_BYTES), dtype=torch.uint8, device=dev)
    d_reid_state = torch.zeros((n, images.REID_STATE_BYTES), dtype=torch.uint8, device=dev)
    d_out = torch.empty((n, out_cap, 28), dtype=torch.uint8, device=dev)
    d_info = torch.empty((n, out_cap, 16), dtype=torch.uint8, device=dev)
    d_info_out = torch.empty_like(d_info)
    d_oc = torch.empty(n, dtype=torch.int32, device=dev)
    d_out_desc = torch.empty((n, out_cap, 68), dtype=torch.uint8, device=dev)
    params = (images.REID_MAX_DISTANCE, images.REID_MAX_AGE, images.REID_BLEND)
    for streams, steps in ((n, 1), (64, 64)):
        d_track_state.zero_()
        d_reid_state.zero_()

        def track():
            images.track_motion_device(d_dets.data_ptr(), d_counts.data_ptr(), streams, steps, "time", cap, TRACKER + gains, d_track_state.data_ptr(),
                                       d_out.data_ptr(), d_info.data_ptr(), d_oc.data_ptr(), out_cap, d_status.data_ptr(), s)

        def reid():
            images.reid_device(d_info.data_ptr(), d_oc.data_ptr(), d_out_desc.data_ptr(), out_cap, streams, steps, "time", params, d_reid_state.data_ptr(),
                               d_info_out.data_ptr(), None, None, s)
        track()
        images.describe_records_device(d_px.data_ptr(), nbytes, "bgr", d_desc.data_ptr(), d_out.data_ptr(), d_oc.data_ptr(), n, out_cap,
                                       d_out_desc.data_ptr(), d_first.data_ptr(), d_status.data_ptr(), stream=s)
        t = timed([reid, track])
        say(f"reid  {streams} streams x {steps} step(s), states carried: reid {t[0]:9.2f} us; tracker with motion model {t[1]:9.2f} us; ratio {t[0] / t[1]:5.2f}")
        st = d_reid_state[:streams].cpu().numpy().view(images.REID_STATE_DTYPE).reshape(streams)
        say(f"#     after the last call: {int((st['entry']['id'] != 0).sum())} entries in use over {streams} streams")
    say("# not tuned: the greedy's inner loop rereads its column of the table for every pair it takes")

    resources(images, say, args.parent_lib)
    lo, hi = distances(say)
    say(f"# images.REID_MAX_DISTANCE = {images.REID_MAX_DISTANCE}: A CHOICE between these two, made on synthetic textures; nothing is measured on labelled video")
    if not lo < images.REID_MAX_DISTANCE < hi:
        say("# WARNING: REID_MAX_DISTANCE does not lie between the two")
    effect(images, torch, say)
    net.destroy()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
