"""The fp16 image path on the MI355X: fp16 frames bit-exact against ptq.resize_linear_u8 and the 256 halves of pixel / 255., the decode of
float32 logits byte for byte against the host build of the same arithmetic (which tests/test_images_float_host.py checks against numpy),
images -> frames -> fp16 network -> logits -> records -> suppression, the whole against the float32 evaluation of the network within the
project's fp16 tolerance, and images.detect(dtype="fp16")."""
import os
import subprocess
import sys

import numpy as np
import pytest

import float_support as fs
from conftest import ROOT
from images_support import FMT_CH, REF_SIZES, last_error, real_images, suppress, tuples
from images_support import images_after_network, ptq, torch_cuda          # noqa: F401 (fixtures; `images` is images_after_network)

pytestmark = pytest.mark.gpu

HALVES = (np.arange(256) / 255.).astype(np.float16).view(np.uint16)


@pytest.fixture(scope="module")
def host():
    return fs.float_host()


@pytest.fixture(scope="module")
def fp16_network(network):
    network.fp16_init()
    return network


def _layout_set(rng):
    """seeded images in all four formats: the reference's sizes, 1 x 1, 1 x W, H x 1, every third a crop that keeps its parent's row stride"""
    sizes = [(1, 1), (1, 300), (300, 1), (1, 2), (55, 57), (113, 111), (56, 56), (480, 640), (3, 1000)] + [(h, w) for (w, h) in REF_SIZES]
    imgs, fmts = [], []
    for k, (h, w) in enumerate(sizes):
        fmt = k % 4
        C = FMT_CH[fmt]
        if k % 3 == 0:
            img = rng.integers(0, 256, (h + 3, w + 5, C), dtype=np.uint8)[2:2 + h, 3:3 + w]
        else:
            img = rng.integers(0, 256, (h, w, C), dtype=np.uint8)
        imgs.append(img)
        fmts.append(fmt)
    return imgs, fmts


def test_prepare_f16_ragged_formats_strides_and_invalid_descriptors(torch_cuda, images, ptq, host):
    assert np.array_equal(fs.host_halves(host), HALVES)
    imgs, fmts = _layout_set(np.random.default_rng(21))
    for fmt in range(4):
        sel = [imgs[i] for i, f in enumerate(fmts) if f == fmt]
        buf, desc = images.pack_images(sel + sel[:3], fmt)
        n = len(sel)
        C = FMT_CH[fmt]
        assert any(desc["row_stride"][:n] > desc["width"][:n] * C)
        # three invalid descriptors among the valid ones: a stride below a row, an image reaching outside the buffer, a side of 0
        desc["row_stride"][n] = desc["width"][n] * C - 1
        desc["offset"][n + 1] = buf.nbytes - 1
        desc["height"][n + 2] = 0
        order = np.array([n] + list(range(n // 2)) + [n + 1] + list(range(n // 2, n)) + [n + 2])
        desc = desc[order].copy()
        b = fs.F16Batch(torch_cuda, images, None, fmt, desc=desc, buf=buf)
        b.prepare(images)
        torch_cuda.cuda.synchronize()
        got, status = b.frames(), b.d_status.cpu().numpy()
        for j, i in enumerate(order):
            if i >= n:
                assert status[j] == 1 and (got[j] == 0).all(), (fmt, j)
            else:
                assert status[j] == 0, (fmt, j)
                assert np.array_equal(got[j], fs.expect_frame_f16(ptq, HALVES, sel[i], fmt)), (fmt, sel[i].shape)
        assert b.untouched_behind()


def test_prepare_f16_uniform(torch_cuda, images, ptq):
    torch = torch_cuda
    rng = np.random.default_rng(22)
    for fmt, (H, W), n in ((0, (362, 410), 5), (3, (1, 1), 3), (2, (1, 77), 2), (1, (450, 306), 4)):
        C = FMT_CH[fmt]
        # crops of one parent tensor: row stride and frame stride are the parent's
        parent = rng.integers(0, 256, (n, H + 2, W + 3, C), dtype=np.uint8)
        rs, fstride = (W + 3) * C, (H + 2) * (W + 3) * C
        off = rs + 2 * C                                                    # the crop starts at row 1, column 2
        d_px = torch.from_numpy(parent.reshape(-1)).cuda()
        d_frames = torch.full((n + 1, 56, 56, 3), fs.FRAME_FILL, dtype=torch.int16, device="cuda")
        images.prepare_f16_device(d_px.data_ptr() + off, parent.size - off, fmt, H, W, rs, fstride, n, d_frames.data_ptr())
        torch.cuda.synchronize()
        got = d_frames.cpu().numpy().view(np.uint16)
        for i in range(n):
            assert np.array_equal(got[i], fs.expect_frame_f16(ptq, HALVES, parent[i, 1:1 + H, 2:2 + W], fmt)), (fmt, i)
        assert (got[n] == fs.FRAME_FILL).all()
        # frame_stride = 0: the same image n times
        d_frames.fill_(fs.FRAME_FILL)
        images.prepare_f16_device(d_px.data_ptr() + off, parent.size - off, fmt, H, W, rs, 0, n, d_frames.data_ptr())
        torch.cuda.synchronize()
        got = d_frames.cpu().numpy().view(np.uint16)
        want = fs.expect_frame_f16(ptq, HALVES, parent[0, 1:1 + H, 2:2 + W], fmt)
        assert all(np.array_equal(got[i], want) for i in range(n)) and (got[n] == fs.FRAME_FILL).all()


def test_prepare_f16_argument_errors(torch_cuda, images):
    torch = torch_cuda
    lib = images.load()
    H, W, n = 20, 30, 2
    d_px = torch.zeros(n * H * W * 3, dtype=torch.uint8, device="cuda")
    d_frames = torch.full((n * 56 * 56 * 3 + 8,), fs.FRAME_FILL, dtype=torch.int16, device="cuda")
    desc = np.zeros(n, images.IMAGE_DTYPE)
    desc["offset"], desc["height"], desc["width"], desc["row_stride"] = np.arange(n) * H * W * 3, H, W, W * 3
    d_desc = torch.from_numpy(desc.view(np.uint8)).cuda()
    d_status = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    px, fr, bytes_ = d_px.data_ptr(), d_frames.data_ptr(), d_px.numel()
    uniform = lambda *a: lib.yf_images_prepare_f16_device(*a, None)                    # noqa: E731
    ragged = lambda *a: lib.yf_images_prepare_f16_ragged_device(*a, None)              # noqa: E731
    for call, args, word in [(uniform, (px, bytes_, 0, H, W, W * 3, H * W * 3, n, fr + 2), "16-byte aligned"),
                             (uniform, (px, bytes_ - 1, 0, H, W, W * 3, H * W * 3, n, fr), "outside"),
                             (uniform, (px, bytes_, 9, H, W, W * 3, H * W * 3, n, fr), "format"),
                             (uniform, (px, bytes_, 0, H, W, W * 3 - 1, H * W * 3, n, fr), "row_stride"),
                             (uniform, (px, bytes_, 0, 0, W, W * 3, H * W * 3, n, fr), "height and width"),
                             (ragged, (px, bytes_, 0, d_desc.data_ptr(), n, fr + 2, d_status.data_ptr()), "16-byte aligned"),
                             (ragged, (px, bytes_, 4, d_desc.data_ptr(), n, fr, d_status.data_ptr()), "format"),
                             (ragged, (px, bytes_, 0, d_desc.data_ptr(), n, fr, None), "d_status"),
                             (ragged, (px, bytes_, 0, d_desc.data_ptr() + 4, n, fr, d_status.data_ptr()), "d_images")]:
        assert call(*args) <= 0
        assert word in last_error(lib), (word, last_error(lib))
    torch.cuda.synchronize()
    assert (d_frames == fs.FRAME_FILL).all().item() and (d_status == -7).all().item()
    assert uniform(px, bytes_, 0, H, W, W * 3, H * W * 3, 0, fr) == 0 and ragged(px, bytes_, 0, d_desc.data_ptr(), 0, fr, d_status.data_ptr()) == 0
    torch.cuda.synchronize()
    assert (d_frames == fs.FRAME_FILL).all().item()


def _decode_inputs():
    """the logits of the host test (real frames, seeded, specials) tiled to 4096 frames"""
    base = np.concatenate([fs.fp32_logits(fs.real_frames_u8()), fs.seeded_logits(), fs.special_logits()])
    return base[np.arange(4096) % base.shape[0]].copy()


@pytest.mark.parametrize("cap", [147, 20])
def test_decode_f32_scalar_scales_against_the_host_build(torch_cuda, images, host, cap):
    torch = torch_cuda
    logits = _decode_inputs()
    n = logits.shape[0]
    d_logits = torch.from_numpy(logits).cuda()
    total = 0
    for ws, hs in (fs.scales_of(410, 362), (1.0, 1.0), fs.scales_of(16384, 16384)):
        d_dets = torch.full((n + 1, cap, 28), 0xA5, dtype=torch.uint8, device="cuda")
        d_counts = torch.full((n + 1,), -7, dtype=torch.int32, device="cuda")
        images.decode_f32_device(d_logits.data_ptr(), n, d_dets.data_ptr(), d_counts.data_ptr(), cap, w_scale=ws, h_scale=hs)
        torch.cuda.synchronize()
        dets, counts, raw = fs.device_records(d_dets, d_counts, cap)
        total += fs.check_records_against_host(host, logits, (ws, hs), dets, counts, raw, cap, frames=range(n))
        assert counts[n] == -7 and (raw[n] == 0xA5).all()
        assert (counts[:n] > cap).any() == (cap < 147) and counts[:n].max() == 147
    assert total > 3 * 4096 * 10


def test_decode_f32_ragged_scales_status_and_sides(torch_cuda, images, host):
    torch = torch_cuda
    logits = _decode_inputs()
    n, cap = logits.shape[0], 147
    desc = np.zeros(n, images.IMAGE_DTYPE)
    sizes = [REF_SIZES[i % len(REF_SIZES)] for i in range(n)]
    desc["width"], desc["height"] = [s[0] for s in sizes], [s[1] for s in sizes]
    desc["width"][5::97] = 16385
    desc["height"][7::97] = 0
    desc["width"][9::97] = -3
    status = np.zeros(n, np.int32)
    status[11::97] = 1
    bad = (desc["width"] < 1) | (desc["width"] > 16384) | (desc["height"] < 1) | (status != 0)
    assert bad.sum() > 100
    d_logits, d_desc, d_status = torch.from_numpy(logits).cuda(), torch.from_numpy(desc.view(np.uint8)).cuda(), torch.from_numpy(status).cuda()
    d_dets = torch.full((n, cap, 28), 0xA5, dtype=torch.uint8, device="cuda")
    d_counts = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    images.decode_f32_ragged_device(d_logits.data_ptr(), d_desc.data_ptr(), n, d_dets.data_ptr(), d_counts.data_ptr(), cap,
                                    d_status=d_status.data_ptr())
    torch.cuda.synchronize()
    dets, counts, raw = fs.device_records(d_dets, d_counts, cap)
    assert (counts[bad] == 0).all() and (raw[bad] == 0xA5).all()
    good = np.nonzero(~bad)[0]
    scales = [fs.scales_of(w, h) for (w, h) in sizes]
    assert fs.check_records_against_host(host, logits, scales, dets, counts, raw, cap, frames=good) > 4096 * 10
    # without the status array only the sides count
    d_counts.fill_(-7)
    images.decode_f32_ragged_device(d_logits.data_ptr(), d_desc.data_ptr(), n, d_dets.data_ptr(), d_counts.data_ptr(), cap)
    torch.cuda.synchronize()
    c2 = d_counts.cpu().numpy()
    flagged = (status != 0) & (desc["width"] >= 1) & (desc["width"] <= 16384) & (desc["height"] >= 1)
    assert np.array_equal(c2[~flagged], counts[~flagged]) and (c2[flagged] > 0).any()
    # argument errors: nothing launched
    lib = images.load()
    d_counts.fill_(-7)
    for args, word in [((d_logits.data_ptr() + 2, n, 1.0, 1.0, d_dets.data_ptr(), d_counts.data_ptr(), cap, None), "d_logits"),
                       ((d_logits.data_ptr(), n, 1.0, 1.0, d_dets.data_ptr(), d_counts.data_ptr(), 148, None), "cap"),
                       ((d_logits.data_ptr(), n, 1.0, 1.0, d_dets.data_ptr(), d_counts.data_ptr(), 0, None), "cap"),
                       ((d_logits.data_ptr(), -1, 1.0, 1.0, d_dets.data_ptr(), d_counts.data_ptr(), cap, None), "n < 0"),
                       ((d_logits.data_ptr(), n, 1.0, 1.0, None, d_counts.data_ptr(), cap, None), "d_dets")]:
        assert lib.yf_images_decode_f32_device(*args) <= 0 and word in last_error(lib), (word, last_error(lib))
    assert lib.yf_images_decode_f32_device(d_logits.data_ptr(), 0, 1.0, 1.0, d_dets.data_ptr(), d_counts.data_ptr(), cap, None) == 0
    torch.cuda.synchronize()
    assert (d_counts == -7).all().item()


def _separate_logits(torch, network, d_frames, n):
    d_out = torch.zeros((n, 7, 7, 18), dtype=torch.float32, device="cuda")
    network.fp16_run_device(d_frames.data_ptr(), d_out.data_ptr(), n)
    torch.cuda.synchronize()
    return d_out


def _check_chain(torch, images, network, host, frames_dev, logits_dev, d_dets, d_counts, n, cap, scales):
    """logits = a separate fp16 launch on the frames, bit for bit; records = the host decode of those logits; suppression at 0.4 = the
    restatement on the same records.  Returns the records per frame."""
    sep = _separate_logits(torch, network, frames_dev, n)
    assert torch.equal(sep.view(torch.int32), logits_dev[:n].view(torch.int32))
    logits = logits_dev[:n].cpu().numpy()
    dets, counts, raw = fs.device_records(d_dets, d_counts, cap)
    fs.check_records_against_host(host, logits, scales, dets, counts, raw, cap, frames=range(n))
    recs = [tuples(dets[i, :min(int(counts[i]), cap)]) for i in range(n)]
    d_out = torch.full_like(d_dets, 0xA5)
    d_oc = torch.full_like(d_counts, -7)
    images.nms_device(d_dets.data_ptr(), d_counts.data_ptr(), n, cap, 0.4, d_out.data_ptr(), d_oc.data_ptr())
    torch.cuda.synchronize()
    out, oc, _ = fs.device_records(d_out, d_oc, cap)
    assert [tuples(out[i, :oc[i]]) for i in range(n)] == [suppress(r, 0.4) for r in recs]
    return recs


def test_run_decode_f16_ragged_on_real_content(fp16_network, torch_cuda, images, ptq, host):
    torch = torch_cuda
    imgs = real_images(ptq)
    buf, desc = images.pack_images(imgs + [imgs[0]], "bgr")
    bad = len(imgs)
    desc["row_stride"][bad] = desc["width"][bad] * 3 - 1                    # stride below a row: status 1, a frame of zeros, count 0
    b = fs.F16Batch(torch, images, None, "bgr", desc=desc, buf=buf)
    b.run_decode(images, fp16_network)
    torch.cuda.synchronize()
    assert b.d_status.cpu().numpy()[:b.n].tolist() == [0] * bad + [1] and b.untouched_behind()
    got = b.frames()
    for i, im in enumerate(imgs):
        assert np.array_equal(got[i], fs.expect_frame_f16(ptq, HALVES, im, 0)), i
    assert (got[bad] == 0).all() and b.d_counts[bad].item() == 0
    scales = [fs.scales_of(im.shape[1], im.shape[0]) for im in imgs]
    recs = _check_chain(torch, images, fp16_network, host, b.d_frames, b.d_logits, b.d_dets[:bad], b.d_counts[:bad], bad, b.cap, scales)
    assert sum(len(r) for r in recs) >= 40


@pytest.mark.parametrize("n", [1, 3, 513])
def test_run_decode_f16_uniform_equals_ragged(fp16_network, torch_cuda, images, ptq, host, n):
    torch = torch_cuda
    H, W, cap = 362, 410, 147
    real = real_images(ptq)[0]
    g = torch.Generator(device="cuda").manual_seed(5)
    noise = torch.randint(-24, 25, (64, H, W, 3), device="cuda", generator=g, dtype=torch.int16)
    variants = (torch.from_numpy(real).cuda().to(torch.int16)[None] + noise).clamp(0, 255).to(torch.uint8)
    px = variants[torch.arange(n, device="cuda") % 64].contiguous()
    fstride, rs = H * W * 3, W * 3
    mk = lambda: (torch.full((n + 1, 56, 56, 3), fs.FRAME_FILL, dtype=torch.int16, device="cuda"),                   # noqa: E731
                  torch.full((n + 1, 7, 7, 18), 7.0, dtype=torch.float32, device="cuda"),
                  torch.full((n + 1, cap, 28), 0xA5, dtype=torch.uint8, device="cuda"), torch.full((n + 1,), -7, dtype=torch.int32, device="cuda"))
    f_u, l_u, d_u, c_u = mk()
    images.run_decode_f16_device(fp16_network, px.data_ptr(), px.numel(), "bgr", H, W, rs, fstride, n, f_u.data_ptr(), l_u.data_ptr(),
                                 d_u.data_ptr(), c_u.data_ptr(), cap)
    desc = np.zeros(n, images.IMAGE_DTYPE)
    desc["offset"], desc["height"], desc["width"], desc["row_stride"] = np.arange(n) * fstride, H, W, rs
    d_desc = torch.from_numpy(desc.view(np.uint8)).cuda()
    f_r, l_r, d_r, c_r = mk()
    st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    images.run_decode_f16_ragged_device(fp16_network, px.data_ptr(), px.numel(), "bgr", d_desc.data_ptr(), n, f_r.data_ptr(), l_r.data_ptr(),
                                        d_r.data_ptr(), c_r.data_ptr(), cap, st.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(f_u, f_r) and torch.equal(l_u.view(torch.int32), l_r.view(torch.int32)) and torch.equal(c_u, c_r) and torch.equal(d_u, d_r)
    assert (st == 0).all().item()
    assert (f_u[n] == fs.FRAME_FILL).all().item() and (l_u[n] == 7.0).all().item() and (d_u[n] == 0xA5).all().item() and c_u[n].item() == -7
    host_px = px.cpu().numpy()
    got = f_u.cpu().numpy().view(np.uint16)
    for i in sorted({0, n // 2, n - 1}):
        assert np.array_equal(got[i], fs.expect_frame_f16(ptq, HALVES, host_px[i], 0)), i
    recs = _check_chain(torch, images, fp16_network, host, f_u, l_u, d_u[:n], c_u[:n], n, cap, fs.scales_of(W, H))
    assert sum(len(r) for r in recs) > 0


def test_run_decode_f16_without_fp16_init():
    """a fresh process, so that the session's network keeps its state: tests/dev/float_without_init.py"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "dev", "float_without_init.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "float-without-init ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_boxes_against_the_float32_network(fp16_network, torch_cuda, images, ptq):
    """End to end against float32: the records of the fp16 path on the real-content batch against the restated decode of the float32
    evaluation of the network (oracle/np_fp32.py) on the float32 frames.  With d = 2e-2 + 2e-2 |t| for a logit t (the project's tolerance
    for this network): a candidate is compared iff its float32 confidence logit is farther than d from ln(7/3); compared
    candidates fire on both sides or on neither; an edge differs by at most scale * (2 d_xy + wh * (e^(d_wh) - 1) / 2) + 1 pixels
    (d(8 sigmoid) <= 2 d, the exponential's derivative, one for the truncation)."""
    torch = torch_cuda
    imgs = real_images(ptq)
    b = fs.F16Batch(torch, images, imgs, "bgr")
    b.run_decode(images, fp16_network)
    torch.cuda.synchronize()
    dets, counts, _ = fs.device_records(b.d_dets, b.d_counts, b.cap)
    frames_u8 = np.stack([ptq.resize_linear_u8(np.ascontiguousarray(im[..., ::-1]), 56, 56) for im in imgs])
    ref = fs.fp32_logits(frames_u8)
    left_out = compared_firing = worst_use = 0
    for f, im in enumerate(imgs):
        ws, hs = fs.scales_of(im.shape[1], im.shape[0])
        want, _ = fs.decode_restated(ref[f], f, ws, hs)
        t = ref[f].reshape(49, 3, 6).transpose(1, 0, 2).reshape(147, 6).astype(np.float64)      # candidate order (anchor, row, col)
        d = 2e-2 + 2e-2 * np.abs(t)
        clear = np.abs(t[:, 4] - fs.LN_7_3) > d[:, 4]
        left_out += int((~clear).sum())
        cand = lambda r: (r["anchor"].astype(int) * 7 + r["row"]) * 7 + r["col"]                   # noqa: E731
        got = dets[f, :counts[f]]
        fire_ref, fire_got = np.zeros(147, bool), np.zeros(147, bool)
        fire_ref[cand(want)] = True
        fire_got[cand(got)] = True
        assert np.array_equal(fire_ref[clear], fire_got[clear]), f
        by_cand = {int(c): r for c, r in zip(cand(got), got)}
        for r in want:
            i = int(cand(r))
            if not clear[i]:
                continue
            compared_firing += 1
            a = int(r["anchor"])
            w, h = np.exp(t[i, 2]) * fs.ANCHORS[a][0], np.exp(t[i, 3]) * fs.ANCHORS[a][1]
            bound_x = ws * (2 * d[i, 0] + w * (np.exp(d[i, 2]) - 1) / 2) + 1
            bound_y = hs * (2 * d[i, 1] + h * (np.exp(d[i, 3]) - 1) / 2) + 1
            g = by_cand[i]
            for e, bound in (("x1", bound_x), ("x2", bound_x), ("y1", bound_y), ("y2", bound_y)):
                diff = abs(int(g[e]) - int(r[e]))
                worst_use = max(worst_use, diff / bound)
                assert diff <= bound, (f, i, e, int(g[e]), int(r[e]), bound)
    print(f"[fp16 boxes vs float32] {compared_firing} firing candidates compared, {left_out} of {147 * len(imgs)} left out, "
          f"worst use of the edge bound {worst_use:.2f}")
    assert left_out <= 0.01 * 147 * len(imgs) and compared_firing >= 40


def test_detect_with_dtype_fp16(fp16_network, yf, torch_cuda, images, ptq):
    torch = torch_cuda
    imgs = real_images(ptq)
    b = fs.F16Batch(torch, images, imgs, "bgr")
    b.run_decode(images, fp16_network)
    torch.cuda.synchronize()
    dets, counts, _ = fs.device_records(b.d_dets, b.d_counts, b.cap)
    recs = [tuples(dets[i, :counts[i]]) for i in range(b.n)]
    plain = images.detect(fp16_network, imgs, "bgr", dtype="fp16")
    assert [bx.tolist() for bx in plain] == [[[r[6], r[7], r[8], r[9]] for r in rr] for rr in recs]
    boxes = images.detect(fp16_network, imgs, "bgr", dtype="fp16", iou_threshold=0.4)
    assert [bx.tolist() for bx in boxes] == [[[r[6], r[7], r[8], r[9]] for r in suppress(rr, 0.4)] for rr in recs]
    assert all(bx.dtype == np.int32 and bx.shape[1] == 4 for bx in boxes)
    assert 0 < sum(len(x) for x in boxes) <= sum(len(x) for x in plain)
    capped = images.detect(fp16_network, imgs, "bgr", dtype="fp16", cap=1)
    assert [bx.tolist() for bx in capped] == [[[r[6], r[7], r[8], r[9]] for r in rr[:1]] for rr in recs]
    with pytest.raises(ValueError):
        images.detect(fp16_network, imgs, "bgr", dtype="fp16", size=160)
    with pytest.raises(ValueError):
        images.detect(fp16_network, imgs, "bgr", dtype="fp32")
    # int8 and the default: what they return today (run_decode_ragged_device on the same batch)
    from images_support import Batch
    b8 = Batch(torch, images, imgs, "bgr")
    b8.run_decode(images, fp16_network)
    recs8, _ = b8.records(yf)
    want8 = [[[r[6], r[7], r[8], r[9]] for r in rr] for rr in recs8]
    assert [bx.tolist() for bx in images.detect(fp16_network, imgs, "bgr")] == want8
    assert [bx.tolist() for bx in images.detect(fp16_network, imgs, "bgr", dtype="int8")] == want8
    assert want8 != [bx.tolist() for bx in plain]                          # two different networks
