"""libyf_images on the MI355X: frames bit-exact against ptq.resize_linear_u8 (the restatement of cv2.resize INTER_LINEAR, unpinned against a
real cv2) for every tap table, every pixel format and layout, and on through the network to records equal to the oracle's decode with each
image's own scales."""
import numpy as np
import pytest

from images_support import FMT_CH, REF_SIZES, Batch, expect_frame, host_lib, real_images
from images_support import images_after_network, ptq, torch_cuda          # noqa: F401 (fixtures; `images` is images_after_network)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("out", [56, 160])
def test_every_tap_table_on_the_device(torch_cuda, images, ptq, out):
    """1 x W for every W in 1..4096 and H x 1 for every H in 1..4096 in one ragged batch each.  Expected frames: the host build of the same
    arithmetic (tests/test_images_host.py proves it equal to ptq.resize_linear_u8 for every side up to 8192), and ptq itself on every 31st."""
    host = host_lib()
    rng = np.random.default_rng(out)
    for shape_of in (lambda s: (1, s, 3), lambda s: (s, 1, 3)):
        imgs = [rng.integers(0, 256, shape_of(s), dtype=np.uint8) for s in range(1, 4097)]
        b = Batch(torch_cuda, images, imgs, 0, out)
        b.prepare(images)
        torch_cuda.cuda.synchronize()
        got = b.d_frames.cpu().numpy()
        assert (b.d_status.cpu().numpy() == 0).all()
        for i, img in enumerate(imgs):
            rgb = np.ascontiguousarray(img[..., ::-1])
            want = np.empty((out, out, 3), np.uint8)
            host.yfi_resize_host(rgb.ctypes.data, rgb.shape[0], rgb.shape[1], 3, rgb.strides[0], out, out, want.ctypes.data)
            if i % 31 == 0:
                assert np.array_equal(want, ptq.resize_linear_u8(rgb, out, out))
            assert np.array_equal(got[i], (want.astype(np.int16) - 128).astype(np.int8)), (img.shape, out)


def _layout_set(rng):
    """~40 seeded images in all four formats, with padded row strides and crops out of larger pictures"""
    sizes = [(1, 1), (55, 57), (112, 112), (113, 111)] + [(h, w) for (w, h) in REF_SIZES] + [(480, 640), (1080, 1920), (2, 3), (56, 56),
                                                                                            (160, 160), (3, 1000), (1000, 3)]
    imgs, fmts = [], []
    for k, (h, w) in enumerate(sizes):
        fmt = k % 4
        C = FMT_CH[fmt]
        if k % 3 == 0:          # padded rows: a crop out of a larger picture
            parent = rng.integers(0, 256, (h + 3, w + 5, C), dtype=np.uint8)
            img = parent[2:2 + h, 3:3 + w]
        else:
            img = rng.integers(0, 256, (h, w, C), dtype=np.uint8)
        imgs.append(img)
        fmts.append(fmt)
    return imgs, fmts


@pytest.mark.parametrize("out", [56, 160])
def test_formats_strides_and_offsets(yf, network, oracle, torch_cuda, images, ptq, out):
    rng = np.random.default_rng(11)
    imgs, fmts = _layout_set(rng)
    frames = {}
    for fmt in range(4):
        sel = [i for i, f in enumerate(fmts) if f == fmt]
        buf, desc = images.pack_images([imgs[i] for i in sel], fmt)
        # a leading gap: the first image does not start at offset 0 either, and the rows keep their padding
        gap = 48
        buf = np.concatenate([np.full(gap, 255, np.uint8), buf])
        desc["offset"] += gap
        assert any(desc["row_stride"] > desc["width"] * FMT_CH[fmt])
        b = Batch(torch_cuda, images, None, fmt, out, desc=desc, buf=buf)
        b.prepare(images)
        torch_cuda.cuda.synchronize()
        assert (b.d_status.cpu().numpy() == 0).all()
        got = b.d_frames.cpu().numpy()
        for j, i in enumerate(sel):
            want = expect_frame(ptq, imgs[i], fmt, out)
            assert np.array_equal(got[j], want), (imgs[i].shape, fmt, out)
            frames[i] = got[j]
    if out == 160:       # the 160 frames feed the network's 160x160 path: heads equal the oracle's at 160x160
        x = np.stack([frames[i] for i in range(8)])
        d_in = torch_cuda.from_numpy(x).cuda()
        d_out = torch_cuda.zeros((8, 20, 20, 18), dtype=torch_cuda.int8, device="cuda")
        network.run_device_hw(160, 160, d_in.data_ptr(), d_out.data_ptr(), 8)
        torch_cuda.cuda.synchronize()
        assert np.array_equal(d_out.cpu().numpy(), oracle.run(x))


def _check_against_oracle(yf, oracle, ptq, b, imgs, variant=0):
    frames_ref = np.stack([expect_frame(ptq, im, 0, 56) for im in imgs])
    assert np.array_equal(b.d_frames.cpu().numpy(), frames_ref)
    heads_ref = oracle.run(frames_ref, variant=variant)
    assert np.array_equal(b.d_heads.cpu().numpy(), heads_ref)
    recs, counts = b.records(yf)
    for i, im in enumerate(imgs):
        h, w = im.shape[:2]
        want = oracle.decode_py(heads_ref[i], i, w_scale=w / 56., h_scale=h / 56.)
        assert recs[i] == want, (i, im.shape)
        assert counts[i] == len(want)
    return recs


def test_real_content_to_boxes(yf, network, oracle, torch_cuda, images, ptq):
    imgs = real_images(ptq)
    b = Batch(torch_cuda, images, imgs, "bgr")
    b.run_decode(images, network)
    torch_cuda.cuda.synchronize()
    assert (b.d_status.cpu().numpy() == 0).all()
    recs = _check_against_oracle(yf, oracle, ptq, b, imgs)
    assert any(len(r) > 0 and (im.shape[0] != 56 or im.shape[1] != 56) for r, im in zip(recs, imgs)), "no image has boxes"
    # the same records from the heads alone (per-image scales, no status), and from detect()
    b.d_dets.zero_()
    images.decode_ragged_device(b.d_heads.data_ptr(), b.d_desc.data_ptr(), b.n, b.d_dets.data_ptr(), b.d_counts.data_ptr(), b.cap)
    assert b.records(yf)[0] == recs
    boxes = images.detect(network, imgs, "bgr")
    assert [bx.tolist() for bx in boxes] == [[[r[6], r[7], r[8], r[9]] for r in rr] for rr in recs]


def test_rounding_is_honoured(yf, network, oracle, torch_cuda, images, ptq):
    imgs = real_images(ptq)
    b = Batch(torch_cuda, images, imgs, "bgr")
    network.set_requant_rounding(yf.YF_ROUND_TIES_UP)
    try:
        b.run_decode(images, network)
        torch_cuda.cuda.synchronize()
        _check_against_oracle(yf, oracle, ptq, b, imgs, variant=1)
    finally:
        network.set_requant_rounding(yf.YF_ROUND_TFLITE_REF)


def test_uniform_equals_ragged(yf, network, torch_cuda, images, ptq):
    """4096 images of 410 x 362 (BGR) in one tensor: the uniform call, the ragged call on the same images and yf_network_run_decode_device with
    the scalar scales give the same records"""
    torch = torch_cuda
    n, H, W = 4096, 362, 410
    real = real_images(ptq)[0]
    assert real.shape == (H, W, 3)
    g = torch.Generator(device="cuda").manual_seed(5)
    base = torch.from_numpy(real).cuda()
    noise = torch.randint(-24, 25, (64, H, W, 3), device="cuda", generator=g, dtype=torch.int16)
    variants = (base.to(torch.int16)[None] + noise).clamp(0, 255).to(torch.uint8)                # 64 distinct faces-with-noise
    idx = torch.arange(n, device="cuda")
    px = variants[idx % 64].contiguous()
    fs, rs = H * W * 3, W * 3
    cap = 147
    mk = lambda: (torch.empty((n, 56, 56, 3), dtype=torch.int8, device="cuda"), torch.empty((n, 7, 7, 18), dtype=torch.int8, device="cuda"),
                  torch.zeros((n, cap, 28), dtype=torch.uint8, device="cuda"), torch.full((n,), -1, dtype=torch.int32, device="cuda"))
    f_u, h_u, d_u, c_u = mk()
    images.run_decode_device(network, px.data_ptr(), px.numel(), "bgr", H, W, rs, fs, n, f_u.data_ptr(), h_u.data_ptr(), d_u.data_ptr(),
                             c_u.data_ptr(), cap)
    desc = np.zeros(n, images.IMAGE_DTYPE)
    desc["offset"], desc["height"], desc["width"], desc["row_stride"] = np.arange(n) * fs, H, W, rs
    d_desc = torch.from_numpy(desc.view(np.uint8)).cuda()
    f_r, h_r, d_r, c_r = mk()
    st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    images.run_decode_ragged_device(network, px.data_ptr(), px.numel(), "bgr", d_desc.data_ptr(), n, f_r.data_ptr(), h_r.data_ptr(),
                                    d_r.data_ptr(), c_r.data_ptr(), cap, st.data_ptr())
    f_s, h_s, d_s, c_s = mk()
    network.run_decode_device(f_u.data_ptr(), h_s.data_ptr(), n, d_s.data_ptr(), c_s.data_ptr(), cap, w_scale=float(np.float32(W / 56.)),
                              h_scale=float(np.float32(H / 56.)))
    torch.cuda.synchronize()
    assert torch.equal(f_u, f_r) and torch.equal(h_u, h_r) and torch.equal(h_u, h_s)
    assert (st == 0).all().item()
    for c in (c_r, c_s):
        assert torch.equal(c_u, c)
    assert int(c_u.sum().item()) > 0
    dt = yf.DET_DTYPE
    cu = c_u.cpu().numpy()
    du, dr, ds = (d.cpu().numpy().view(dt).reshape(n, cap) for d in (d_u, d_r, d_s))
    for i in range(n):
        k = min(int(cu[i]), cap)
        assert du[i, :k].tobytes() == dr[i, :k].tobytes() == ds[i, :k].tobytes(), i
    # and a sample of frames against the restatement
    host = px[:3].cpu().numpy()
    for i in range(3):
        assert np.array_equal(f_u[i].cpu().numpy(), expect_frame(ptq, host[i], 0, 56))


def test_invalid_descriptors_are_flagged_and_never_read(yf, network, torch_cuda, images, ptq):
    rng = np.random.default_rng(3)
    imgs = [rng.integers(0, 256, (60 + 7 * i, 50 + 5 * i, 3), dtype=np.uint8) for i in range(7)]
    buf, desc = images.pack_images(imgs, "bgr")
    desc["height"][1] = 0                                      # zero height
    desc["row_stride"][3] = desc["width"][3] * 3 - 1           # stride below a row
    desc["offset"][5] = buf.nbytes + 16                        # past the end
    b = Batch(torch_cuda, images, None, "bgr", desc=desc, buf=buf)
    b.run_decode(images, network)
    torch_cuda.cuda.synchronize()
    assert b.d_status.cpu().numpy().tolist() == [0, 1, 0, 1, 0, 1, 0]
    frames = b.d_frames.cpu().numpy()
    counts = b.d_counts.cpu().numpy()
    for i in range(7):
        if i in (1, 3, 5):
            assert (frames[i] == -128).all() and counts[i] == 0
        else:
            assert np.array_equal(frames[i], expect_frame(ptq, imgs[i], 0, 56))
    # the last image ends exactly at the end of the buffer: valid; one byte less is not
    last = len(imgs) - 1
    for shrink, st in ((0, 0), (1, 1)):
        b2 = Batch(torch_cuda, images, None, "bgr", desc=desc[last:last + 1].copy(), buf=buf[:buf.nbytes - shrink].copy())
        b2.prepare(images)
        torch_cuda.cuda.synchronize()
        assert b2.d_status.cpu().numpy().tolist() == [st]


def test_counts_zero_one_and_100000(yf, network, torch_cuda, images):
    torch = torch_cuda
    # n = 0: nothing launched, nothing written
    b0 = Batch(torch, images, [], "bgr")
    assert b0.n == 0
    b0.run_decode(images, network)
    b0.prepare(images)
    torch.cuda.synchronize()
    assert (b0.d_frames == 77).all().item() and (b0.d_counts == -7).all().item()
    # n = 1
    one = [np.full((9, 13, 3), 200, np.uint8)]
    b1 = Batch(torch, images, one, "rgb")
    b1.run_decode(images, network)
    torch.cuda.synchronize()
    assert (b1.d_frames.cpu().numpy() == 72).all() and b1.d_status.cpu().numpy().tolist() == [0] and b1.d_counts.cpu().numpy()[0] >= 0
    # 100 000 1 x 1 images: every frame is its pixel, RGB order
    n = 100000
    rng = np.random.default_rng(9)
    px = rng.integers(0, 256, (n, 3), dtype=np.uint8)
    desc = np.zeros(n, images.IMAGE_DTYPE)
    desc["offset"], desc["height"], desc["width"], desc["row_stride"] = np.arange(n) * 3, 1, 1, 3
    b = Batch(torch, images, None, "bgr", desc=desc, buf=px.reshape(-1))
    b.run_decode(images, network)
    torch.cuda.synchronize()
    frames = b.d_frames.cpu().numpy().reshape(n, -1, 3)
    want = (px[:, ::-1].astype(np.int16) - 128).astype(np.int8)
    assert (frames == want[:, None, :]).all()
    assert (b.d_status.cpu().numpy() == 0).all()
    # the records: the network's decode of the same heads with the scalar scale of a 1 x 1 image
    d_dets = torch.zeros_like(b.d_dets)
    d_counts = torch.zeros_like(b.d_counts)
    s = float(np.float32(1 / 56.))
    network.decode_device(b.d_heads.data_ptr(), n, d_dets.data_ptr(), d_counts.data_ptr(), b.cap, w_scale=s, h_scale=s)
    torch.cuda.synchronize()
    assert torch.equal(d_counts, b.d_counts)
    cnt = d_counts.cpu().numpy()
    a, c = d_dets.cpu().numpy().view(yf.DET_DTYPE).reshape(n, -1), b.d_dets.cpu().numpy().view(yf.DET_DTYPE).reshape(n, -1)
    for i in np.nonzero(cnt)[0][:2000]:
        k = min(int(cnt[i]), b.cap)
        assert a[i, :k].tobytes() == c[i, :k].tobytes()
