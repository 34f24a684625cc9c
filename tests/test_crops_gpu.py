"""Face chips on the MI355X (yf_images_crop_records_device, yf_images_crop_records_yuv_device): the device against the host build of
csrc/yf_images_crop.h byte for byte on the designed records of tests/crops_support.py, written into sentinel-filled buffers; the cut at
chips_cap; NV12 / NV21 surfaces against the packed-RGB crop of the restated conversion; invalid descriptors between valid ones; the host's
argument checks; stream capture; and `detect_chips` end to end on the real images.  Every comparison is exact."""
import ctypes

import numpy as np
import pytest

import crops_support as cs
from images_support import images_after_network, last_error, ptq, real_images, torch_cuda      # noqa: F401 (fixtures; `images` is images_after_network)
from images_yuv_support import lay_out, real_surfaces, surface

pytestmark = pytest.mark.gpu

SENTINEL32 = -1515870811                    # 0xA5A5A5A5


class Dev:
    """a batch on the device: pixels, descriptors, records and counts, uploaded once"""

    def __init__(self, torch, buf, desc, dets, counts, fmt, cap):
        self.n, self.cap, self.fmt, self.nbytes = dets.shape[0], cap, fmt, buf.nbytes
        self.d_px = torch.from_numpy(buf).cuda()
        self.d_desc = torch.from_numpy(np.ascontiguousarray(desc).view(np.uint8).copy()).cuda()
        self.d_dets = torch.from_numpy(np.ascontiguousarray(dets).view(np.uint8).reshape(self.n, cap, 28).copy()).cuda()
        self.d_counts = torch.from_numpy(np.ascontiguousarray(counts).copy()).cuda()


def outputs(torch, n, room, out_h, out_w):
    """d_chips, d_info, d_first that show what was written: every byte 0xA5"""
    return (torch.full((max(room, 1), out_h, out_w, 3), 0xA5, dtype=torch.uint8, device="cuda"),
            torch.full((max(room, 1), 28), 0xA5, dtype=torch.uint8, device="cuda"),
            torch.full((n + 1,), SENTINEL32, dtype=torch.int32, device="cuda"))


def launch(images, b, out, out_h, out_w, margin, square, order, chips_cap, stream=None):
    d_chips, d_info, d_first = out
    crop = images.crop_records_yuv_device if b.fmt in (4, 5) else images.crop_records_device
    crop(b.d_px.data_ptr(), b.nbytes, b.fmt, b.d_desc.data_ptr(), b.d_dets.data_ptr(), b.d_counts.data_ptr(), b.n, b.cap, out_h, out_w,
         d_chips.data_ptr(), chips_cap, d_first.data_ptr(), d_info.data_ptr(), order=order, margin_permille=margin, square=square, stream=stream)


def device_crop(torch, images, b, out_h, out_w, margin, square, order, chips_cap):
    """-> (chips, info CHIP, first) as the device left them in sentinel-filled buffers of max(chips_cap, 1) chips"""
    out = outputs(torch, b.n, chips_cap, out_h, out_w)
    launch(images, b, out, out_h, out_w, margin, square, order, chips_cap)
    torch.cuda.synchronize()
    return out[0].cpu().numpy(), out[1].cpu().numpy().view(cs.CHIP).reshape(-1), out[2].cpu().numpy()


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_device_equals_the_host_build_on_the_designed_records(torch_cuda, images, fmt):
    buf, desc, dets, counts, keys = cs.designed_batch(fmt)
    b = Dev(torch_cuda, buf, desc, dets, counts, fmt, cs.CAP)
    total = 67
    for out_h, out_w in cs.OUTS:
        for margin, square in cs.GRID:
            for order in ("rgb", "bgr"):
                where = (fmt, out_h, out_w, margin, square, order)
                rc, chips, info, first = cs.host_crop(buf, fmt, desc, dets, counts, cs.CAP, out_h, out_w, margin, square, order, total + 2)
                assert rc == b.n and first[-1] == total, where
                got, got_info, got_first = device_crop(torch_cuda, images, b, out_h, out_w, margin, square, order, total + 2)
                assert np.array_equal(got_first, first), where
                assert got_info.tobytes() == info.tobytes(), where                # the rows beyond the total: the sentinel on both sides
                assert np.array_equal(got, chips), where
                assert (got[total:] == 0xA5).all() and (got_info[total:].view(np.uint8) == 0xA5).all(), where
    # ... and the host build is the restatement (tests/test_crops_host.py); once here, so that this file stands alone
    want, want_info, want_first = cs.expected(dets, counts, cs.CAP, keys, 32, 48, 250, True, "bgr")
    assert np.array_equal(got[:total], want) and got_info[:total].tobytes() == want_info.tobytes() and np.array_equal(got_first, want_first)


def test_truncation_inside_a_frame(torch_cuda, images):
    buf, desc, dets, counts, keys = cs.designed_batch(1)
    b = Dev(torch_cuda, buf, desc, dets, counts, 1, cs.CAP)
    want, want_info, want_first = cs.expected(dets, counts, cs.CAP, keys, 16, 32, 0, False, "rgb")
    for chips_cap in (20, 1, 0):                                               # 20: seven chips into frame 1
        got, info, first = device_crop(torch_cuda, images, b, 16, 32, 0, False, "rgb", chips_cap)
        assert np.array_equal(first, want_first) and first[-1] == 67, chips_cap           # the true total
        assert np.array_equal(got[:chips_cap], want[:chips_cap]) and info[:chips_cap].tobytes() == want_info[:chips_cap].tobytes()
        if chips_cap == 20:
            assert info["frame"].tolist() == [0] * 13 + [1] * 7
        if chips_cap == 0:
            assert (got == 0xA5).all() and (info.view(np.uint8) == 0xA5).all()
    # one slot of room more than the cut: it keeps its sentinel
    out = outputs(torch_cuda, b.n, 21, 16, 32)
    launch(images, b, out, 16, 32, 0, False, "rgb", 20)
    torch_cuda.cuda.synchronize()
    assert (out[0][20] == 0xA5).all().item() and (out[1][20] == 0xA5).all().item() and np.array_equal(out[0][:20].cpu().numpy(), want[:20])


YUV_SHAPES = [3, 4, 8, 0]                   # images_yuv_support.SHAPES: 6 x 10, 54 x 58, 362 x 410, 2 x 2 (h x w)


def _yuv_batch(fmt):
    """surfaces laid out with odd pitches and UV before Y; per surface the designed boxes and boxes with odd origins and odd sides"""
    surfaces = [surface(k, False) for k in YUV_SHAPES]
    buf, desc = lay_out(surfaces)
    n, cap = len(surfaces), 16
    dets = np.frombuffer(bytes([0xA5]) * (n * cap * 28), cs.DET).reshape(n, cap).copy()
    counts = np.zeros(n, np.int32)
    keys = []
    for i, (y, uv) in enumerate(surfaces):
        h, w = y.shape
        boxes = cs.designed_boxes(w, h) + [(1, 1, w - 2, h - 2), (3, 1, 7, 7), (w - 3, h - 5, w - 1, h - 1)]
        counts[i] = len(boxes)
        for s, box in enumerate(boxes):
            dets[i, s] = (i, 0, 0, 0, 0, 0.9, *box)
        rgb = cs._mod("ptq").yuv420sp_to_rgb_u8(y, uv, fmt == 5)
        keys.append(cs.register(("yuv", YUV_SHAPES[i], fmt), rgb))
    return buf, desc, dets, counts, keys, cap


@pytest.mark.parametrize("fmt", [4, 5])
def test_surfaces_equal_the_packed_crop_of_the_converted_picture(torch_cuda, images, fmt):
    buf, desc, dets, counts, keys, cap = _yuv_batch(fmt)
    b = Dev(torch_cuda, buf, desc, dets, counts, fmt, cap)
    total = int(counts.sum())
    for (out_h, out_w), (margin, square), order in (((16, 16), (0, False), "rgb"), ((112, 112), (250, True), "rgb"), ((32, 48), (0, True), "bgr"),
                                                    ((112, 112), (0, False), "bgr"), ((32, 48), (250, False), "rgb")):
        where = (fmt, out_h, out_w, margin, square, order)
        want, want_info, want_first = cs.expected(dets, counts, cap, keys, out_h, out_w, margin, square, order)
        got, info, first = device_crop(torch_cuda, images, b, out_h, out_w, margin, square, order, total + 1)
        assert np.array_equal(first, want_first), where
        assert info[:total].tobytes() == want_info.tobytes(), where
        assert np.array_equal(got[:total], want), where
        assert (got[total:] == 0xA5).all(), where
        rc, h_chips, h_info, h_first = cs.host_crop(buf, fmt, desc, dets, counts, cap, out_h, out_w, margin, square, order, total + 1)
        assert rc == b.n and np.array_equal(h_chips, got) and h_info.tobytes() == info.tobytes() and np.array_equal(h_first, first), where
    plain = cs.expected(dets, counts, cap, keys, 16, 16, 0, False, "rgb")[1]
    odd = plain[(plain["status"] == 0) & (plain["x0"] % 2 == 1) & (plain["y0"] % 2 == 1)]
    assert odd.size >= 3 and (odd["width"] % 2 == 1).any() and (odd["height"] % 2 == 1).any()       # odd origins and odd sides were cut


def test_invalid_descriptors_between_valid_ones(torch_cuda, images):
    """the buffer ends with its last picture (no tail): a descriptor one byte too far would read past the allocation if it were read"""
    # packed: frames 1, 3 and 5 are invalid
    buf, desc, dets, counts, keys = cs.designed_batch(0)
    desc = desc.copy()
    ext = lambda d: (int(d["height"]) - 1) * int(d["row_stride"]) + int(d["width"]) * 3
    assert int(desc["offset"][6]) + ext(desc[6]) == buf.nbytes                 # tail-less
    desc["row_stride"][1] = int(desc["width"][1]) * 3 - 1                      # a stride below the row
    desc["offset"][3] = buf.nbytes + 1 - ext(desc[3])                          # ends one byte past the buffer
    desc["height"][5] = 0
    bad = {1, 3, 5}
    b = Dev(torch_cuda, buf, desc, dets, counts, 0, cs.CAP)
    want, want_info, want_first = cs.expected(dets, counts, cs.CAP, keys, 32, 48, 250, False, "rgb", invalid=bad)
    got, info, first = device_crop(torch_cuda, images, b, 32, 48, 250, False, "rgb", 67)
    assert np.array_equal(first, want_first) and info.tobytes() == want_info.tobytes() and np.array_equal(got, want)
    for f in range(b.n):
        rows = info[info["frame"] == f]
        assert (rows["status"] == 2).all() if f in bad else (rows["status"] != 2).all(), f
    assert (got[info["status"] == 2] == 0).all() and (info["status"] == 2).sum() == 13 + 13 + cs.CAP
    assert cs.host_crop(buf, 0, desc, dets, counts, cs.CAP, 32, 48, 250, False, "rgb", 67)[1].tobytes() == got.tobytes()
    # surfaces: 1 (odd height) and 2 (the UV plane ends one byte past the buffer) are invalid
    buf, desc, dets, counts, keys, cap = _yuv_batch(4)
    desc = desc.copy()
    desc["height"][1] += 1
    d2 = desc[2]
    desc["offset_uv"][2] = buf.nbytes + 1 - ((int(d2["height"]) // 2 - 1) * int(d2["stride_uv"]) + int(d2["width"]))
    bad = {1, 2}
    b = Dev(torch_cuda, buf, desc, dets, counts, 4, cap)
    total = int(counts.sum())
    want, want_info, want_first = cs.expected(dets, counts, cap, keys, 16, 16, 0, True, "bgr", invalid=bad)
    got, info, first = device_crop(torch_cuda, images, b, 16, 16, 0, True, "bgr", total)
    assert np.array_equal(first, want_first) and info.tobytes() == want_info.tobytes() and np.array_equal(got, want)
    assert (info["status"] == 2).sum() == 2 * 16 and (got[info["status"] == 2] == 0).all()


def test_host_argument_checks_launch_nothing(torch_cuda, images):
    torch = torch_cuda
    lib = images.load()
    buf, desc, dets, counts, _ = cs.designed_batch(0)
    b = Dev(torch, buf, desc, dets, counts, 0, cs.CAP)
    ybuf, ydesc, ydets, ycounts, _, ycap = _yuv_batch(4)
    yb = Dev(torch, ybuf, ydesc, ydets, ycounts, 4, ycap)
    d_chips, d_info, d_first = outputs(torch, b.n, 70, 16, 16)
    untouched = lambda: (torch.cuda.synchronize(), (d_chips == 0xA5).all().item() and (d_info == 0xA5).all().item()
                         and (d_first == SENTINEL32).all().item())[1]

    def call(entry="crop_records_device", batch=b, fmt=0, n=None, cap=None, out_h=16, out_w=16, out_format=1, margin=0, flags=0, chips=None,
             chips_cap=70):
        fn = getattr(lib, "yf_images_" + entry)
        return fn(batch.d_px.data_ptr(), batch.nbytes, fmt, batch.d_desc.data_ptr(), batch.d_dets.data_ptr(), batch.d_counts.data_ptr(),
                  batch.n if n is None else n, batch.cap if cap is None else cap, out_h, out_w, out_format, margin, flags,
                  d_chips.data_ptr() if chips is None else chips, chips_cap, d_first.data_ptr(), d_info.data_ptr(), None)

    yuv = dict(entry="crop_records_yuv_device", batch=yb, fmt=4)
    for kw, text in ((dict(out_h=24), "multiples of 16"), (dict(out_w=272), "multiples of 16"), (dict(out_h=0), "multiples of 16"),
                     (dict(fmt=4), "yf_images_crop_records_yuv_device"), (dict(fmt=5), "yf_images_crop_records_yuv_device"),
                     (dict(yuv, fmt=0), "yf_images_crop_records_device"), (dict(yuv, fmt=3), "yf_images_crop_records_device"),
                     (dict(fmt=6), "format"), (dict(yuv, fmt=7), "format"),
                     (dict(margin=1001), "margin_permille"), (dict(margin=-1), "margin_permille"),
                     (dict(chips=d_chips.data_ptr() + 4), "16-byte aligned"), (dict(chips_cap=-1), "chips_cap"),
                     (dict(out_format=2), "out_format"), (dict(flags=2), "flags"), (dict(cap=0), "cap"), (dict(cap=1201), "cap"),
                     (dict(n=-1), "n must"), (dict(yuv, out_h=260), "multiples of 16"), (dict(yuv, margin=2000), "margin_permille")):
        assert call(**kw) <= 0 and text in last_error(lib), (kw, last_error(lib))
        assert untouched(), kw
    # n = 0: nothing is launched, 0 is returned, after the checks
    assert call(n=0) == 0 and untouched()
    assert call(n=0, out_h=17) == 0 and "multiples of 16" in last_error(lib)
    # ... and the same arguments accepted
    assert call() == b.n and call(**yuv, chips_cap=70) == yb.n
    torch.cuda.synchronize()
    assert d_first[yb.n].item() == int(ycounts.sum())


def test_crop_is_capturable(torch_cuda, images):
    """one call captured with the buffers allocated beforehand and replayed once; the process keeps its default queue count"""
    torch = torch_cuda
    buf, desc, dets, counts, keys = cs.designed_batch(2)
    b = Dev(torch, buf, desc, dets, counts, 2, cs.CAP)
    args = (112, 112, 250, True, "rgb", 67)
    want = device_crop(torch, images, b, *args)                                # an ordinary call first, and the yardstick of the replay
    out = outputs(torch, b.n, 67, 112, 112)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            launch(images, b, out, *args, stream=s.cuda_stream)
    torch.cuda.synchronize()
    assert (out[2] == SENTINEL32).all().item() and (out[0] == 0xA5).all().item()          # captured, not run
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out[0].cpu().numpy(), want[0]) and out[1].cpu().numpy().tobytes() == want[1].tobytes()
    assert np.array_equal(out[2].cpu().numpy(), want[2])
    ref, ref_info, ref_first = cs.expected(dets, counts, cs.CAP, keys, 112, 112, 250, True, "rgb")
    assert np.array_equal(want[0], ref) and want[1].tobytes() == ref_info.tobytes() and np.array_equal(want[2], ref_first)


# ---- end to end ----
def _check_chips(ptq, pictures_rgb, boxes, chips, info, out_h, out_w, permille, square, order):
    for i, rgb in enumerate(pictures_rgb):
        assert chips[i].shape == (boxes[i].shape[0], out_h, out_w, 3) and info[i].shape[0] == boxes[i].shape[0], i
        for s, box in enumerate(boxes[i]):
            want = ptq.crop_resize_u8(rgb, box, out_w, out_h, permille, square)
            assert np.array_equal(chips[i][s], want if order == "rgb" else want[..., ::-1]), (i, s, box.tolist())
            region = ptq.crop_region(box, rgb.shape[1], rgb.shape[0], permille, square)
            row = info[i][s]
            assert (row["frame"], row["slot"]) == (i, s)
            assert tuple(int(row[k]) for k in ("x0", "y0", "width", "height", "status")) == ((0, 0, 0, 0, 1) if region is None else region + (0,))


def test_detect_chips_on_the_real_images(network, torch_cuda, images, ptq):
    """The 27 real images: on the CPU the oracle (oracle/oracle.py on the restated 56x56 frames, decode_py with each picture's scales) finds
    39 records in them (tests/test_images_yuv_gpu.py states the same count), so the boxes asserted below exist."""
    bgr = real_images(ptq)
    rgb = [img[..., ::-1] for img in bgr]
    want = images.detect(network, bgr, iou_threshold=0.4)
    assert sum(w.shape[0] for w in want) >= 1, "detect reports no box: the comparison shows nothing"
    boxes, chips, info = images.detect_chips(network, bgr)
    assert len(boxes) == len(want) and all(np.array_equal(a, w) and a.dtype == w.dtype for a, w in zip(boxes, want))
    _check_chips(ptq, rgb, boxes, chips, info, 112, 112, 0, False, "rgb")
    boxes, chips, info = images.detect_chips(network, bgr, out=(32, 48), margin=0.25, square=True, order="bgr", chips_cap=200)
    assert all(np.array_equal(a, w) for a, w in zip(boxes, want))
    _check_chips(ptq, rgb, boxes, chips, info, 32, 48, 250, True, "bgr")
    with pytest.raises(images.ImagesError, match="chips_cap holds 1"):
        images.detect_chips(network, bgr, out=16, chips_cap=1)
    assert images.detect_chips(network, []) == ([], [], [])


def test_detect_chips_on_surfaces_and_on_tiles(network, torch_cuda, images, ptq):
    nv12, _, bgr = real_surfaces()
    want = images.detect(network, nv12, fmt="nv12", iou_threshold=0.4)
    assert sum(w.shape[0] for w in want) >= 1
    boxes, chips, info = images.detect_chips(network, nv12, fmt="nv12", out=(48, 32), margin=0.1)
    assert all(np.array_equal(a, w) for a, w in zip(boxes, want))
    _check_chips(ptq, [img[..., ::-1] for img in bgr], boxes, chips, info, 48, 32, 100, False, "rgb")
    # tiles of 160 with the whole picture in front: the boxes are detect_tiled's, the chips are cut from the parents
    photos = real_images(ptq)[:6]
    tiled = images.detect_tiled(network, photos, 160, stride=120)
    assert sum(t.shape[0] for t in tiled) >= 1
    boxes, chips, info = images.detect_chips(network, photos, tile=160, stride=120, out=64, square=True)
    assert all(np.array_equal(a, t) for a, t in zip(boxes, tiled))
    _check_chips(ptq, [img[..., ::-1] for img in photos], boxes, chips, info, 64, 64, 0, True, "rgb")
