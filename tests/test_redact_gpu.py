"""The redaction on the MI355X (yf_images_redact_records_device, yf_images_redact_records_yuv_device): the device against the host build
of csrc/yf_images_redact.h byte for byte over the whole pixel buffer of the designed batches of tests/redact_support.py -- padded rows, odd
gaps, a filler byte wherever no pixel lies -- in every format, both modes, with d_first and d_status; once per format against the
plain-Python statement, so that this file stands alone; permuted records and a second call; the frame of 1200 records; invalid descriptors
between valid ones; the host's argument checks; stream capture; and `detect_redacted` end to end on the real images.  Every comparison is
exact."""
import numpy as np
import pytest

import crops_support as cs
import redact_support as rs
from images_support import images_after_network, last_error, ptq, real_images, torch_cuda      # noqa: F401 (fixtures; `images` is images_after_network)
from images_yuv_support import real_surfaces

pytestmark = pytest.mark.gpu


class Dev:
    """a batch on the device: descriptors, records and counts uploaded once; the pixels anew for every call, which writes them"""

    def __init__(self, torch, buf, desc, dets, counts, fmt, cap):
        self.torch, self.n, self.cap, self.fmt, self.nbytes, self.buf = torch, dets.shape[0], cap, fmt, buf.nbytes, buf
        self.d_desc = torch.from_numpy(np.ascontiguousarray(desc).view(np.uint8).copy()).cuda()
        self.d_dets = torch.from_numpy(np.ascontiguousarray(dets).view(np.uint8).reshape(self.n, cap, 28).copy()).cuda()
        self.d_counts = torch.from_numpy(np.ascontiguousarray(counts).copy()).cuda()

    def pixels(self, buf=None):
        return self.torch.from_numpy((self.buf if buf is None else buf).copy()).cuda()

    def outputs(self):
        """d_first, d_status that show what was written"""
        return (self.torch.full((self.n + 1,), rs.SENTINEL32, dtype=self.torch.int32, device="cuda"),
                self.torch.full((self.n,), rs.SENTINEL32, dtype=self.torch.int32, device="cuda"))


def launch(images, b, d_px, out, mode, block, margin, square, stream=None):
    redact = images.redact_records_yuv_device if b.fmt in (4, 5) else images.redact_records_device
    redact(d_px.data_ptr(), b.nbytes, b.fmt, b.d_desc.data_ptr(), b.d_dets.data_ptr(), b.d_counts.data_ptr(), b.n, b.cap, out[0].data_ptr(),
           out[1].data_ptr(), mode=mode, block=block, colour=rs.FILL, margin_permille=margin, square=square, stream=stream)


def device_redact(torch, images, b, mode, block, margin, square, buf=None):
    """-> (buffer, first, status) as the device left them"""
    d_px, out = b.pixels(buf), b.outputs()
    launch(images, b, d_px, out, mode, block, margin, square)
    torch.cuda.synchronize()
    return d_px.cpu().numpy(), out[0].cpu().numpy(), out[1].cpu().numpy()


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_device_equals_the_host_build_on_the_designed_batch(torch_cuda, images, fmt):
    dets, counts = rs.designed()
    buf, desc, pictures = rs.packed_batch(fmt)
    b = Dev(torch_cuda, buf, desc, dets, counts, fmt, rs.CAP)
    for mode, block, margin, square in rs.cases():
        where = (fmt, mode, block, margin, square)
        rc, want, first, status = rs.host_redact(buf, fmt, desc, dets, counts, rs.CAP, mode, block, margin, square)
        assert rc == b.n and not np.array_equal(want, buf), where
        got, got_first, got_status = device_redact(torch_cuda, images, b, mode, block, margin, square)
        assert np.array_equal(got_first, first) and np.array_equal(got_status, status) and not status.any(), where
        assert np.array_equal(got, want), where
    # ... and the host build is the restatement (tests/test_redact_host.py); once per mode here, so that this file stands alone
    for mode, block, margin, square in ((rs.MOSAIC, 8, 250, True), (rs.FILLED, 0, 0, False)):
        got = device_redact(torch_cuda, images, b, mode, block, margin, square)[0]
        assert np.array_equal(got, rs.expected_packed(pictures, fmt, dets, counts, rs.CAP, mode, block, margin, square)), (fmt, mode)


@pytest.mark.parametrize("fmt", [4, 5])
def test_device_equals_the_host_build_on_surfaces(torch_cuda, images, fmt):
    buf, desc, surfaces, dets, counts = rs.yuv_batch()
    b = Dev(torch_cuda, buf, desc, dets, counts, fmt, rs.YUV_CAP)
    for mode, block, margin, square in rs.cases():
        where = (fmt, mode, block, margin, square)
        rc, want, first, status = rs.host_redact(buf, fmt, desc, dets, counts, rs.YUV_CAP, mode, block, margin, square)
        assert rc == b.n and not np.array_equal(want, buf), where
        got, got_first, got_status = device_redact(torch_cuda, images, b, mode, block, margin, square)
        assert np.array_equal(got_first, first) and np.array_equal(got_status, status) and not status.any(), where
        assert np.array_equal(got, want), where
    for mode, block, margin, square in ((rs.MOSAIC, 4, 0, False), (rs.FILLED, 0, 250, True)):
        got = device_redact(torch_cuda, images, b, mode, block, margin, square)[0]
        assert np.array_equal(got, rs.expected_yuv(surfaces, fmt, dets, counts, rs.YUV_CAP, mode, block, margin, square)), (fmt, mode)


def _permuted(dets, counts, cap, seed):
    rng = np.random.default_rng(seed)
    out = dets.copy()
    for f in range(dets.shape[0]):
        m = cs.clamp(counts[f], cap)
        out[f, :m] = dets[f, rng.permutation(m)]
    return out


def test_permuted_records_and_a_second_call(torch_cuda, images):
    dets, counts = rs.designed()
    buf, desc, _ = rs.packed_batch(3)
    ybuf, ydesc, _, ydets, ycounts = rs.yuv_batch()
    for fmt, (pb, pd, pdets, pcounts, cap) in ((3, (buf, desc, dets, counts, rs.CAP)), (4, (ybuf, ydesc, ydets, ycounts, rs.YUV_CAP))):
        b = Dev(torch_cuda, pb, pd, pdets, pcounts, fmt, cap)
        shuffled = _permuted(pdets, pcounts, cap, 5600 + fmt)
        assert shuffled.tobytes() != pdets.tobytes()
        bs = Dev(torch_cuda, pb, pd, shuffled, pcounts, fmt, cap)
        for block, margin, square in ((4, 0, False), (8, 250, True), (64, 0, False)):
            where = (fmt, block, margin, square)
            once = device_redact(torch_cuda, images, b, rs.MOSAIC, block, margin, square)[0]
            assert not np.array_equal(once, pb), where
            assert np.array_equal(device_redact(torch_cuda, images, bs, rs.MOSAIC, block, margin, square)[0], once), where
            assert np.array_equal(device_redact(torch_cuda, images, b, rs.MOSAIC, block, margin, square, buf=once)[0], once), where


def test_the_capacity_frame(torch_cuda, images):
    """1200 records on one 37 x 53 picture, cap 1200: the last slot's list of earlier owners holds 1199 entries"""
    dets, counts = rs.capacity_batch()
    pictures = [cs.in_format(rs.picture(0), 0)]
    buf, desc = rs.lay_out_packed(pictures)
    b = Dev(torch_cuda, buf, desc, dets, counts, 0, 1200)
    for mode, block in ((rs.MOSAIC, 4), (rs.MOSAIC, 8), (rs.FILLED, 0)):
        rc, want, first, status = rs.host_redact(buf, 0, desc, dets, counts, 1200, mode, block, 0, False)
        got, got_first, got_status = device_redact(torch_cuda, images, b, mode, block, 0, False)
        assert rc == 1 and got_first.tolist() == [0, 1200] and got_status.tolist() == [0]
        assert np.array_equal(got, want) and not np.array_equal(got, buf), (mode, block)
    assert np.array_equal(got, rs.expected_packed(pictures, 0, dets, counts, 1200, rs.FILLED, 0, 0, False))


def test_invalid_descriptors_between_valid_ones(torch_cuda, images):
    """the buffer ends with its last picture (no tail): a descriptor one byte too far would touch bytes past the allocation if it were used"""
    dets, counts = rs.designed()
    buf, desc, pictures = rs.packed_batch(0)
    desc = desc.copy()
    desc["row_stride"][1] = int(desc["width"][1]) * 3 - 1                      # a stride below the row
    desc["offset"][3] = buf.nbytes + 1 - ((362 - 1) * int(desc["row_stride"][3]) + 410 * 3)          # ends one byte past the buffer
    desc["height"][5] = 0
    b = Dev(torch_cuda, buf, desc, dets, counts, 0, rs.CAP)
    for mode, block in ((rs.MOSAIC, 8), (rs.FILLED, 0)):
        got, first, status = device_redact(torch_cuda, images, b, mode, block, 250, False)
        assert status.tolist() == [0, 1, 0, 1, 0, 1, 0] and np.array_equal(first, rs.first_of(counts, rs.CAP))
        assert np.array_equal(got, rs.expected_packed(pictures, 0, dets, counts, rs.CAP, mode, block, 250, False, invalid={1, 3, 5}))
        assert np.array_equal(got, rs.host_redact(buf, 0, desc, dets, counts, rs.CAP, mode, block, 250, False)[1])
    # surfaces: 1 (odd height) and 2 (the UV plane ends one byte past the buffer) are invalid
    ybuf, ydesc, surfaces, ydets, ycounts = rs.yuv_batch()
    ydesc = ydesc.copy()
    ydesc["height"][1] += 1
    d2 = ydesc[2]
    ydesc["offset_uv"][2] = ybuf.nbytes + 1 - ((int(d2["height"]) // 2 - 1) * int(d2["stride_uv"]) + int(d2["width"]))
    b = Dev(torch_cuda, ybuf, ydesc, ydets, ycounts, 5, rs.YUV_CAP)
    for mode, block in ((rs.MOSAIC, 4), (rs.FILLED, 0)):
        got, first, status = device_redact(torch_cuda, images, b, mode, block, 0, True)
        assert status.tolist() == [0, 1, 1, 0]
        assert np.array_equal(got, rs.expected_yuv(surfaces, 5, ydets, ycounts, rs.YUV_CAP, mode, block, 0, True, invalid={1, 2}))


def test_host_argument_checks_launch_nothing(torch_cuda, images):
    torch = torch_cuda
    lib = images.load()
    dets, counts = rs.designed()
    buf, desc, _ = rs.packed_batch(0)
    b = Dev(torch, buf, desc, dets, counts, 0, rs.CAP)
    ybuf, ydesc, _, ydets, ycounts = rs.yuv_batch()
    yb = Dev(torch, ybuf, ydesc, ydets, ycounts, 4, rs.YUV_CAP)
    px = {id(b): b.pixels(), id(yb): yb.pixels()}
    d_first, d_status = b.outputs()

    def untouched():
        torch.cuda.synchronize()
        return ((d_first == rs.SENTINEL32).all().item() and (d_status == rs.SENTINEL32).all().item()
                and np.array_equal(px[id(b)].cpu().numpy(), buf) and np.array_equal(px[id(yb)].cpu().numpy(), ybuf))

    def call(entry="redact_records_device", batch=b, fmt=0, n=None, cap=None, mode=0, block=8, colour=0, margin=0, flags=0, first=None):
        fn = getattr(lib, "yf_images_" + entry)
        return fn(px[id(batch)].data_ptr(), batch.nbytes, fmt, batch.d_desc.data_ptr(), batch.d_dets.data_ptr(), batch.d_counts.data_ptr(),
                  batch.n if n is None else n, batch.cap if cap is None else cap, mode, block, colour, margin, flags,
                  d_first.data_ptr() if first is None else first, d_status.data_ptr(), None)

    yuv = dict(entry="redact_records_yuv_device", batch=yb, fmt=4)
    for kw, text in ((dict(block=0), "block must be 4"), (dict(block=12), "block must be 4"), (dict(block=128), "block must be 4"),
                     (dict(mode=1, block=8), "block must be 0"), (dict(mode=1, block=0, colour=0x01000000), "top byte"),
                     (dict(mode=2), "mode"), (dict(margin=1001), "margin_permille"), (dict(margin=-1), "margin_permille"),
                     (dict(flags=2), "flags"), (dict(cap=0), "cap"), (dict(cap=1201), "cap"), (dict(n=-1), "n must"),
                     (dict(n=2 ** 31 // 1200 + 1, cap=1200), "n * cap"),
                     (dict(fmt=4), "yf_images_redact_records_yuv_device"), (dict(fmt=5), "yf_images_redact_records_yuv_device"),
                     (dict(yuv, fmt=0), "yf_images_redact_records_device"), (dict(yuv, fmt=3), "yf_images_redact_records_device"),
                     (dict(fmt=6), "format"), (dict(yuv, fmt=7), "format"), (dict(first=d_first.data_ptr() + 2), "4-byte aligned"),
                     (dict(yuv, block=6), "block must be 4"), (dict(yuv, mode=1, block=0, colour=0xFF000000), "top byte"),
                     (dict(yuv, margin=2000), "margin_permille")):
        assert call(**kw) <= 0 and text in last_error(lib), (kw, last_error(lib))
        assert untouched(), kw
    # n = 0: nothing is launched, 0 is returned, after the checks
    assert call(n=0) == 0 and untouched()
    assert call(n=0, block=5) == 0 and "block must be 4" in last_error(lib)
    # ... and the same arguments accepted
    assert call() == b.n and call(**yuv) == yb.n
    torch.cuda.synchronize()
    assert d_first[yb.n].item() == int(ycounts.sum()) and not untouched()


def test_redaction_is_capturable(torch_cuda, images):
    """one call captured with the buffers allocated beforehand and replayed once: two kernels in a single chain"""
    torch = torch_cuda
    dets, counts = rs.designed()
    buf, desc, _ = rs.packed_batch(2)
    b = Dev(torch, buf, desc, dets, counts, 2, rs.CAP)
    args = (rs.MOSAIC, 8, 250, True)
    want = device_redact(torch, images, b, *args)                              # an ordinary call first, and the yardstick of the replay
    d_px, out = b.pixels(), b.outputs()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            launch(images, b, d_px, out, *args, stream=s.cuda_stream)
    torch.cuda.synchronize()
    assert (out[0] == rs.SENTINEL32).all().item() and np.array_equal(d_px.cpu().numpy(), buf)            # captured, not run
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(d_px.cpu().numpy(), want[0]) and np.array_equal(out[0].cpu().numpy(), want[1])
    assert np.array_equal(out[1].cpu().numpy(), want[2]) and not np.array_equal(want[0], buf)


# ---- end to end ----
def _regions(ptq, boxes, w, h, permille, square):
    return [ptq.crop_region(box, w, h, permille, square) for box in boxes]


def _set_mask(regions, w, h, block):
    """the pixels of the redacted set: the touched blocks (mosaic) or the regions themselves (block 0)"""
    mask = np.zeros((h, w), bool)
    for x0, y0, rw, rh in (r for r in regions if r is not None):
        if block:
            mask[y0 // block * block:((y0 + rh - 1) // block + 1) * block, x0 // block * block:((x0 + rw - 1) // block + 1) * block] = True
        else:
            mask[y0:y0 + rh, x0:x0 + rw] = True
    return mask


def test_detect_redacted_on_the_real_images(network, torch_cuda, images, ptq):
    bgr = real_images(ptq)
    originals = [img.copy() for img in bgr]
    want = images.detect(network, bgr, iou_threshold=0.4)
    assert sum(w.shape[0] for w in want) >= 1, "detect reports no box: the comparison shows nothing"
    for kw, mode, block, colour, permille, square in ((dict(), "mosaic", 8, None, 0, False),
                                                      (dict(mode="mosaic", block=32, margin=0.25, square=True), "mosaic", 32, None, 250, True),
                                                      (dict(mode="fill", colour=(200, 45, 90), margin=0.1), "fill", 0, (90, 45, 200), 100, False)):
        pictures, boxes = images.detect_redacted(network, bgr, **kw)
        assert len(pictures) == len(bgr) and all(np.array_equal(a, w) and a.dtype == w.dtype for a, w in zip(boxes, want))
        changed = 0
        for i, img in enumerate(bgr):
            assert np.array_equal(img, originals[i])                           # the caller's arrays are not written
            regions = _regions(ptq, boxes[i], img.shape[1], img.shape[0], permille, square)
            assert pictures[i].shape == img.shape and np.array_equal(pictures[i], ptq.redact_u8(img, regions, mode, block, colour)), (kw, i)
            differs = (pictures[i] != img).any(axis=2)
            assert not (differs & ~_set_mask(regions, img.shape[1], img.shape[0], block)).any(), (kw, i)
            changed += int(differs.sum())
        assert changed > 0, kw
    assert images.detect_redacted(network, []) == ([], [])
    # tiles of 160 with the whole picture in front: the boxes are detect_tiled's, the parents are redacted
    photos = bgr[:6]
    tiled = images.detect_tiled(network, photos, 160, stride=120)
    assert sum(t.shape[0] for t in tiled) >= 1
    pictures, boxes = images.detect_redacted(network, photos, block=16, tile=160, stride=120)
    assert all(np.array_equal(a, t) for a, t in zip(boxes, tiled))
    for i, img in enumerate(photos):
        assert np.array_equal(pictures[i], ptq.redact_u8(img, _regions(ptq, boxes[i], img.shape[1], img.shape[0], 0, False), "mosaic", 16, None)), i


def test_detect_redacted_on_surfaces(network, torch_cuda, images, ptq):
    nv12, _, _ = real_surfaces()
    want = images.detect(network, nv12, fmt="nv12", iou_threshold=0.4)
    assert sum(w.shape[0] for w in want) >= 1
    for kw, mode, block, permille in ((dict(block=8), "mosaic", 8, 0), (dict(mode="fill", colour=(200, 45, 90), margin=0.25), "fill", 0, 250)):
        pictures, boxes = images.detect_redacted(network, nv12, fmt="nv12", **kw)
        assert all(np.array_equal(a, w) for a, w in zip(boxes, want))
        changed = 0
        for i, (y, uv) in enumerate(nv12):
            regions = _regions(ptq, boxes[i], y.shape[1], y.shape[0], permille, False)
            ry, ruv = ptq.redact_yuv420sp(y, uv, regions, mode, block, (200, 45, 90))
            assert np.array_equal(pictures[i][0], ry) and np.array_equal(pictures[i][1], ruv), (kw, i)
            differs = pictures[i][0] != y
            assert not (differs & ~_set_mask(regions, y.shape[1], y.shape[0], block)).any(), (kw, i)
            changed += int(differs.sum())
        assert changed > 0, kw
