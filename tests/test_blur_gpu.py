"""The blur on the MI355X (yf_images_blur_records_device, yf_images_blur_records_yuv_device): the device against the host build of
csrc/yf_images_blur.h byte for byte over the whole pixel buffer of the designed batches of tests/redact_support.py -- padded rows, odd gaps,
a filler byte wherever no pixel lies -- in every format at grids 1, 8 and 16, with d_first and d_status; once per format against the
plain-numpy statement, so that this file stands alone; the strips of every small width as one ragged batch; a workspace too small; invalid
descriptors between valid ones; the frame of 1200 records; a surface whose Y sum passes 2^32; the host's argument checks; stream capture;
`detect_blurred` end to end on the real images; and the tracker's records fed to the blur.  Every comparison is exact."""
import numpy as np
import pytest

import blur_support as bs
import crops_support as cs
import redact_support as rs
import track_support as ts
from images_support import images_after_network, last_error, ptq, real_images, torch_cuda      # noqa: F401 (fixtures; `images` is images_after_network)
from images_yuv_support import real_surfaces

pytestmark = pytest.mark.gpu

CASES = [(g, m, s) for g in (1, 8, 16) for m, s in ((0, False), (250, True))]


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

    def work(self, images, records_cap, grid):
        """a workspace of exactly its size (torch's allocations are aligned far beyond 16 bytes)"""
        room = images.blur_workspace(records_cap, grid)
        assert room == bs.workspace(records_cap, grid)
        return self.torch.full((max(room, 1),), 0xA5, dtype=self.torch.uint8, device="cuda"), room


def launch(images, b, d_px, out, work, records_cap, grid, margin, square, stream=None):
    blur = images.blur_records_yuv_device if b.fmt in (4, 5) else images.blur_records_device
    blur(d_px.data_ptr(), b.nbytes, b.fmt, b.d_desc.data_ptr(), b.d_dets.data_ptr(), b.d_counts.data_ptr(), b.n, b.cap, work[0].data_ptr(),
         work[1], records_cap, out[0].data_ptr(), out[1].data_ptr(), grid=grid, colour=bs.FILL, margin_permille=margin, square=square,
         stream=stream)


def device_blur(torch, images, b, grid, margin, square, records_cap=None, buf=None):
    """-> (buffer, first, status) as the device left them"""
    records_cap = b.n * b.cap if records_cap is None else records_cap
    d_px, out, work = b.pixels(buf), b.outputs(), b.work(images, records_cap, grid)
    launch(images, b, d_px, out, work, records_cap, grid, margin, square)
    torch.cuda.synchronize()
    return d_px.cpu().numpy(), out[0].cpu().numpy(), out[1].cpu().numpy()


@pytest.mark.parametrize("fmt", [0, 1, 2, 3, 4, 5])
def test_device_equals_the_host_build_on_the_designed_batch(torch_cuda, images, fmt):
    if fmt in (4, 5):
        buf, desc, pictures, dets, counts = rs.yuv_batch()
        cap, expected = rs.YUV_CAP, bs.expected_yuv
    else:
        dets, counts = rs.designed()
        buf, desc, pictures = rs.packed_batch(fmt)
        cap, expected = rs.CAP, bs.expected_packed
    b = Dev(torch_cuda, buf, desc, dets, counts, fmt, cap)
    for grid, margin, square in CASES:
        where = (fmt, grid, margin, square)
        rc, want, first, status = bs.host_blur(buf, fmt, desc, dets, counts, cap, grid, margin, square)
        assert rc == b.n and not np.array_equal(want, buf), where
        got, got_first, got_status = device_blur(torch_cuda, images, b, grid, margin, square)
        assert np.array_equal(got_first, first) and np.array_equal(got_status, status) and not status.any(), where
        assert np.array_equal(got, want), where
    # ... and the host build is the restatement (tests/test_blur_host.py); once here, so that this file stands alone
    got = device_blur(torch_cuda, images, b, 8, 250, True)[0]
    assert np.array_equal(got, expected(pictures, fmt, dets, counts, cap, 8, 250, True)), fmt


@pytest.mark.parametrize("grid", bs.GRIDS)
def test_the_strips_as_one_ragged_batch(torch_cuda, images, grid):
    buf, desc, _, dets, counts = bs.strips()
    b = Dev(torch_cuda, buf, desc, dets, counts, 1, 1)
    rc, want, first, status = bs.host_blur(buf, 1, desc, dets, counts, 1, grid, 0, False)
    got, got_first, got_status = device_blur(torch_cuda, images, b, grid, 0, False)
    assert rc == b.n and np.array_equal(got_first, first) and np.array_equal(got_status, status) and not status.any()
    assert np.array_equal(got, want) and not np.array_equal(got, buf)


@pytest.mark.parametrize("fmt", [2, 4])
def test_a_workspace_too_small_fills_the_tail(torch_cuda, images, fmt):
    if fmt == 4:
        buf, desc, pictures, dets, counts = rs.yuv_batch()
        cap, expected = rs.YUV_CAP, bs.expected_yuv
    else:
        dets, counts = rs.designed()
        buf, desc, pictures = rs.packed_batch(fmt)
        cap, expected = rs.CAP, bs.expected_packed
    b = Dev(torch_cuda, buf, desc, dets, counts, fmt, cap)
    total = int(rs.first_of(counts, cap)[-1])
    for records_cap in (0, 1, total - 1, total):
        rc, want, first, status = bs.host_blur(buf, fmt, desc, dets, counts, cap, 8, 250, False, records_cap=records_cap)
        got, got_first, got_status = device_blur(torch_cuda, images, b, 8, 250, False, records_cap=records_cap)
        assert rc == b.n and np.array_equal(got_first, first) and np.array_equal(got_status, status), records_cap
        assert got_status.tolist() == bs.want_status(counts, cap, records_cap), records_cap
        assert np.array_equal(got, want), records_cap
    assert np.array_equal(got, expected(pictures, fmt, dets, counts, cap, 8, 250, False)) and not got_status.any()
    got = device_blur(torch_cuda, images, b, 8, 250, False, records_cap=7)[0]
    assert np.array_equal(got, expected(pictures, fmt, dets, counts, cap, 8, 250, False, records_cap=7))


def test_invalid_descriptors_between_valid_ones(torch_cuda, images):
    """the buffer ends with its last picture (no tail): a descriptor one byte too far would touch bytes past the allocation if it were used"""
    dets, counts = rs.designed()
    buf, desc, pictures = rs.packed_batch(0)
    desc = desc.copy()
    desc["row_stride"][1] = int(desc["width"][1]) * 3 - 1                      # a stride below the row
    desc["offset"][3] = buf.nbytes + 1 - ((362 - 1) * int(desc["row_stride"][3]) + 410 * 3)          # ends one byte past the buffer
    desc["height"][5] = 0
    b = Dev(torch_cuda, buf, desc, dets, counts, 0, rs.CAP)
    for records_cap, want_status in ((None, [0, 1, 0, 1, 0, 1, 0]), (20, [0, 3, 2, 3, 2, 1, 0])):
        got, first, status = device_blur(torch_cuda, images, b, 8, 250, False, records_cap=records_cap)
        assert status.tolist() == want_status and np.array_equal(first, rs.first_of(counts, rs.CAP))
        assert np.array_equal(got, bs.expected_packed(pictures, 0, dets, counts, rs.CAP, 8, 250, False, records_cap=records_cap, invalid={1, 3, 5}))
        assert np.array_equal(got, bs.host_blur(buf, 0, desc, dets, counts, rs.CAP, 8, 250, False, records_cap=records_cap)[1])
    # surfaces: 1 (odd height) and 2 (the UV plane ends one byte past the buffer) are invalid
    ybuf, ydesc, surfaces, ydets, ycounts = rs.yuv_batch()
    ydesc = ydesc.copy()
    ydesc["height"][1] += 1
    d2 = ydesc[2]
    ydesc["offset_uv"][2] = ybuf.nbytes + 1 - ((int(d2["height"]) // 2 - 1) * int(d2["stride_uv"]) + int(d2["width"]))
    b = Dev(torch_cuda, ybuf, ydesc, ydets, ycounts, 5, rs.YUV_CAP)
    got, first, status = device_blur(torch_cuda, images, b, 16, 0, True)
    assert status.tolist() == [0, 1, 1, 0]
    assert np.array_equal(got, bs.expected_yuv(surfaces, 5, ydets, ycounts, rs.YUV_CAP, 16, 0, True, invalid={1, 2}))


def test_the_capacity_frame(torch_cuda, images):
    """1200 records on one 37 x 53 picture, cap 1200: the last slot's list of earlier owners holds 1199 entries"""
    dets, counts = rs.capacity_batch()
    pictures = [cs.in_format(rs.picture(0), 0)]
    buf, desc = rs.lay_out_packed(pictures)
    b = Dev(torch_cuda, buf, desc, dets, counts, 0, 1200)
    for grid, records_cap in ((8, 1200), (3, 600)):
        rc, want, first, status = bs.host_blur(buf, 0, desc, dets, counts, 1200, grid, 0, False, records_cap=records_cap)
        got, got_first, got_status = device_blur(torch_cuda, images, b, grid, 0, False, records_cap=records_cap)
        assert rc == 1 and got_first.tolist() == [0, 1200] and got_status.tolist() == [0 if records_cap == 1200 else 2] == status.tolist()
        assert np.array_equal(got, want) and not np.array_equal(got, buf), (grid, records_cap)
    assert np.array_equal(got, bs.expected_packed(pictures, 0, dets, counts, 1200, 3, 0, False, records_cap=600))


def test_a_sum_above_32_bits(torch_cuda, images):
    """4128 x 4096, every Y byte 255, grid 1: one cell whose sum is 4 311 613 440; every Y byte must still be 255"""
    torch = torch_cuda
    buf, desc, dets, counts = bs.big_surface()
    b = Dev(torch, buf, desc, dets, counts, 4, 1)
    d_px, out, work = torch.from_numpy(buf).cuda(), b.outputs(), b.work(images, 1, 1)
    launch(images, b, d_px, out, work, 1, 1, 0, False)
    torch.cuda.synchronize()
    assert out[0].cpu().tolist() == [0, 1] and out[1].cpu().tolist() == [0]
    assert (d_px[:4128 * 4096] == 255).all().item() and (d_px[4128 * 4096:] == 77).all().item()


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
    d_work, room = b.work(images, b.n * b.cap, 16)

    def untouched():
        torch.cuda.synchronize()
        return ((d_first == rs.SENTINEL32).all().item() and (d_status == rs.SENTINEL32).all().item() and (d_work == 0xA5).all().item()
                and np.array_equal(px[id(b)].cpu().numpy(), buf) and np.array_equal(px[id(yb)].cpu().numpy(), ybuf))

    def call(entry="blur_records_device", batch=b, fmt=0, n=None, cap=None, grid=8, colour=0, margin=0, flags=0, work=None, work_bytes=None,
             records_cap=None, first=None):
        fn = getattr(lib, "yf_images_" + entry)
        return fn(px[id(batch)].data_ptr(), batch.nbytes, fmt, batch.d_desc.data_ptr(), batch.d_dets.data_ptr(), batch.d_counts.data_ptr(),
                  batch.n if n is None else n, batch.cap if cap is None else cap, grid, colour, margin, flags,
                  d_work.data_ptr() if work is None else work, room if work_bytes is None else work_bytes,
                  batch.n * batch.cap if records_cap is None else records_cap, d_first.data_ptr() if first is None else first,
                  d_status.data_ptr(), None)

    yuv = dict(entry="blur_records_yuv_device", batch=yb, fmt=4)
    for kw, text in ((dict(grid=0), "grid must be"), (dict(grid=17), "grid must be"), (dict(grid=-1), "grid must be"),
                     (dict(colour=0x01000000), "top byte"), (dict(margin=1001), "margin_permille"), (dict(margin=-1), "margin_permille"),
                     (dict(flags=2), "flags"), (dict(cap=0), "cap"), (dict(cap=1201), "cap"), (dict(n=-1), "n must"),
                     (dict(n=2 ** 31 // 1200 + 1, cap=1200), "n * cap"), (dict(records_cap=-1), "records_cap"),
                     (dict(records_cap=b.n * b.cap + 1), "records_cap"), (dict(work_bytes=b.n * b.cap * 256 - 1), "work_bytes"),
                     (dict(work=0), "d_work"), (dict(work=d_work.data_ptr() + 8), "d_work"),
                     (dict(fmt=4), "yf_images_blur_records_yuv_device"), (dict(fmt=5), "yf_images_blur_records_yuv_device"),
                     (dict(yuv, fmt=0), "yf_images_blur_records_device"), (dict(yuv, fmt=3), "yf_images_blur_records_device"),
                     (dict(fmt=6), "format"), (dict(yuv, fmt=7), "format"), (dict(first=d_first.data_ptr() + 2), "4-byte aligned"),
                     (dict(yuv, grid=20), "grid must be"), (dict(yuv, colour=0xFF000000), "top byte"), (dict(yuv, margin=2000), "margin_permille")):
        assert call(**kw) <= 0 and text in last_error(lib), (kw, last_error(lib))
        assert untouched(), kw
    # n = 0: nothing is launched, 0 is returned, after the checks
    assert call(n=0, records_cap=0) == 0 and untouched()
    assert call(n=0, records_cap=0, grid=0) == 0 and "grid must be" in last_error(lib)
    assert images.blur_workspace(3, 3) == 112 and images.blur_workspace(-1, 8) == 0 and images.blur_workspace(1, 17) == 0
    # ... and the same arguments accepted; without a workspace no pointer is asked for
    assert call() == b.n and call(**yuv) == yb.n and call(records_cap=0, work=0, work_bytes=0) == b.n
    torch.cuda.synchronize()
    assert d_first[b.n].item() == int(rs.first_of(counts, rs.CAP)[-1]) and not untouched()


def test_the_blur_is_capturable(torch_cuda, images):
    """one call captured with the buffers allocated beforehand and replayed once: three kernels in a single chain"""
    torch = torch_cuda
    dets, counts = rs.designed()
    buf, desc, _ = rs.packed_batch(2)
    b = Dev(torch, buf, desc, dets, counts, 2, rs.CAP)
    records_cap = 100                                                          # the tail of the batch takes the fill path
    want = device_blur(torch, images, b, 8, 250, True, records_cap=records_cap)       # an ordinary call first, and the yardstick of the replay
    d_px, out, work = b.pixels(), b.outputs(), b.work(images, records_cap, 8)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            launch(images, b, d_px, out, work, records_cap, 8, 250, True, stream=s.cuda_stream)
    torch.cuda.synchronize()
    assert (out[0] == rs.SENTINEL32).all().item() and np.array_equal(d_px.cpu().numpy(), buf)            # captured, not run
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(d_px.cpu().numpy(), want[0]) and np.array_equal(out[0].cpu().numpy(), want[1])
    assert np.array_equal(out[1].cpu().numpy(), want[2]) and not np.array_equal(want[0], buf) and (want[2] & 2).any()


# ---- end to end ----
def _regions(ptq, boxes, w, h, permille, square):
    return [ptq.crop_region(box, w, h, permille, square) for box in boxes]


def _mask(regions, w, h):
    mask = np.zeros((h, w), bool)
    for x0, y0, rw, rh in (r for r in regions if r is not None):
        mask[y0:y0 + rh, x0:x0 + rw] = True
    return mask


def test_detect_blurred_on_the_real_images(network, torch_cuda, images, ptq):
    bgr = real_images(ptq)
    originals = [img.copy() for img in bgr]
    want = images.detect(network, bgr, iou_threshold=0.4)
    assert sum(w.shape[0] for w in want) >= 1, "detect reports no box: the comparison shows nothing"
    for kw, grid, permille, square in ((dict(), 8, 0, False), (dict(grid=16, margin=0.25, square=True), 16, 250, True), (dict(grid=1, margin=0.1), 1, 100, False)):
        pictures, boxes = images.detect_blurred(network, bgr, **kw)
        assert len(pictures) == len(bgr) and all(np.array_equal(a, w) and a.dtype == w.dtype for a, w in zip(boxes, want))
        changed = 0
        for i, img in enumerate(bgr):
            assert np.array_equal(img, originals[i])                           # the caller's arrays are not written
            regions = _regions(ptq, boxes[i], img.shape[1], img.shape[0], permille, square)
            assert pictures[i].shape == img.shape and np.array_equal(pictures[i], ptq.blur_u8(img, regions, grid)), (kw, i)
            differs = (pictures[i] != img).any(axis=2)
            assert not (differs & ~_mask(regions, img.shape[1], img.shape[0])).any(), (kw, i)
            changed += int(differs.sum())
        assert changed > 0, kw
    assert images.detect_blurred(network, []) == ([], [])
    with pytest.raises(ValueError, match="grid"):
        images.detect_blurred(network, bgr[:1], grid=17)


def test_detect_blurred_on_surfaces(network, torch_cuda, images, ptq):
    nv12, _, _ = real_surfaces()
    want = images.detect(network, nv12, fmt="nv12", iou_threshold=0.4)
    assert sum(w.shape[0] for w in want) >= 1
    for kw, grid, permille in ((dict(), 8, 0), (dict(grid=3, margin=0.25), 3, 250)):
        pictures, boxes = images.detect_blurred(network, nv12, fmt="nv12", **kw)
        assert all(np.array_equal(a, w) for a, w in zip(boxes, want))
        changed = 0
        for i, (y, uv) in enumerate(nv12):
            regions = _regions(ptq, boxes[i], y.shape[1], y.shape[0], permille, False)
            ry, ruv = ptq.blur_yuv420sp(y, uv, regions, grid)
            assert np.array_equal(pictures[i][0], ry) and np.array_equal(pictures[i][1], ruv), (kw, i)
            differs = pictures[i][0] != y
            assert not (differs & ~_mask(regions, y.shape[1], y.shape[0])).any(), (kw, i)
            changed += int(differs.sum())
        assert changed > 0, kw


def test_tracked_records_go_straight_into_the_blur(torch_cuda, images, ptq):
    """a clip of three frames whose middle frame has no detection: the tracker holds the face over, and the blur, which takes the
    tracker's output as its records, hides it there too"""
    torch = torch_cuda
    fmt, cap, out_cap, params = 0, 4, 8, (0.3, 1, 2)
    frames = [[([(10, 8, 33, 30), (40, 20, 55, 41)], None), ([], None), ([(12, 9, 35, 31)], None)]]
    dets, counts = ts.lay_out(frames, cap, ts.TIME)
    want = ts.expected(dets, counts, 1, 3, ts.TIME, cap, params, ts.empty_state(1), out_cap)
    assert want.out_counts.tolist() == [2, 2, 2]
    pictures = [cs.in_format(rs.picture(f), fmt) for f in (1, 4, 6)]             # three 64 x 48 pictures
    buf, desc = rs.lay_out_packed(pictures)
    tracker = images.Tracker(1, *params)
    d_dets = torch.from_numpy(dets.view(np.uint8).reshape(3, cap, 28).copy()).cuda()
    d_counts = torch.from_numpy(counts.copy()).cuda()
    d_out, d_info, d_oc, d_status = tracker.update(d_dets, d_counts, 3, "time", out_cap=out_cap)
    d_px = torch.from_numpy(buf.copy()).cuda()
    d_desc = torch.from_numpy(desc.view(np.uint8).copy()).cuda()
    d_first = torch.empty(4, dtype=torch.int32, device="cuda")
    d_bstatus = torch.empty(3, dtype=torch.int32, device="cuda")
    room = images.blur_workspace(3 * out_cap, 8)
    d_work = torch.empty(room, dtype=torch.uint8, device="cuda")
    images.blur_records_device(d_px.data_ptr(), buf.nbytes, fmt, d_desc.data_ptr(), d_out.data_ptr(), d_oc.data_ptr(), 3, out_cap,
                               d_work.data_ptr(), room, 3 * out_cap, d_first.data_ptr(), d_bstatus.data_ptr(), grid=8)
    torch.cuda.synchronize()
    assert d_oc.cpu().numpy().tolist() == [2, 2, 2] and not d_status.cpu().numpy().any() and not d_bstatus.cpu().numpy().any()
    blurred = []
    for f, p in enumerate(pictures):
        regions = [ptq.crop_region((int(d["x1"]), int(d["y1"]), int(d["x2"]), int(d["y2"])), 64, 48) for d in want.out[f, :want.out_counts[f]]]
        blurred.append(ptq.blur_u8(p, regions, 8))
    assert np.array_equal(d_px.cpu().numpy(), rs.lay_out_packed(blurred)[0])
    assert not np.array_equal(blurred[1], pictures[1])                         # the middle frame is blurred although it has no detection
