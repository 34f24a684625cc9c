"""The drawing on the MI355X (yf_images_draw_records_device, yf_images_draw_records_yuv_device): the device against the host build of
csrc/yf_images_draw.h byte for byte over the whole pixel buffer of the designed batches of tests/draw_support.py -- padded rows, odd gaps,
a filler byte wherever no pixel lies, an invalid descriptor between valid ones -- in every format, half 0 to 3, with one colour and with
keyed colours, with d_first and d_status; once per format against the plain-numpy statement, so that this file stands alone; the frame of
1200 keyed records; invalid descriptors whose use would leave the allocation; a tracker's info rows as keys at stride 16; the host's
argument checks; stream capture; and `detect_drawn` end to end on the real images, without and with a `Tracker`.  Every comparison is
exact."""
import numpy as np
import pytest

import draw_support as ds
from images_support import images_after_network, last_error, ptq, real_images, torch_cuda      # noqa: F401 (fixtures; `images` is images_after_network)

pytestmark = pytest.mark.gpu

FORMATS = [0, 1, 2, 3, 4, 5]


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
        return (self.torch.full((self.n + 1,), ds.SENTINEL32, dtype=self.torch.int32, device="cuda"),
                self.torch.full((self.n,), ds.SENTINEL32, dtype=self.torch.int32, device="cuda"))


def _as_i32(torch, a):
    """uint32 host array -> int32 device tensor of the same bytes"""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).cuda()


def launch(images, b, d_px, out, half, d_keys=None, key_stride=0, d_pal=None, pn=0, stream=None):
    draw = images.draw_records_yuv_device if b.fmt in (4, 5) else images.draw_records_device
    draw(d_px.data_ptr(), b.nbytes, b.fmt, b.d_desc.data_ptr(), b.d_dets.data_ptr(), b.d_counts.data_ptr(), b.n, b.cap, out[0].data_ptr(),
         out[1].data_ptr(), half=half, colour=ds.COLOUR, d_keys=None if d_keys is None else d_keys.data_ptr(), key_stride=key_stride,
         d_palette=None if d_pal is None else d_pal.data_ptr(), palette_n=pn, stream=stream)


def device_draw(torch, images, b, half, keys=None, pal=None, buf=None):
    """-> (buffer, first, status) as the device left them; keys uint32 [n, cap, stride / 4], pal uint32 [palette_n], or None"""
    d_px, out = b.pixels(buf), b.outputs()
    if keys is None:
        launch(images, b, d_px, out, half)
    else:
        launch(images, b, d_px, out, half, _as_i32(torch, keys), keys.shape[2] * 4, _as_i32(torch, pal), pal.shape[0])
    torch.cuda.synchronize()
    return d_px.cpu().numpy(), out[0].cpu().numpy(), out[1].cpu().numpy()


@pytest.mark.parametrize("fmt", FORMATS)
def test_device_equals_the_host_build_on_the_designed_batch(torch_cuda, images, fmt):
    for half in ds.HALVES:
        buf, desc, _, dets, counts = ds.batch_of(fmt, half)
        b = Dev(torch_cuda, buf, desc, dets, counts, fmt, ds.CAP)
        stride, pn = ds.KEYED[half]
        keys, pal = ds.keys_for(b.n, ds.CAP, stride, half), ds.palette(pn)
        for k, p in ((None, None), (keys, pal)):
            where = (fmt, half, k is not None)
            rc, want, first, status = ds.host_draw(buf, fmt, desc, dets, counts, ds.CAP, half, keys=k, pal=p)
            assert rc == b.n and not np.array_equal(want, buf) and status.sum() == 1, where
            got, got_first, got_status = device_draw(torch_cuda, images, b, half, k, p)
            assert np.array_equal(got_first, first) and np.array_equal(got_status, status), where
            assert np.array_equal(got, want), where
    # ... and the host build is the restatement (tests/test_draw_host.py); once per format here, so that this file stands alone
    half = 1 + fmt % 3
    buf, desc, _, dets, counts = ds.batch_of(fmt, half)
    b = Dev(torch_cuda, buf, desc, dets, counts, fmt, ds.CAP)
    keys, pal = ds.keys_for(b.n, ds.CAP, 16, 9), ds.palette(256)
    assert np.array_equal(device_draw(torch_cuda, images, b, half)[0], ds.expected(fmt, half)), fmt
    assert np.array_equal(device_draw(torch_cuda, images, b, half, keys, pal)[0], ds.expected(fmt, half, keys, pal)), fmt


def test_a_second_call_and_permuted_records(torch_cuda, images):
    for fmt in (3, 5):
        buf, desc, _, dets, counts = ds.batch_of(fmt, 2)
        b = Dev(torch_cuda, buf, desc, dets, counts, fmt, ds.CAP)
        once = device_draw(torch_cuda, images, b, 2)[0]
        assert np.array_equal(device_draw(torch_cuda, images, b, 2, buf=once)[0], once)
        rng = np.random.default_rng(6600 + fmt)
        shuffled = dets.copy()
        for f in range(b.n):
            m = min(max(int(counts[f]), 0), ds.CAP)
            shuffled[f, :m] = dets[f, rng.permutation(m)]
        bs = Dev(torch_cuda, buf, desc, shuffled, counts, fmt, ds.CAP)
        assert np.array_equal(device_draw(torch_cuda, images, bs, 2)[0], once)
        keys, pal = ds.keys_for(b.n, ds.CAP, 4, 3), ds.palette(256)
        keyed = device_draw(torch_cuda, images, b, 2, keys, pal)[0]
        assert np.array_equal(device_draw(torch_cuda, images, b, 2, keys, pal, buf=keyed)[0], keyed)


def test_the_capacity_frame(torch_cuda, images):
    """1200 keyed records on one 64 x 48 picture, cap 1200: the first slot's list of later owners holds 1199 candidates"""
    dets, counts = ds.capacity_batch()
    for fmt in (1, 2):
        pictures = [ds.cs.in_format(ds._rgb(4), fmt)]
        buf, desc = ds.rs.lay_out_packed(pictures)
        b = Dev(torch_cuda, buf, desc, dets, counts, fmt, 1200)
        keys, pal = ds.keys_for(1, 1200, 16), ds.palette(256)
        for half in (0, 3):
            rc, want, first, status = ds.host_draw(buf, fmt, desc, dets, counts, 1200, half, keys=keys, pal=pal)
            got, got_first, got_status = device_draw(torch_cuda, images, b, half, keys, pal)
            assert rc == 1 and got_first.tolist() == [0, 1200] and got_status.tolist() == [0]
            assert np.array_equal(got, want) and not np.array_equal(got, buf), (fmt, half)
    assert np.array_equal(got, ds.expected_packed(pictures, 2, dets, counts, 1200, 3, keys, pal, invalid=()))


def test_invalid_descriptors_between_valid_ones(torch_cuda, images):
    """the buffer ends with its last picture (no tail): a descriptor one byte too far would touch bytes past the allocation if it were used"""
    buf, desc, pictures, dets, counts = ds.batch_of(0, 1)
    desc = desc.copy()
    w, h = ds.PACKED[5]
    desc["offset"][5] = buf.nbytes + 1 - ((h - 1) * int(desc["row_stride"][5]) + w * 3)          # ends one byte past the buffer
    desc["height"][0] = 0
    b = Dev(torch_cuda, buf, desc, dets, counts, 0, ds.CAP)
    keys, pal = ds.keys_for(b.n, ds.CAP, 4), ds.palette(3)
    for k, p in ((None, None), (keys, pal)):
        got, first, status = device_draw(torch_cuda, images, b, 1, k, p)
        assert status.tolist() == [1, 0, 1, 0, 0, 1, 0]
        assert np.array_equal(got, ds.expected_packed(pictures, 0, dets, counts, ds.CAP, 1, k, p, invalid=(0, 2, 5)))
        assert np.array_equal(got, ds.host_draw(buf, 0, desc, dets, counts, ds.CAP, 1, keys=k, pal=p)[1])
    # surfaces: 2 (odd height) and 3 (the UV plane ends one byte past the buffer) are invalid
    ybuf, ydesc, surfaces, ydets, ycounts = ds.batch_of(5, 3)
    ydesc = ydesc.copy()
    d3 = ydesc[3]
    ydesc["offset_uv"][3] = ybuf.nbytes + 1 - ((int(d3["height"]) // 2 - 1) * int(d3["stride_uv"]) + int(d3["width"]))
    b = Dev(torch_cuda, ybuf, ydesc, ydets, ycounts, 5, ds.CAP)
    got, first, status = device_draw(torch_cuda, images, b, 3)
    assert status.tolist() == [0, 0, 1, 1, 0, 0]
    assert np.array_equal(got, ds.expected_surfaces(surfaces, 5, ydets, ycounts, ds.CAP, 3, invalid=(2, 3)))


def test_track_info_rows_as_keys(torch_cuda, images):
    """the id column of a yf_track_info array, passed as the array with stride 16"""
    torch = torch_cuda
    buf, desc, pictures, dets, counts = ds.batch_of(1, 1)
    b = Dev(torch, buf, desc, dets, counts, 1, ds.CAP)
    info = np.zeros((b.n, ds.CAP), images.TRACK_INFO_DTYPE)
    info["id"] = 1 + np.arange(b.n * ds.CAP).reshape(b.n, ds.CAP) * 5
    info["hits"], info["misses"], info["age"] = 0x7F7F7F7F, -1, 0x01010101
    pal = np.array([c[0] << 16 | c[1] << 8 | c[2] for c in images.TRACK_PALETTE], np.uint32)
    keys = info.view(np.uint32).reshape(b.n, ds.CAP, 4)
    got = device_draw(torch, images, b, 1, keys, pal)[0]
    assert np.array_equal(got, ds.expected(1, 1, keys, pal))


def test_host_argument_checks_launch_nothing(torch_cuda, images):
    torch = torch_cuda
    lib = images.load()
    buf, desc, _, dets, counts = ds.batch_of(0, 1)
    b = Dev(torch, buf, desc, dets, counts, 0, ds.CAP)
    ybuf, ydesc, _, ydets, ycounts = ds.batch_of(4, 1)
    yb = Dev(torch, ybuf, ydesc, ydets, ycounts, 4, ds.CAP)
    px = {id(b): b.pixels(), id(yb): yb.pixels()}
    d_first, d_status = b.outputs()
    d_keys, d_pal = _as_i32(torch, ds.keys_for(b.n, ds.CAP, 16)), _as_i32(torch, ds.palette(3))
    kp, pp = d_keys.data_ptr(), d_pal.data_ptr()

    def untouched():
        torch.cuda.synchronize()
        return ((d_first == ds.SENTINEL32).all().item() and (d_status == ds.SENTINEL32).all().item()
                and np.array_equal(px[id(b)].cpu().numpy(), buf) and np.array_equal(px[id(yb)].cpu().numpy(), ybuf))

    def call(entry="draw_records_device", batch=b, fmt=0, n=None, cap=None, half=1, colour=0, keys=None, key_stride=0, palette=None, palette_n=0,
             first=None):
        fn = getattr(lib, "yf_images_" + entry)
        return fn(px[id(batch)].data_ptr(), batch.nbytes, fmt, batch.d_desc.data_ptr(), batch.d_dets.data_ptr(), batch.d_counts.data_ptr(),
                  batch.n if n is None else n, batch.cap if cap is None else cap, half, colour, keys, key_stride, palette, palette_n,
                  d_first.data_ptr() if first is None else first, d_status.data_ptr(), None)

    yuv = dict(entry="draw_records_yuv_device", batch=yb, fmt=4)
    keyed = dict(keys=kp, key_stride=16, palette=pp, palette_n=3)
    for kw, text in ((dict(half=-1), "half must be in [0, 3]"), (dict(half=4), "half must be in [0, 3]"), (dict(colour=0x01000000), "top byte"),
                     (dict(key_stride=4), "without d_keys"), (dict(palette=pp), "without d_keys"), (dict(palette_n=3), "without d_keys"),
                     (dict(keyed, key_stride=6), "key_stride"), (dict(keyed, key_stride=0), "key_stride"), (dict(keyed, key_stride=68), "key_stride"),
                     (dict(keyed, palette=None), "d_palette is NULL"), (dict(keyed, palette_n=0), "palette_n"), (dict(keyed, palette_n=257), "palette_n"),
                     (dict(keyed, keys=kp + 2), "4-byte aligned"), (dict(cap=0), "cap"), (dict(cap=1201), "cap"), (dict(n=-1), "n must"),
                     (dict(n=2 ** 31 // 1200 + 1, cap=1200), "n * cap"),
                     (dict(fmt=4), "yf_images_draw_records_yuv_device"), (dict(fmt=5), "yf_images_draw_records_yuv_device"),
                     (dict(yuv, fmt=0), "yf_images_draw_records_device"), (dict(yuv, fmt=3), "yf_images_draw_records_device"),
                     (dict(fmt=6), "format"), (dict(yuv, fmt=7), "format"), (dict(first=d_first.data_ptr() + 2), "4-byte aligned"),
                     (dict(yuv, half=5), "half"), (dict(yuv, colour=0xFF000000), "top byte"), (dict(yuv, **dict(keyed, key_stride=2)), "key_stride")):
        assert call(**kw) <= 0 and text in last_error(lib), (kw, last_error(lib))
        assert untouched(), kw
    # n = 0: nothing is launched, 0 is returned, after the checks
    assert call(n=0) == 0 and untouched()
    assert call(n=0, half=7) == 0 and "half must be" in last_error(lib)
    # ... and the same arguments accepted
    assert call() == b.n and call(**yuv) == yb.n and call(**keyed) == b.n
    torch.cuda.synchronize()
    assert d_first[b.n].item() == int(np.clip(counts, 0, ds.CAP).sum()) and not untouched()


def test_drawing_is_capturable(torch_cuda, images):
    """one keyed call captured with the buffers allocated beforehand and replayed once: two kernels in a single chain"""
    torch = torch_cuda
    buf, desc, _, dets, counts = ds.batch_of(2, 1)
    b = Dev(torch, buf, desc, dets, counts, 2, ds.CAP)
    keys, pal = ds.keys_for(b.n, ds.CAP, 4), ds.palette(256)
    want = device_draw(torch, images, b, 1, keys, pal)                         # an ordinary call first, and the yardstick of the replay
    d_px, out, d_keys, d_pal = b.pixels(), b.outputs(), _as_i32(torch, keys), _as_i32(torch, pal)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            launch(images, b, d_px, out, 1, d_keys, 4, d_pal, 256, stream=s.cuda_stream)
    torch.cuda.synchronize()
    assert (out[0] == ds.SENTINEL32).all().item() and np.array_equal(d_px.cpu().numpy(), buf)            # captured, not run
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(d_px.cpu().numpy(), want[0]) and np.array_equal(out[0].cpu().numpy(), want[1])
    assert np.array_equal(out[1].cpu().numpy(), want[2]) and not np.array_equal(want[0], buf)


# ---- end to end ----
def test_detect_drawn_on_the_real_images(network, torch_cuda, images, ptq):
    bgr = real_images(ptq)
    originals = [img.copy() for img in bgr]
    want = images.detect(network, bgr, iou_threshold=0.4)
    assert sum(w.shape[0] for w in want) >= 1, "detect reports no box: the comparison shows nothing"
    for kw, half, colour in ((dict(), 1, (0, 0, 255)), (dict(half=0, colour=(10, 200, 30)), 0, (30, 200, 10)), (dict(half=3, colour=0x0A0B0C), 3, (12, 11, 10))):
        pictures, boxes = images.detect_drawn(network, bgr, **kw)
        assert len(pictures) == len(bgr) and all(np.array_equal(a, w) and a.dtype == w.dtype for a, w in zip(boxes, want))
        changed = 0
        for i, img in enumerate(bgr):
            assert np.array_equal(img, originals[i])                           # the caller's arrays are not written
            assert pictures[i].shape == img.shape and np.array_equal(pictures[i], ptq.draw_rectangles_u8(img, boxes[i], half, colour)), (kw, i)
            changed += int((pictures[i] != img).any(axis=2).sum())
        assert changed > 0, kw
    assert images.detect_drawn(network, []) == ([], [])
    with pytest.raises(ValueError):
        images.detect_drawn(network, bgr[:1], half=4)


def test_detect_drawn_on_surfaces(network, torch_cuda, images, ptq):
    from images_yuv_support import real_surfaces
    nv12, nv21, _ = real_surfaces()
    for fmt, surfaces in (("nv12", nv12[:9]), ("nv21", nv21[:9])):
        want = images.detect(network, surfaces, fmt=fmt, iou_threshold=0.4)
        assert sum(w.shape[0] for w in want) >= 1
        pictures, boxes = images.detect_drawn(network, surfaces, fmt=fmt, half=2, colour=(81, 90, 240))
        assert all(np.array_equal(a, w) for a, w in zip(boxes, want))
        changed = 0
        for i, (y, uv) in enumerate(surfaces):
            ry, ruv = ptq.draw_rectangles_yuv420sp(y, uv, boxes[i], 2, (81, 90, 240), fmt == "nv21")
            assert np.array_equal(pictures[i][0], ry) and np.array_equal(pictures[i][1], ruv), (fmt, i)
            changed += int((pictures[i][0] != y).sum())
        assert changed > 0, fmt


def test_detect_drawn_with_a_tracker(network, torch_cuda, images, ptq):
    """two steps of one stream: the same photo, then the photo moved by two pixels -- its faces match across the frames and keep their
    colours; the tracks are detect_tracked's from an equal tracker"""
    bgr = real_images(ptq)
    first = next(img for img, boxes in zip(bgr, images.detect(network, bgr, iou_threshold=0.4)) if boxes.shape[0] >= 1)
    second = np.ascontiguousarray(np.roll(first, 2, axis=1))
    frames = [first, second]
    want = images.detect_tracked(network, frames, images.Tracker(1), 2)
    pictures, tracks = images.detect_drawn(network, frames, tracker=images.Tracker(1), steps=2)
    assert tracks == want and len(want[0]) >= 1
    shared = {t[0] for t in tracks[0]} & {t[0] for t in tracks[1]}
    assert shared, "no face matches across the two frames: the comparison shows nothing"
    table = [c[::-1] for c in images.TRACK_PALETTE]                            # BGR pictures
    for f, img in enumerate(frames):
        colours = [table[t[0] % 16] for t in tracks[f]]
        assert np.array_equal(pictures[f], ptq.draw_rectangles_u8(img, [t[1:5] for t in tracks[f]], 1, colours)), f
    for tid in shared:                                                         # the outline's own pixel (a corner of the box) carries the track's colour
        for f in range(2):
            t = next(t for t in tracks[f] if t[0] == tid)
            own = ptq.outline_mask(t[1:5], 1, frames[f].shape[1], frames[f].shape[0])
            for u in tracks[f]:
                if u[0] > tid:
                    own &= ~ptq.outline_mask(u[1:5], 1, frames[f].shape[1], frames[f].shape[0])
            assert own.any() and (pictures[f][own] == np.array(table[tid % 16], np.uint8)).all(), (tid, f)
    # a palette of the caller's: one colour draws every track alike
    pictures, tracks = images.detect_drawn(network, frames, tracker=images.Tracker(1), palette=[(1, 2, 3)], half=0)
    assert tracks == want
    for f, img in enumerate(frames):
        assert np.array_equal(pictures[f], ptq.draw_rectangles_u8(img, [t[1:5] for t in tracks[f]], 0, (3, 2, 1))), f
