"""Area-averaged frames on the MI355X: the device frames bit-equal to `ptq.resize_area_u8` / `ptq.letterbox_u8(..., interp="area")` at the
smallest shapes where the kernel can still go wrong -- one source pixel, one row, one column, one axis enlarged and one reduced, the
identity, one pixel off it, the exact 2x, rows of 16384 pixels (more than one range of columns) and 16384 rows of two --, in every
format, both frame sides, both elements and both fits, with odd offsets, row strides with slack and planes in either order, in a buffer
of exactly the pictures' extent; a picture whose sum needs 64 bits; the same pictures under every band count the host picks; invalid
descriptors, an empty batch and every argument refusal; and `detect(..., interp="area")` against the low-level calls composed by hand."""
import numpy as np
import pytest

from area_support import LETTERBOX, STRETCH, expect_frame_area, lay_out_packed
from fit_support import in_format, real_rgb, seeded_rgb, seeded_surface, surface_rgb
from images_support import images_after_network, last_error, ptq, sentinels, torch_cuda          # noqa: F401 (fixtures)
from images_yuv_support import lay_out, real_surfaces

pytestmark = pytest.mark.gpu
KINDS = [(56, False), (160, False), (56, True)]             # (frame side, fp16 frames)
FITS = [(STRETCH, "stretch"), (LETTERBOX, "letterbox")]
PAD = 93
SIZES = [(1, 1), (1, 7), (7, 1), (55, 57), (56, 56), (57, 57), (112, 112), (113, 111), (167, 300), (2, 16384), (16384, 2)]
YUV_SIZES = [(2, 2), (2, 8), (8, 2), (54, 58), (56, 56), (58, 58), (112, 112), (114, 110), (168, 300), (2, 16384), (16384, 2)]


@pytest.fixture(scope="module")
def fp16_network(network):
    network.fp16_init()
    return network


class AreaFrames:
    """frames and status of a ragged batch on the device, prefilled with 77 and -7, one frame more than the batch has so that a write
    beyond the last frame shows; the pixels are an allocation of exactly buf.nbytes"""

    def __init__(self, torch, buf, desc, S, f16, d_px=None):
        self.torch, self.n, self.nbytes, self.S, self.f16 = torch, desc.shape[0], buf.nbytes if d_px is None else d_px.numel(), S, f16
        self.d_px = torch.from_numpy(buf).cuda() if d_px is None else d_px
        self.d_desc = torch.from_numpy(desc.view(np.uint8).copy()).cuda()
        self.d_frames = torch.full((self.n + 1, S, S, 3), 77, dtype=torch.int16 if f16 else torch.int8, device="cuda")
        self.d_status = torch.full((self.n + 1,), -7, dtype=torch.int32, device="cuda")

    def prepare(self, images, fmt, fit="stretch", pad=PAD, n=None):
        n = self.n if n is None else n
        a = (self.d_px.data_ptr(), self.nbytes, fmt, self.d_desc.data_ptr(), n)
        yuv = images.is_yuv(fmt)
        if self.f16:
            (images.prepare_area_yuv_f16_ragged_device if yuv else images.prepare_area_f16_ragged_device)(
                *a, self.d_frames.data_ptr(), self.d_status.data_ptr(), fit=fit, pad=pad)
        else:
            (images.prepare_area_yuv_ragged_device if yuv else images.prepare_area_ragged_device)(
                *a, self.S, self.d_frames.data_ptr(), self.d_status.data_ptr(), fit=fit, pad=pad)

    def results(self):
        self.torch.cuda.synchronize()
        frames, status = self.d_frames.cpu().numpy(), self.d_status.cpu().numpy()
        assert (frames[self.n] == 77).all() and status[self.n] == -7, "written beyond the last frame"
        return (frames[:self.n].view(np.uint16) if self.f16 else frames[:self.n]), status[:self.n]


def _check(images, torch, buf, desc, rgbs, fmt, bad):
    for S, f16 in KINDS:
        for fit, name in FITS:
            b = AreaFrames(torch, buf, desc, S, f16)
            b.prepare(images, fmt, name)
            frames, status = b.results()
            assert status.tolist() == [int(i == bad) for i in range(len(rgbs))]
            for i, rgb in enumerate(rgbs):
                if i == bad:
                    assert (frames[i] == (0 if f16 else -128)).all()
                else:
                    assert np.array_equal(frames[i], expect_frame_area(rgb, S, fit, PAD, f16)), (fmt, S, f16, name, i, rgb.shape)


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_packed_frames_equal_the_restatement(torch_cuda, images, fmt):
    rgbs = [seeded_rgb(h, w) for h, w in SIZES]
    buf, desc = lay_out_packed([in_format(r, fmt) for r in rgbs], images.IMAGE_DTYPE)     # odd offsets, strides with slack, exact extent
    bad = 4                                                               # an invalid descriptor between valid ones: its neighbours stay right
    desc["row_stride"][bad] = desc["width"][bad] * images.CHANNELS[fmt] - 1
    _check(images, torch_cuda, buf, desc, rgbs, fmt, bad)


@pytest.mark.parametrize("fmt", ["nv12", "nv21"])
def test_surface_frames_equal_the_restatement_of_the_converted_surface(torch_cuda, images, fmt):
    v_first = fmt == "nv21"
    surfaces = [seeded_surface(h, w) for h, w in YUV_SIZES]
    buf, desc = lay_out(surfaces)                                         # odd pitches, UV planes before Y planes, nothing aligned
    bad = 5
    desc["height"][bad] += 1                                              # an odd height
    rgbs = [surface_rgb(y, uv, v_first) for y, uv in surfaces]
    _check(images, torch_cuda, buf, desc, rgbs, fmt, bad)


def test_pads_and_a_picture_that_ends_with_the_buffer(torch_cuda, images):
    rgbs = [seeded_rgb(3, 200), seeded_rgb(200, 3), seeded_rgb(57, 56)]
    buf, desc = lay_out_packed(rgbs, images.IMAGE_DTYPE, slack=0)
    for pad in (0, 255):
        for S, f16 in KINDS:
            b = AreaFrames(torch_cuda, buf, desc, S, f16)
            b.prepare(images, "rgb", "letterbox", pad)
            frames, status = b.results()
            assert not status.any()
            for i, rgb in enumerate(rgbs):
                assert np.array_equal(frames[i], expect_frame_area(rgb, S, LETTERBOX, pad, f16)), (S, f16, pad, i)


@pytest.mark.parametrize("S", [56, 160])
def test_a_sum_that_needs_64_bits(torch_cuda, images, S):
    """4112 x 4100 pixels of 255: H W 255 is above 2^32 (4104 x 4100, the size the issue names as an example of that, falls 0.1 % short
    of it), the frame is all 127; no restatement needed"""
    torch, h, w = torch_cuda, 4112, 4100
    assert h * w * 255 >= 2 ** 32
    d_px = torch.full((h * w * 3,), 255, dtype=torch.uint8, device="cuda")
    desc = np.zeros(1, images.IMAGE_DTYPE)
    desc[0] = (0, h, w, w * 3)
    b = AreaFrames(torch, None, desc, S, False, d_px=d_px)
    b.prepare(images, "bgr")
    frames, status = b.results()
    assert status.tolist() == [0] and (frames == 127).all()


@pytest.mark.parametrize("S,f16", KINDS)
def test_the_frames_do_not_depend_on_the_split_into_bands(torch_cuda, images, S, f16):
    """the small pictures as batches of one, inside a batch of 100 and inside one of 2100, padded with 8 x 8 pictures: three band counts"""
    torch = torch_cuda
    rgbs = [seeded_rgb(h, w) for h, w in SIZES[:9]] + [seeded_rgb(8, 8)]
    buf, desc = lay_out_packed(rgbs, images.IMAGE_DTYPE)
    k = len(rgbs) - 1
    counts = (1, 100, 2100)
    bands = [images.area_bands(n, S) for n in counts]
    assert bands[0] == S // 2 and bands[2] == 1 and len(set(bands)) == 3, bands          # else the test would pass vacuously
    d_px = torch.from_numpy(buf).cuda()
    for fit, name in FITS:
        want = np.stack([expect_frame_area(r, S, fit, PAD, f16) for r in rgbs])
        for n in counts[1:]:
            big = desc[np.concatenate([np.arange(k), np.full(n - k, k)])].copy()
            b = AreaFrames(torch, buf, big, S, f16, d_px=d_px)
            b.prepare(images, "rgb", name)
            torch.cuda.synchronize()
            d_want = torch.from_numpy(want.view(np.int16) if f16 else want).cuda()
            assert torch.equal(b.d_frames[:k], d_want[:k]), (n, name)
            assert torch.equal(b.d_frames[k:n], d_want[k:].expand(n - k, -1, -1, -1)), (n, name)
            assert (b.d_status[:n] == 0).all().item() and (b.d_frames[n] == 77).all().item() and b.d_status[n].item() == -7
        for i in range(k):
            b = AreaFrames(torch, buf, desc[i:i + 1].copy(), S, f16, d_px=d_px)
            b.prepare(images, "rgb", name)
            frames, status = b.results()
            assert status.tolist() == [0] and np.array_equal(frames[0], want[i]), (i, name)


def test_an_empty_batch_and_every_argument_refusal(torch_cuda, images):
    torch = torch_cuda
    rgb = seeded_rgb(7, 9)
    buf, desc = images.pack_images([rgb], "rgb")
    b = AreaFrames(torch, buf, desc, 56, False)
    b.prepare(images, "rgb", n=0)                                         # launches nothing, writes nothing
    torch.cuda.synchronize()
    assert (b.d_frames == 77).all().item() and (b.d_status == -7).all().item()
    lib = images.load()
    px, im, fr, st = b.d_px.data_ptr(), b.d_desc.data_ptr(), b.d_frames.data_ptr(), b.d_status.data_ptr()
    ok = dict(px=px, fmt=1, im=im, n=1, S=56, fit=0, pad=114, fr=fr, st=st)

    def call(entry, **kw):
        a = dict(ok, **kw)
        head = (a["px"], buf.nbytes, a["fmt"], a["im"], a["n"])
        tail = (a["fit"], a["pad"], a["fr"], a["st"], None)
        f16 = "f16" in entry
        rc = getattr(lib, "yf_images_" + entry)(*head, *(() if f16 else (a["S"],)), *tail)
        return rc, last_error(lib)

    packed, planes = ("prepare_area_ragged_device", "prepare_area_f16_ragged_device"), ("prepare_area_yuv_ragged_device", "prepare_area_yuv_f16_ragged_device")
    cases = [(dict(fmt=9), "format must be"), (dict(fit=2), "fit must be"), (dict(fit=-1), "fit must be"), (dict(pad=256), "pad"),
             (dict(pad=-1), "pad"), (dict(n=-1), "n < 0"), (dict(fr=None), "d_frames"), (dict(fr=fr + 8), "d_frames"), (dict(px=None), "d_pixels"),
             (dict(im=None), "d_pixels"), (dict(im=im + 4), "d_pixels"), (dict(st=None), "d_pixels"), (dict(st=st + 2), "d_pixels")]
    for entry in packed + planes:
        yuv = entry in planes
        base = dict(fmt=4) if yuv else {}
        for kw, word in cases + [(dict(fmt=1 if yuv else 4), "go through")] + ([] if "f16" in entry else [(dict(S=57), "56 or 160")]):
            rc, text = call(entry, **dict(base, **kw))
            assert rc == 0 and word in text, (entry, kw, text)
    torch.cuda.synchronize()
    assert (b.d_frames == 77).all().item() and (b.d_status == -7).all().item()          # no refusal launched anything
    rc, _ = call(packed[0])
    torch.cuda.synchronize()
    assert rc == 1 and b.d_status[0].item() == 0
    with pytest.raises(ValueError, match="fit"):
        b.prepare(images, "rgb", "crop")
    with pytest.raises(images.ImagesError):
        images.area_bands(1, 57)


# ---- end to end ----
def _by_hand(images, torch, network, pics, fmt, size, f16, fit, tile=None):
    """the area frames, the network and the decode that exists for the fit, from the low-level calls -> (frames, records, counts) as bytes"""
    yuv = images.is_yuv(fmt)
    buf, pictures = images.pack_yuv_images(pics, fmt) if yuv else images.pack_images(pics, fmt)
    desc = images.yuv_sizes(pictures) if yuv else pictures
    if tile is not None:
        _, desc, _ = images.plan_tiles(pictures, fmt, tile, None, True)
        pictures = desc
    n, grid = desc.shape[0], size // 8
    cap = 3 * grid * grid
    up = lambda a: torch.from_numpy(a.view(np.uint8).copy()).cuda()
    d_px, d_pictures, d_desc = torch.from_numpy(buf).cuda(), up(pictures), up(desc)
    d_frames = torch.empty((n, size, size, 3), dtype=torch.float16 if f16 else torch.int8, device="cuda")
    d_heads = torch.empty((n, grid, grid, 18), dtype=torch.float32 if f16 else torch.int8, device="cuda")
    d_dets = torch.empty((n, cap, 28), dtype=torch.uint8, device="cuda")
    d_counts = torch.empty(n, dtype=torch.int32, device="cuda")
    d_status = torch.empty(n, dtype=torch.int32, device="cuda")
    a = (d_px.data_ptr(), buf.nbytes, fmt, d_pictures.data_ptr(), n)
    out = (d_dets.data_ptr(), d_counts.data_ptr(), cap)
    if f16:
        (images.prepare_area_yuv_f16_ragged_device if yuv else images.prepare_area_f16_ragged_device)(*a, d_frames.data_ptr(), d_status.data_ptr(), fit=fit)
        network.fp16_run_device(d_frames.data_ptr(), d_heads.data_ptr(), n)
        (images.decode_f32_fit_ragged_device if fit == "letterbox" else images.decode_f32_ragged_device)(
            d_heads.data_ptr(), d_desc.data_ptr(), n, *out, d_status=d_status.data_ptr())
    else:
        images.set_decode_tables(*network.decode_tables())
        (images.prepare_area_yuv_ragged_device if yuv else images.prepare_area_ragged_device)(*a, size, d_frames.data_ptr(), d_status.data_ptr(), fit=fit)
        if size == 56:
            network.run_device(d_frames.data_ptr(), d_heads.data_ptr(), n)
        else:
            network.run_device_hw(size, size, d_frames.data_ptr(), d_heads.data_ptr(), n)
        if fit == "letterbox":
            images.decode_fit_ragged_device(d_heads.data_ptr(), d_desc.data_ptr(), n, size, *out, d_status=d_status.data_ptr())
        elif size == 56:
            images.decode_ragged_device(d_heads.data_ptr(), d_desc.data_ptr(), n, *out)
        else:
            images.decode160_ragged_device(d_heads.data_ptr(), d_desc.data_ptr(), n, *out, d_status=d_status.data_ptr())
    torch.cuda.synchronize()
    assert not d_status.cpu().numpy().any()
    return d_frames.cpu().numpy().tobytes(), d_dets.cpu().numpy(), d_counts.cpu().numpy()


def _records_equal(dets_a, counts_a, dets_b, counts_b):
    assert np.array_equal(counts_a, counts_b)
    for i, c in enumerate(counts_a):
        assert dets_a[i, :c].tobytes() == dets_b[i, :c].tobytes(), i
    return int(counts_a.sum())


VARIANTS = [dict(), dict(fit="letterbox"), dict(size=160), dict(size=160, fit="letterbox"), dict(dtype="fp16"), dict(dtype="fp16", fit="letterbox"),
            dict(fmt="nv12"), dict(fmt="nv21", fit="letterbox", size=160), dict(fmt="rgba")]


@pytest.mark.parametrize("kw", VARIANTS, ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()) or "default")
def test_detect_with_area_equals_the_calls_composed_by_hand(fp16_network, torch_cuda, images, kw):
    network, torch = fp16_network, torch_cuda
    fmt, size, f16, fit = kw.get("fmt", "bgr"), kw.get("size", 56), kw.get("dtype") == "fp16", kw.get("fit", "stretch")
    if images.is_yuv(fmt):
        nv12, nv21, _ = real_surfaces()
        pics = list(nv21 if fmt == "nv21" else nv12)[:12]
    else:
        pics = [in_format(r, images.format_code(fmt)) for r in real_rgb()[:12]]
    frames, dets, counts = _by_hand(images, torch, network, pics, fmt, size, f16, fit)
    b = images._stage(network, pics, fmt, None, None, None, size, "fp16" if f16 else "int8", fit=fit, interp="area")
    b.stream.synchronize()
    assert b.held[1].cpu().numpy().tobytes() == frames
    total = _records_equal(b.d_dets.cpu().numpy(), b.d_counts.cpu().numpy(), dets, counts)
    assert total > 3, "hardly a record: the comparison shows nothing"
    got = images.detect(network, pics, interp="area", **kw)
    want = b.boxes(counts)
    assert len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))
    linear = images.detect(network, pics, **kw)
    assert any(not np.array_equal(g, p) for g, p in zip(got, linear)), "area and linear frames gave the same boxes everywhere"


@pytest.mark.parametrize("size", [56, 160])
def test_detect_tiled_with_area_equals_the_calls_composed_by_hand(network, torch_cuda, images, size):
    real = real_rgb()
    rgb = np.ascontiguousarray(np.concatenate([real[0][:300, :350], real[3][:300, :299], real[9][:300, :51]], axis=1))
    bgr = [np.ascontiguousarray(rgb[..., ::-1])]
    for fit in ("stretch", "letterbox"):
        frames, dets, counts = _by_hand(images, torch_cuda, network, bgr, "bgr", size, False, fit, tile=400)
        assert counts.shape[0] == 3                                           # two tiles and the whole picture
        b = images._stage(network, bgr, "bgr", None, None, 0.4, size, "int8", tile=400, fit=fit, interp="area")
        b.stream.synchronize()
        assert b.held[1].cpu().numpy().tobytes() == frames
        assert _records_equal(b.held[3].cpu().numpy(), b.held[4].cpu().numpy(), dets, counts) > 0
        got = images.detect_tiled(network, bgr, 400, iou_threshold=0.4, size=size, fit=fit, interp="area")
        want = b.boxes(np.minimum(b.d_counts.cpu().numpy(), b.cap))
        assert np.array_equal(got[0], want[0]) and got[0].shape[0] > 0


def test_interp_linear_is_the_call_without_the_argument(network, torch_cuda, images):
    bgr = [np.ascontiguousarray(r[..., ::-1]) for r in real_rgb()[:12]]
    for kw in (dict(), dict(fit="letterbox"), dict(size=160)):
        a = images._stage(network, bgr, "bgr", None, None, None, kw.get("size", 56), "int8", fit=kw.get("fit", "stretch"))
        b = images._stage(network, bgr, "bgr", None, None, None, kw.get("size", 56), "int8", fit=kw.get("fit", "stretch"), interp="linear")
        a.stream.synchronize()
        assert _records_equal(a.d_dets.cpu().numpy(), a.d_counts.cpu().numpy(), b.d_dets.cpu().numpy(), b.d_counts.cpu().numpy()) > 3
        assert torch_cuda.equal(a.held[1], b.held[1])
        plain, again = images.detect(network, bgr, **kw), images.detect(network, bgr, interp="linear", **kw)
        assert all(np.array_equal(p, q) for p, q in zip(plain, again))
    with pytest.raises(ValueError, match="interp"):
        images.detect(network, bgr, interp="cubic")
    with pytest.raises(ValueError, match="interp"):
        images.evaluate(network, bgr, [np.zeros((0, 4))] * len(bgr), interp="nearest")
