"""Letterboxed frames on the MI355X: the prepare kernels bit-equal to `ptq.letterbox_u8` (packed formats and NV12 / NV21, both frame
sides, int8 and fp16, an invalid descriptor between valid ones, more frames than workgroups), the decodes bit-equal to the host build
(both grids and the float logits, mixed aspects, caps below and above the firing count, with and without d_status), the identity with
the plain path on square pictures, and `detect` / `detect_tiled` with fit="letterbox" against the chain oracle -> restated decode ->
restated suppression."""
import numpy as np
import pytest

import tiles_support as ts
from fit_support import (DECODE_SIDES, DET, SMALL_SHAPES, YUV_SHAPES, decode_int8_restated, expect_frame_fit, host_decode_f32,
                         host_decode_int8, in_format, real_rgb, seeded_rgb, seeded_surface, sizes_desc, surface_rgb)
from float_support import special_logits
from images_support import (expect_kept, images_after_network, ptq, sentinels, suppress, synthetic_heads, synthetic_heads160,          # noqa: F401
                            torch_cuda)
from images_yuv_support import lay_out, real_surfaces

pytestmark = pytest.mark.gpu
KINDS = [(56, False), (160, False), (56, True)]             # (frame side, fp16 frames)
PAD = 114


@pytest.fixture(scope="module")
def fp16_network(network):
    network.fp16_init()
    return network


class FitFrames:
    """frames and status of a ragged batch on the device, prefilled with 77 and -7, one frame more than the batch has so that a write
    beyond the last frame shows"""

    def __init__(self, torch, buf, desc, S, f16):
        self.torch, self.n, self.nbytes, self.S, self.f16 = torch, desc.shape[0], buf.nbytes, S, f16
        self.d_px = torch.from_numpy(buf).cuda()
        self.d_desc = torch.from_numpy(desc.view(np.uint8).copy()).cuda()
        self.d_frames = torch.full((self.n + 1, S, S, 3), 77, dtype=torch.int16 if f16 else torch.int8, device="cuda")
        self.d_status = torch.full((self.n + 1,), -7, dtype=torch.int32, device="cuda")

    def prepare(self, images, fmt, pad=PAD):
        a = (self.d_px.data_ptr(), self.nbytes, fmt, self.d_desc.data_ptr(), self.n)
        yuv = images.is_yuv(fmt)
        if self.f16:
            (images.prepare_fit_yuv_f16_ragged_device if yuv else images.prepare_fit_f16_ragged_device)(
                *a, self.d_frames.data_ptr(), self.d_status.data_ptr(), pad=pad)
        else:
            (images.prepare_fit_yuv_ragged_device if yuv else images.prepare_fit_ragged_device)(
                *a, self.S, self.d_frames.data_ptr(), self.d_status.data_ptr(), pad=pad)

    def results(self):
        self.torch.cuda.synchronize()
        frames, status = self.d_frames.cpu().numpy(), self.d_status.cpu().numpy()
        assert (frames[self.n] == 77).all() and status[self.n] == -7, "written beyond the last frame"
        return (frames[:self.n].view(np.uint16) if self.f16 else frames[:self.n]), status[:self.n]


def _pictures():
    """about 35 RGB pictures: the small shapes, then the 27 real ones"""
    return [seeded_rgb(h, w) for h, w in SMALL_SHAPES] + list(real_rgb())


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_packed_frames_equal_letterbox_u8(torch_cuda, images, fmt):
    rgbs = _pictures()
    bad = len(rgbs) // 2                                                  # one invalid descriptor in the middle: its neighbours stay right
    buf, desc = images.pack_images([in_format(r, fmt) for r in rgbs], fmt)
    desc["row_stride"][bad] = desc["width"][bad] * images.CHANNELS[fmt] - 1
    for S, f16 in KINDS:
        b = FitFrames(torch_cuda, buf, desc, S, f16)
        b.prepare(images, fmt)
        frames, status = b.results()
        assert status.tolist() == [int(i == bad) for i in range(len(rgbs))]
        for i, rgb in enumerate(rgbs):
            if i == bad:
                assert (frames[i] == (0 if f16 else -128)).all()
            else:
                assert np.array_equal(frames[i], expect_frame_fit(rgb, S, PAD, f16)), (fmt, S, f16, i, rgb.shape)
    # the other pads on the small shapes (the padding is most of such a frame)
    small = len(SMALL_SHAPES)
    sbuf, sdesc = images.pack_images([in_format(r, fmt) for r in rgbs[:small]], fmt)
    for pad in (0, 255):
        for S, f16 in KINDS:
            b = FitFrames(torch_cuda, sbuf, sdesc, S, f16)
            b.prepare(images, fmt, pad=pad)
            frames, status = b.results()
            assert not status.any()
            for i in range(small):
                assert np.array_equal(frames[i], expect_frame_fit(rgbs[i], S, pad, f16)), (fmt, S, f16, pad, i)


@pytest.mark.parametrize("fmt", ["nv12", "nv21"])
def test_surface_frames_equal_letterbox_u8_of_the_converted_surface(torch_cuda, images, fmt):
    v_first = fmt == "nv21"
    nv12, nv21, _ = real_surfaces()
    surfaces = [seeded_surface(h, w) for h, w in YUV_SHAPES] + list(nv21 if v_first else nv12)
    buf, desc = lay_out(surfaces)                                         # odd pitches, UV planes before Y planes, nothing aligned
    bad = len(surfaces) // 2
    desc["height"][bad] += 1                                              # an odd height
    rgbs = [surface_rgb(y, uv, v_first) for y, uv in surfaces]
    for S, f16 in KINDS:
        b = FitFrames(torch_cuda, buf, desc, S, f16)
        b.prepare(images, fmt)
        frames, status = b.results()
        assert status.tolist() == [int(i == bad) for i in range(len(surfaces))]
        for i, rgb in enumerate(rgbs):
            if i == bad:
                assert (frames[i] == (0 if f16 else -128)).all()
            else:
                assert np.array_equal(frames[i], expect_frame_fit(rgb, S, PAD, f16)), (fmt, S, f16, i, rgb.shape)


@pytest.mark.parametrize("S,f16", KINDS)
def test_more_frames_than_workgroups(torch_cuda, images, S, f16):
    """pictures of 1 x 1 .. 8 x 8, the 64 shapes over and over: at least 600 of them and more than the launch has workgroups (eight per
    compute unit at most), so that every workgroup takes a second frame"""
    torch = torch_cuda
    n = max(600, torch.cuda.get_device_properties(0).multi_processor_count * 8 + 130)
    shapes = [(1 + k % 8, 1 + k // 8) for k in range(64)]
    rgbs = [seeded_rgb(h, w) for h, w in shapes]
    buf, d64 = images.pack_images(rgbs, "rgb")
    desc = d64[np.arange(n) % 64].copy()
    b = FitFrames(torch, buf, desc, S, f16)
    b.prepare(images, "rgb")
    torch.cuda.synchronize()
    want64 = np.stack([expect_frame_fit(r, S, PAD, f16) for r in rgbs])
    want = torch.from_numpy(want64.view(np.int16) if f16 else want64).cuda()[torch.arange(n, device="cuda") % 64]
    assert torch.equal(b.d_frames[:n], want)
    assert (b.d_status[:n] == 0).all().item() and (b.d_frames[n] == 77).all().item() and b.d_status[n].item() == -7


def _mixed_sides(n):
    sides = [DECODE_SIDES[i % len(DECODE_SIDES)] for i in range(n)]
    for i, hw in ((5, (0, 7)), (9, (7, 16385))):                          # sides out of range: count 0
        if i < n:
            sides[i] = hw
    return sides


def _check_decode(images, torch, kind, values, sides, cap, with_status):
    """one decode of `values` (int8 heads or float32 logits) with the descriptors of `sides` into sentinels: every frame's records and
    count equal the host build's, byte for byte; slots beyond min(count, cap) keep their sentinel"""
    n = values.shape[0]
    desc = sizes_desc(sides)
    d_desc = torch.from_numpy(desc.view(np.uint8).copy()).cuda()
    d_values = torch.from_numpy(values).cuda()
    d_dets, d_counts = sentinels(torch, n + 1, cap)
    status = np.zeros(n, np.int32)
    status[3::7] = 1
    d_status = torch.from_numpy(status).cuda() if with_status else None
    st = d_status.data_ptr() if with_status else None
    if kind == "f32":
        images.decode_f32_fit_ragged_device(d_values.data_ptr(), d_desc.data_ptr(), n, d_dets.data_ptr(), d_counts.data_ptr(), cap, d_status=st)
    else:
        images.decode_fit_ragged_device(d_values.data_ptr(), d_desc.data_ptr(), n, kind, d_dets.data_ptr(), d_counts.data_ptr(), cap, d_status=st)
    torch.cuda.synchronize()
    raw, counts = d_dets.cpu().numpy(), d_counts.cpu().numpy()
    assert (raw[n] == 0xA5).all() and counts[n] == -7, "written beyond the last frame"
    total = clipped = 0
    for f in range(n):
        h, w = sides[f]
        s = int(status[f]) if with_status else 0
        count, want = host_decode_f32(values[f], f, h, w, cap, status=s) if kind == "f32" else host_decode_int8(values[f], f, h, w, kind, cap, status=s)
        assert counts[f] == count, (kind, f, counts[f], count)
        k = min(count, cap)
        assert raw[f, :k].tobytes() == want.tobytes(), (kind, f, h, w)
        assert (raw[f, k:] == 0xA5).all(), (kind, f)
        total += k
        clipped += count > cap
    return total, clipped


@pytest.mark.parametrize("with_status", [False, True])
def test_decodes_equal_the_host_build(network, torch_cuda, images, with_status):
    images.set_decode_tables(*network.decode_tables())                    # the shipped pair, which the host build has compiled in
    rng = np.random.default_rng(77)
    heads56, heads160, logits = synthetic_heads(rng, 130), synthetic_heads160(rng, 26), special_logits()
    for kind, values, caps in ((56, heads56, (147, 20)), (160, heads160, (1200, 100)), ("f32", logits, (147, 5))):
        sides = _mixed_sides(values.shape[0])
        for cap in caps:                                                  # every candidate, and a cap below the firing count of most frames
            total, clipped = _check_decode(images, torch_cuda, kind, values, sides, cap, with_status)
            assert total > 0 and (clipped > 0) == (cap == caps[1]), (kind, cap, total, clipped)


def test_square_pictures_give_the_plain_paths_bytes(yf, fp16_network, torch_cuda, images):
    torch, network = torch_cuda, fp16_network
    rgbs = [seeded_rgb(1, 1), seeded_rgb(56, 56), real_rgb()[0][:300, :300], seeded_rgb(300, 300)] + [real_rgb()[k][:280, :280] for k in (1, 4, 6)]
    buf, desc = images.pack_images([np.ascontiguousarray(r[..., ::-1]) for r in rgbs], "bgr")
    n = len(rgbs)
    d_px, d_desc = torch.from_numpy(buf).cuda(), torch.from_numpy(desc.view(np.uint8).copy()).cuda()
    for S, f16 in KINDS:
        grid, cap = S // 8, 3 * (S // 8) ** 2
        out = []
        for fit in (False, True):
            d_frames = torch.full((n, S, S, 3), 77, dtype=torch.int16 if f16 else torch.int8, device="cuda")
            d_plain = torch.full((n, S, S, 3), 77, dtype=torch.int16 if f16 else torch.int8, device="cuda")
            d_heads = torch.zeros((n, grid, grid, 18), dtype=torch.float32 if f16 else torch.int8, device="cuda")
            d_dets, d_counts = sentinels(torch, n, cap)
            d_status = torch.full((n,), -7, dtype=torch.int32, device="cuda")
            head = (network, d_px.data_ptr(), buf.nbytes, "bgr", d_desc.data_ptr(), n)
            tail = (d_heads.data_ptr(), d_dets.data_ptr(), d_counts.data_ptr(), cap, d_status.data_ptr())
            if fit and f16:
                images.run_decode_fit_f16_ragged_device(*head, d_frames.data_ptr(), *tail)
                images.prepare_fit_f16_ragged_device(*head[1:], d_plain.data_ptr(), d_status.data_ptr())
            elif fit:
                images.run_decode_fit_ragged_device(*head, S, d_frames.data_ptr(), *tail)
                images.prepare_fit_ragged_device(*head[1:], S, d_plain.data_ptr(), d_status.data_ptr())
            elif f16:
                images.run_decode_f16_ragged_device(*head, d_frames.data_ptr(), *tail)
                images.prepare_f16_ragged_device(*head[1:], d_plain.data_ptr(), d_status.data_ptr())
            else:
                (images.run_decode_ragged_device if S == 56 else images.run_decode160_ragged_device)(*head, d_frames.data_ptr(), *tail)
                images.prepare_ragged_device(*head[1:], S, d_plain.data_ptr(), d_status.data_ptr())
            torch.cuda.synchronize()
            assert torch.equal(d_frames, d_plain) and not (d_frames == 77).all().item()
            out.append((d_frames.cpu().numpy(), d_heads.cpu().numpy(), d_dets.cpu().numpy(), d_counts.cpu().numpy(), d_status.cpu().numpy()))
        for a, b in zip(*out):
            assert a.tobytes() == b.tobytes(), (S, f16)
        assert out[0][3].sum() > 0, "no record on the square pictures: the identity of the decodes shows nothing"


def _chain(oracle, rgbs, S, first_frame=0):
    """the CPU chain on RGB pictures: ptq.letterbox_u8 frames, the oracle's network, the restated decode -> one DET array per picture"""
    frames = np.stack([expect_frame_fit(r, S, PAD) for r in rgbs])
    heads = oracle.run(frames)
    return [decode_int8_restated(heads[i], first_frame + i, r.shape[0], r.shape[1], S, oracle.sig, oracle.ex) for i, r in enumerate(rgbs)]


def _edges(recs):
    return np.stack([recs["x1"], recs["y1"], recs["x2"], recs["y2"]], axis=1).reshape(-1, 4).tolist() if len(recs) else []


@pytest.mark.parametrize("size", [56, 160])
def test_detect_letterbox_equals_the_chain(network, oracle, torch_cuda, images, size):
    rgbs = list(real_rgb())
    bgr = [np.ascontiguousarray(r[..., ::-1]) for r in rgbs]
    recs = _chain(oracle, rgbs, size)
    assert sum(r.shape[0] for r in recs) > 10 and max(r.shape[0] for r in recs) > 2, "hardly a record: the comparison shows nothing"
    got = images.detect(network, bgr, fit="letterbox", size=size)
    assert [g.tolist() for g in got] == [_edges(r) for r in recs]
    kept = images.detect(network, bgr, fit="letterbox", size=size, iou_threshold=0.4)
    want = [suppress(list(r), 0.4) for r in recs]
    assert [g.tolist() for g in kept] == [[[int(r[6]), int(r[7]), int(r[8]), int(r[9])] for r in rr] for rr in want]
    # "stretch" is the call without the keyword, and not the letterbox
    plain = images.detect(network, bgr, size=size)
    again = images.detect(network, bgr, fit="stretch", size=size)
    assert all(np.array_equal(a, b) for a, b in zip(plain, again)) and len(plain) == len(again)
    assert any(not np.array_equal(a, b) for a, b in zip(plain, got))
    # the records themselves, byte for byte, through the run entry with a cap below some counts
    cap = 2
    buf, desc = images.pack_images(bgr, "bgr")
    torch, n, grid = torch_cuda, len(bgr), size // 8
    d_px, d_desc = torch.from_numpy(buf).cuda(), torch.from_numpy(desc.view(np.uint8).copy()).cuda()
    d_frames = torch.empty((n, size, size, 3), dtype=torch.int8, device="cuda")
    d_heads = torch.empty((n, grid, grid, 18), dtype=torch.int8, device="cuda")
    d_dets, d_counts = sentinels(torch, n, cap)
    d_status = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    images.run_decode_fit_ragged_device(network, d_px.data_ptr(), buf.nbytes, "bgr", d_desc.data_ptr(), n, size, d_frames.data_ptr(),
                                        d_heads.data_ptr(), d_dets.data_ptr(), d_counts.data_ptr(), cap, d_status.data_ptr())
    torch.cuda.synchronize()
    raw, counts = d_dets.cpu().numpy(), d_counts.cpu().numpy()
    assert not d_status.cpu().numpy().any()
    for i, r in enumerate(recs):
        k = min(r.shape[0], cap)
        assert counts[i] == r.shape[0] and raw[i, :k].tobytes() == r[:k].tobytes() and (raw[i, k:] == 0xA5).all(), i


@pytest.mark.parametrize("size", [56, 160])
def test_detect_tiled_letterbox_equals_the_chain(network, oracle, torch_cuda, images, size):
    """one picture of 700 x 300 under tiles of 400 x 400: two tiles of 300 x 400 and the whole picture, none of them square"""
    real = real_rgb()
    rgb = np.ascontiguousarray(np.concatenate([real[0][:300, :350], real[3][:300, :299], real[9][:300, :51]], axis=1))
    assert rgb.shape == (300, 700, 3)
    bgr = [np.ascontiguousarray(rgb[..., ::-1])]
    tiles = ts.image_tiles(300, 700, 400, 400, 400, 400, True)
    assert len(tiles) == 3 and all(h != w for _, _, h, w in tiles)
    crops = [np.ascontiguousarray(rgb[y0:y0 + h, x0:x0 + w]) for x0, y0, h, w in tiles]
    recs = _chain(oracle, crops, size)
    cap = max(1, max(r.shape[0] for r in recs))
    dets = np.zeros((len(tiles), cap), DET)
    for j, r in enumerate(recs):
        dets[j, :r.shape[0]] = r
    counts = np.array([r.shape[0] for r in recs], np.int32)
    tile_rows = np.array([(0, x0, y0, h, w) for x0, y0, h, w in tiles], ts.TILE)
    merged = ts.merge_restated(dets, counts, cap, tile_rows, np.array([0, len(tiles)], np.int32))[0]
    assert merged.shape[0] > 0, "no record in any tile: the comparison shows nothing"
    got = images.detect_tiled(network, bgr, 400, fit="letterbox", iou_threshold=None, size=size)
    assert got[0].tolist() == _edges(merged)
    kept = expect_kept(merged, merged.shape[0], max(merged.shape[0], 1), 0.4)
    got = images.detect_tiled(network, bgr, 400, fit="letterbox", iou_threshold=0.4, size=size)
    assert got[0].tolist() == _edges(kept)
