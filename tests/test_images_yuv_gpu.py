"""NV12 / NV21 surfaces on the MI355X: frames bit-exact against the restated conversion (ptq.yuv420sp_to_rgb_u8, unpinned against a real
cv2) under the frame of the BGR path that exists, for every shape of the list, both chroma orders, both frame sizes, int8 and fp16, in a
layout with odd pitches, UV planes before Y planes and filler between the samples; and the whole path -- surfaces to boxes -- against
the BGR path on the converted pictures."""
import numpy as np
import pytest

from images_support import images_after_network, ptq, torch_cuda          # noqa: F401 (fixtures; `images` is images_after_network)
from images_yuv_support import SHAPES, all_surfaces, expected_frame, f16_table, lay_out, real_surfaces, restated_rgb, surface

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fp16_network(network):
    network.fp16_init()
    return network


class YuvBatch:
    """a laid-out ragged batch of surfaces on the device; one frame more than the batch has, so that a write beyond the last frame shows"""

    def __init__(self, torch, buf, desc, out, f16=False):
        self.n, self.nbytes, self.out, self.f16 = desc.shape[0], buf.nbytes, out, f16
        self.d_px = torch.from_numpy(buf).cuda()
        self.d_desc = torch.from_numpy(desc.view(np.uint8).copy()).cuda()
        self.d_frames = torch.full((self.n + 1, out, out, 3), 77, dtype=torch.int16 if f16 else torch.int8, device="cuda")
        self.d_status = torch.full((self.n + 1,), -7, dtype=torch.int32, device="cuda")

    def prepare(self, images, fmt):
        if self.f16:
            images.prepare_yuv_f16_ragged_device(self.d_px.data_ptr(), self.nbytes, fmt, self.d_desc.data_ptr(), self.n, self.d_frames.data_ptr(),
                                                 self.d_status.data_ptr())
        else:
            images.prepare_yuv_ragged_device(self.d_px.data_ptr(), self.nbytes, fmt, self.d_desc.data_ptr(), self.n, self.out,
                                             self.d_frames.data_ptr(), self.d_status.data_ptr())

    def results(self, torch):
        """(frames [n], status [n]) after checking the guards behind them"""
        torch.cuda.synchronize()
        frames, status = self.d_frames.cpu().numpy(), self.d_status.cpu().numpy()
        assert (frames[self.n] == 77).all() and status[self.n] == -7, "written beyond the last frame"
        return frames[:self.n].view(np.uint16) if self.f16 else frames[:self.n], status[:self.n]


@pytest.mark.parametrize("out", [56, 160])
@pytest.mark.parametrize("fmt", ["nv12", "nv21"])
def test_ragged_frames_equal_the_restatement(torch_cuda, images, fmt, out):
    items = all_surfaces()
    buf, desc = lay_out([surface(k, c) for k, c in items])
    b = YuvBatch(torch_cuda, buf, desc, out)
    b.prepare(images, fmt)
    frames, status = b.results(torch_cuda)
    assert (status == 0).all()
    for i, (k, c) in enumerate(items):
        assert np.array_equal(frames[i], expected_frame(k, c, fmt == "nv21", out)), (SHAPES[k], c, fmt, out)


@pytest.mark.parametrize("fmt", ["nv12", "nv21"])
def test_ragged_fp16_frames_equal_the_restatement(torch_cuda, images, fmt):
    items = all_surfaces()
    buf, desc = lay_out([surface(k, c) for k, c in items])
    b = YuvBatch(torch_cuda, buf, desc, 56, f16=True)
    b.prepare(images, fmt)
    frames, status = b.results(torch_cuda)
    assert (status == 0).all()
    half = f16_table()
    for i, (k, c) in enumerate(items):
        assert np.array_equal(frames[i], half[restated_rgb(k, c, fmt == "nv21", 56)]), (SHAPES[k], c, fmt)


def test_uniform_batch(torch_cuda, images, ptq):
    """5 surfaces of 112 x 112, frame_stride above the surface's size, uv_offset above stride_y * h, odd pitches, filler everywhere else"""
    torch = torch_cuda
    n, h, w = 5, 112, 112
    sy, suv = w + 3, w + 6
    uv_off = sy * h + 9
    fs = uv_off + suv * (h // 2) + 13
    rng = np.random.default_rng(21)
    ext_uv = (h // 2 - 1) * suv + w
    buf = np.full((n - 1) * fs + uv_off + ext_uv, 0x5B, np.uint8)              # the last UV plane ends with the buffer
    surfaces = []
    for i in range(n):
        y, uv = rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w), dtype=np.uint8)
        np.lib.stride_tricks.as_strided(buf[i * fs:], (h, w), (sy, 1))[:] = y
        np.lib.stride_tricks.as_strided(buf[i * fs + uv_off:], (h // 2, w), (suv, 1))[:] = uv
        surfaces.append((y, uv))
    d_px = torch.from_numpy(buf).cuda()
    half = f16_table()
    for fmt in ("nv12", "nv21"):
        rgb = [ptq.yuv420sp_to_rgb_u8(y, uv, fmt == "nv21") for y, uv in surfaces]
        for out in (56, 160):
            d_frames = torch.full((n + 1, out, out, 3), 77, dtype=torch.int8, device="cuda")
            images.prepare_yuv_device(d_px.data_ptr(), buf.nbytes, fmt, h, w, sy, uv_off, suv, fs, n, out, d_frames.data_ptr())
            torch.cuda.synchronize()
            got = d_frames.cpu().numpy()
            assert (got[n] == 77).all()
            for i in range(n):
                want = ptq.resize_linear_u8(rgb[i], out, out)
                assert np.array_equal(got[i], (want.astype(np.int16) - 128).astype(np.int8)), (fmt, out, i)
        d_f16 = torch.full((n + 1, 56, 56, 3), 77, dtype=torch.int16, device="cuda")
        images.prepare_yuv_f16_device(d_px.data_ptr(), buf.nbytes, fmt, h, w, sy, uv_off, suv, fs, n, d_f16.data_ptr())
        torch.cuda.synchronize()
        got = d_f16.cpu().numpy()
        assert (got[n] == 77).all()
        for i in range(n):
            assert np.array_equal(got[i].view(np.uint16), half[ptq.resize_linear_u8(rgb[i], 56, 56)]), (fmt, i)
    # one byte less of buffer: refused on the host, nothing launched
    with pytest.raises(images.ImagesError, match="last surface"):
        images.prepare_yuv_device(d_px.data_ptr(), buf.nbytes - 1, "nv12", h, w, sy, uv_off, suv, fs, n, 56, d_frames.data_ptr())


def test_invalid_descriptors_are_flagged_between_valid_ones(torch_cuda, images):
    ks = [3, 7, 4, 8, 6, 9, 1, 5, 0, 3, 2]
    buf, desc = lay_out([surface(k, False) for k in ks])
    ext = lambda d, rows, stride: (int(d[rows]) - 1) * int(d[stride]) + int(d["width"])
    desc["height"][1] += 1                                                     # odd height
    desc["offset_y"][3] = buf.nbytes + 1 - ext(desc[3], "height", "stride_y")  # the Y plane ends one byte past the buffer
    d5 = desc[5]
    desc["offset_uv"][5] = buf.nbytes + 1 - ((int(d5["height"]) // 2 - 1) * int(d5["stride_uv"]) + int(d5["width"]))   # ... the UV plane
    desc["stride_y"][7] = desc["width"][7] - 1                                 # a stride below the width
    desc["width"][9] -= 1                                                      # odd width
    bad = [1, 3, 5, 7, 9]
    for out, f16 in ((56, False), (160, False), (56, True)):
        b = YuvBatch(torch_cuda, buf, desc, out, f16)
        b.prepare(images, "nv12")
        frames, status = b.results(torch_cuda)
        assert status.tolist() == [int(i in bad) for i in range(len(ks))]
        half = f16_table()
        for i, k in enumerate(ks):
            if i in bad:
                assert (frames[i] == (0 if f16 else -128)).all(), (i, out, f16)
            elif f16:
                assert np.array_equal(frames[i], half[restated_rgb(k, False, False, 56)]), (i, SHAPES[k])
            else:
                assert np.array_equal(frames[i], expected_frame(k, False, False, out)), (i, SHAPES[k], out)
    # the planes that end exactly with the buffer are valid (lay_out ends the last plane there): status 0 above for the last surface


def _centre_boxes(shapes):
    return [np.array([[w / 4, h / 4, 3 * w / 4, 3 * h / 4]]) for h, w in shapes]


@pytest.mark.parametrize("size,dtype", [(56, "int8"), (160, "int8"), (56, "fp16")])
def test_surfaces_to_boxes_equal_the_bgr_path(fp16_network, torch_cuda, images, size, dtype):
    """The 27 real images, cropped to even sides and turned into NV12 by a float forward conversion (input only): detect and evaluate on the
    surfaces equal detect and evaluate (the code that exists) on the restated BGR of the same surfaces, array for array, without and with
    suppression; the NV21 spelling of the same surfaces gives the same boxes.  The BGR side must report boxes, or the comparison is
    vacuous: on the CPU the oracle (oracle/oracle.py: run on the restated 56x56 frames, decode_py with each picture's scales) finds 37
    records in 25 of these 27 converted pictures (39 in the pictures before the conversion)."""
    network = fp16_network
    nv12, nv21, bgr = real_surfaces()
    gts = _centre_boxes([y.shape for y, _ in nv12])
    for thr in (None, 0.4):
        want = images.detect(network, bgr, fmt="bgr", iou_threshold=thr, size=size, dtype=dtype)
        assert sum(b.shape[0] for b in want) >= 1, "the BGR path reports no box: the comparison shows nothing"
        for fmt, surfaces in (("nv12", nv12), ("nv21", nv21)):
            got = images.detect(network, surfaces, fmt=fmt, iou_threshold=thr, size=size, dtype=dtype)
            assert len(got) == len(want)
            for i, (g, w) in enumerate(zip(got, want)):
                assert g.dtype == w.dtype and np.array_equal(g, w), (fmt, thr, i)
        score = images.evaluate(network, bgr, gts, fmt="bgr", iou_threshold=thr, size=size, dtype=dtype)
        assert score["detections"] >= 1
        assert images.evaluate(network, nv12, gts, fmt="nv12", iou_threshold=thr, size=size, dtype=dtype) == score
    # cv2's one-array layout is the same surface
    whole = [np.concatenate([y, uv]) for y, uv in nv12[:3]]
    a = images.detect(network, whole, fmt="nv12", size=size, dtype=dtype)
    b = images.detect(network, nv12[:3], fmt="nv12", size=size, dtype=dtype)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
