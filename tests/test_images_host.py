"""libyf_images on the host (no GPU): pack_images' layout, the argument checks of the uniform entry points (which return before any launch),
and the resize arithmetic of csrc/yf_images_taps.h -- the same functions the device kernel calls, compiled for the host -- against
ptq.resize_linear_u8 for every image side 1..8192 at both output sizes."""
import concurrent.futures
import ctypes
import importlib
import os

import numpy as np
import pytest

from images_support import PKG, host, host_lib, images, last_error          # noqa: F401 (host, images: fixtures)


def _resize_host(lib, img, out):
    a = np.ascontiguousarray(img)
    h, w, c = a.shape
    dst = np.empty((out, out, c), np.uint8)
    assert lib.yfi_resize_host(a.ctypes.data, h, w, c, a.strides[0], out, out, dst.ctypes.data) == 0
    return dst


def _sweep(args):
    """one worker: sizes [lo, hi) as 1 x W and H x 1 images at output size `out`; returns the sizes that differ"""
    lo, hi, out = args
    ptq = importlib.import_module("stm32h7-yolo_amd.ptq")
    lib = host_lib(build=False)
    bad = []
    for s in range(lo, hi):
        rng = np.random.default_rng(s * 1000 + out)
        for shape in ((1, s, 3), (s, 1, 3)):
            img = rng.integers(0, 256, shape, dtype=np.uint8)
            if not np.array_equal(_resize_host(lib, img, out), ptq.resize_linear_u8(img, out, out)):
                bad.append(shape)
    return bad


@pytest.mark.parametrize("out", [56, 160])
def test_taps_equal_the_restatement_for_every_side_up_to_8192(host, out):
    chunks = [(lo, min(lo + 512, 8193), out) for lo in range(1, 8193, 512)]
    workers = max(1, min(8, os.cpu_count() or 1))
    with concurrent.futures.ProcessPoolExecutor(workers) as ex:
        bad = [b for part in ex.map(_sweep, chunks) for b in part]
    assert not bad, f"{len(bad)} sizes differ from ptq.resize_linear_u8 at {out}: {bad[:10]}"


def test_taps_on_2d_images_and_exact_halving(host):
    ptq = importlib.import_module("stm32h7-yolo_amd.ptq")
    rng = np.random.default_rng(7)
    for (h, w) in [(112, 112), (362, 410), (55, 57), (1, 1), (480, 640), (113, 111), (7, 3000)]:
        for c in (3, 4):
            img = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
            for out in (56, 160):
                assert np.array_equal(_resize_host(host, img, out), ptq.resize_linear_u8(img, out, out)), (h, w, c, out)
    # an exact 2x reduction is OpenCV's INTER_AREA path: (a + b + c + d + 2) >> 2 -- the linear weights give the same
    img = rng.integers(0, 256, (112, 112, 3), dtype=np.uint8).astype(np.int32)
    area = (img[0::2, 0::2] + img[0::2, 1::2] + img[1::2, 0::2] + img[1::2, 1::2] + 2) >> 2
    assert np.array_equal(_resize_host(host, img.astype(np.uint8), 56), area.astype(np.uint8))


def test_taps_stay_inside_the_image(host):
    t = (ctypes.c_int32 * 4)()
    for n_in in (1, 2, 3, 55, 56, 57, 111, 112, 113, 159, 160, 161, 8192, 16384):
        for out in (56, 160):
            for d in range(out):
                host.yfi_tap_host(d, out, n_in, t)
                s0, s1, w0, w1 = list(t)
                assert 0 <= s0 <= s1 <= n_in - 1 and s1 - s0 <= 1 and w0 >= 0 and w1 >= 0 and w0 + w1 == 2048, (n_in, out, d, list(t))


def test_descriptor_check(host):
    ok = host.yfi_image_ok_host
    assert ok(0, 2, 3, 9, 3, 18) == 1                 # (2 - 1) * 9 + 3 * 3 = 18
    assert ok(0, 2, 3, 9, 3, 17) == 0
    assert ok(1, 2, 3, 9, 3, 18) == 0                 # offset pushes the last pixel past the end
    assert ok(0, 0, 3, 9, 3, 100) == 0 and ok(0, 2, 0, 9, 3, 100) == 0
    assert ok(0, 16385, 1, 3, 3, 1 << 40) == 0 and ok(0, 1, 16385, 49155, 3, 1 << 40) == 0
    assert ok(0, 2, 3, 8, 3, 100) == 0                # row stride below w * C
    assert ok(0, 1, 3, 1 << 62, 3, 9) == 1            # one row: the stride is never applied
    assert ok(0, 16384, 1, 1 << 62, 3, (1 << 64) - 1) == 0     # no overflow in (h - 1) * row_stride
    assert ok((1 << 64) - 1, 1, 1, 3, 3, 10) == 0
    assert ok(0, 2, 2, 8, 4, 16) == 1                 # 4 bytes per pixel


def test_pack_images_offsets_and_strides(images):
    rng = np.random.default_rng(1)
    a = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    parent = rng.integers(0, 256, (40, 50, 3), dtype=np.uint8)
    crop = parent[10:30, 5:25]                         # a view: row stride 150 bytes
    b = rng.integers(0, 256, (1, 1, 3), dtype=np.uint8)
    buf, desc = images.pack_images([a, crop, b], "bgr")
    assert desc.dtype == images.IMAGE_DTYPE and desc.dtype.itemsize == 24
    assert list(desc["height"]) == [5, 20, 1] and list(desc["width"]) == [7, 20, 1]
    assert list(desc["row_stride"]) == [21, 150, 3]
    assert desc["offset"][0] == 0 and all(o % 16 == 0 for o in desc["offset"])
    assert desc["offset"][1] >= 5 * 21 and desc["offset"][2] >= desc["offset"][1] + 19 * 150 + 60
    for img, d in zip([a, crop, b], desc):
        o, h, w, rs = int(d["offset"]), int(d["height"]), int(d["width"]), int(d["row_stride"])
        got = np.lib.stride_tricks.as_strided(buf[o:], shape=(h, w, 3), strides=(rs, 3, 1))
        assert np.array_equal(got, img)
    assert buf.nbytes == desc["offset"][2] + 3


def test_pack_images_four_channels_and_other_layouts(images):
    rng = np.random.default_rng(2)
    rgba = rng.integers(0, 256, (9, 11, 4), dtype=np.uint8)
    planar = np.ascontiguousarray(rng.integers(0, 256, (3, 6, 8), dtype=np.uint8)).transpose(1, 2, 0)    # channel stride 48: copied
    buf, desc = images.pack_images([rgba[1:8, 2:9]], "rgba")
    assert int(desc["row_stride"][0]) == 44 and int(desc["width"][0]) == 7
    got = np.lib.stride_tricks.as_strided(buf, shape=(7, 7, 4), strides=(44, 4, 1))
    assert np.array_equal(got, rgba[1:8, 2:9])
    buf, desc = images.pack_images([planar], images.YF_PIX_RGB8)
    assert int(desc["row_stride"][0]) == 24
    assert np.array_equal(buf[:6 * 24].reshape(6, 8, 3), planar)
    with pytest.raises(ValueError, match="negative"):
        images.pack_images([rgba[::-1]], "rgba")
    with pytest.raises(ValueError):
        images.pack_images([rgba], "bgr")                # 4 channels under a 3-byte format
    with pytest.raises(ValueError):
        images.pack_images([rgba.astype(np.int16)], "rgba")
    with pytest.raises(ValueError):
        images.pack_images([rgba], "yuv")


def test_uniform_entry_points_check_every_argument_before_any_launch(images):
    lib = images.load()
    P, F, H, D, C = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000        # never dereferenced: every call below fails its host checks
    good = dict(d_pixels=P, pixels_bytes=362 * 1230 * 4, format=0, height=362, width=410, row_stride=1230, frame_stride=362 * 1230, n=4,
                out_hw=56, d_frames=F)

    def prep(**kw):
        a = dict(good, **kw)
        rc = lib.yf_images_prepare_device(a["d_pixels"], a["pixels_bytes"], a["format"], a["height"], a["width"], a["row_stride"],
                                          a["frame_stride"], a["n"], a["out_hw"], a["d_frames"], None)
        return rc, last_error(lib)

    cases = {
        "format": dict(format=4), "out_hw": dict(out_hw=112), "n < 0": dict(n=-1), "16-byte": dict(d_frames=F + 4),
        "height and width": dict(height=0), "row_stride": dict(row_stride=1229), "frame_stride < 0": dict(frame_stride=-1),
        "d_pixels": dict(d_pixels=None), "first image": dict(pixels_bytes=1000), "last image": dict(pixels_bytes=362 * 1230 * 4 - 1),
    }
    for word, kw in cases.items():
        rc, text = prep(**kw)
        assert rc <= 0 and word in text, (kw, rc, text)
    rc, text = prep(width=16385, row_stride=16385 * 3)
    assert rc <= 0 and "height and width" in text
    rc, text = prep(format=2, row_stride=410 * 3)        # BGRA: 4 bytes per pixel
    assert rc <= 0 and "row_stride" in text
    # the run-and-decode form checks the decode arguments too, all before its first launch
    a = good

    def run(net=0x60000, mode=0, cap=147, heads=H, dets=D, counts=C):
        rc = lib.yf_images_run_decode_device(net, a["d_pixels"], a["pixels_bytes"], 0, 362, 410, 1230, 362 * 1230, 4, F, heads, mode,
                                             dets, counts, cap, None)
        return rc, last_error(lib)
    for kw, word in [(dict(net=None), "handle"), (dict(mode=3), "mode"), (dict(cap=0), "cap"), (dict(dets=None), "NULL"),
                     (dict(counts=C + 2), "aligned")]:
        rc, text = run(**kw)
        assert rc <= 0 and word in text, (kw, rc, text)
    rc = lib.yf_images_run_decode_device(0x60000, P, 100, 0, 362, 410, 1230, 0, 1, F, H, 0, D, C, 147, None)
    assert rc <= 0 and "first image" in last_error(lib)
    # the ragged forms: host-side checks of what the host can see
    rc = lib.yf_images_prepare_ragged_device(P, 100, 0, None, 3, 56, F, 0x70000, None)
    assert rc <= 0 and "d_images" in last_error(lib)
    rc = lib.yf_images_decode_ragged_device(H, 0x70000, 3, 7, D, C, 147, None)
    assert rc <= 0 and "mode" in last_error(lib)
    # n = 0 is a valid empty batch: nothing is launched
    assert prep(n=0, d_pixels=None, pixels_bytes=0)[0] == 0


def test_library_is_built_from_its_own_sources(images):
    lib = images.load()
    assert (lib.yf_images_build_id() or b"").decode() == images.expected_build_id()
    # the network library's build id is computed from flags.mk's DEVICE_SRCS, which the companion library is not part of
    binding = importlib.import_module("stm32h7-yolo_amd.binding")
    flags = open(os.path.join(PKG, "csrc", "flags.mk")).read()
    assert "yf_images" not in flags
    assert binding.expected_build_id() == (binding.load().yf_network_build_id() or b"").decode()
