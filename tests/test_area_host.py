"""Area-averaged frames on the host (no GPU): the functions the device kernels call (csrc/yf_images_area.h), compiled for the host
(csrc/yf_images_host.c), bit for bit against `ptq.resize_area_u8` / `ptq.letterbox_u8(..., interp="area")`, and both against a
brute-force statement written here that is a copy of neither: the picture is spread over the grid of (H * out) x (W * out) cells -- every
source pixel a rectangle of out x out cells -- and an output pixel is the sum of the H x W cells of its own rectangle; v = (2 S + H W)
// (2 H W).  The properties stand on the definition alone.

The reason for the feature, as the issue states it, is a 448 x 448 checkerboard of one-pixel squares: under the area average it is a
constant frame of int8 0 (127.5 rounds up to 128), whatever its phase.  The issue also expects the LINEAR frame of that picture not to be
constant and to change with a one-pixel shift; that expectation is arithmetically wrong for this picture and is not asserted: at an even
integer ratio (448 / 56 = 8) INTER_LINEAR's sample point falls exactly between two source pixels on either axis (f = 8 d + 3.5), so it
averages a 2 x 2 block, which on one-pixel squares is 127.5 everywhere too.  What the issue means to show is shown on the 392 x 392 board
(7x, an odd ratio: the linear sample falls ON a pixel): the linear frame is a checkerboard of -128 and 127 that inverts under the
one-pixel shift, the area frame stays within 3 of 127.5 and moves by at most 5."""
import ctypes

import numpy as np
import pytest

from area_support import (LETTERBOX, STRETCH, area_host, as_frame, checkerboard, expect_frame_area, expect_u8, host_area_packed, host_area_yuv,
                          host_linear_frame, host_weight)
from fit_support import YfImage, in_format, seeded_rgb, seeded_surface, surface_rgb
from images_support import ptq          # noqa: F401 (fixture)
from images_yuv_support import lay_out

FRAMES = [(56, False), (56, True), (160, False)]            # (S, fp16 frames)


def brute_force(rgb, out_h, out_w):
    """every source pixel's rectangle and every output pixel's rectangle on the (H * out_h) x (W * out_w) grid, the shared cells added up"""
    h, w = rgb.shape[:2]
    cells = np.repeat(np.repeat(rgb.astype(np.int64), out_h, axis=0), out_w, axis=1)       # pixel (sy, sx) fills out_h x out_w cells
    total = cells.reshape(out_h, h, out_w, w, -1).sum(axis=(1, 3))                          # output (y, x) owns h x w cells
    return ((2 * total + h * w) // (2 * h * w)).astype(np.uint8)


def test_host_equals_the_restatement_and_the_brute_force_for_every_small_size(ptq):
    for h in range(1, 25):
        for w in range(1, 25):
            rgb = seeded_rgb(h, w)
            want = brute_force(rgb, 56, 56)
            assert np.array_equal(ptq.resize_area_u8(rgb, 56, 56), want), (h, w)
            fmt = (h + w) % 4
            st, frame = host_area_packed(in_format(rgb, fmt), fmt, 56)
            assert st == 0 and np.array_equal(frame, as_frame(want)), (h, w, fmt)


def test_host_equals_the_restatement_and_the_brute_force_on_a_sample_at_160(ptq):
    for h, w in [(1, 1), (2, 2), (1, 24), (24, 1), (3, 5), (7, 13), (13, 7), (11, 9)]:           # grids of up to 3840 x 2080 cells
        rgb = seeded_rgb(h, w)
        want = brute_force(rgb, 160, 160)
        assert np.array_equal(ptq.resize_area_u8(rgb, 160, 160), want), (h, w)
        for fmt in range(4):
            st, frame = host_area_packed(in_format(rgb, fmt), fmt, 160)
            assert st == 0 and np.array_equal(frame, as_frame(want)), (h, w, fmt)


def test_other_shapes_formats_and_frame_types(ptq):
    """the GPU test's sizes on the host: every format, both sizes, both elements, a row stride with slack"""
    for h, w in [(1, 7), (7, 1), (55, 57), (56, 56), (57, 57), (112, 112), (113, 111), (167, 300)]:
        rgb = seeded_rgb(h, w)
        for fmt in range(4):
            img = in_format(rgb, fmt)
            for S, f16 in FRAMES:
                for fit in (STRETCH, LETTERBOX):
                    st, frame = host_area_packed(img, fmt, S, fit, 93, f16, row_stride=img.shape[1] * img.shape[2] + 5)
                    assert st == 0 and np.array_equal(frame, expect_frame_area(rgb, S, fit, 93, f16)), (h, w, fmt, S, f16, fit)
    rgb = seeded_rgb(113, 111)
    assert np.array_equal(expect_u8(rgb, 56), brute_force(rgb, 56, 56))
    x0, y0, fw, fh = ptq.letterbox_fit(167, 300, 56)
    assert np.array_equal(expect_u8(seeded_rgb(167, 300), 56, LETTERBOX, 93)[y0:y0 + fh, x0:x0 + fw], brute_force(seeded_rgb(167, 300), fh, fw))


# ---- properties ----
@pytest.mark.parametrize("n_out", [56, 160])
def test_the_weights_of_every_output_index_sum_to_n_in(n_out):
    lib = area_host()
    lib.yfi_area_axis_host.restype = ctypes.c_int
    lib.yfi_area_axis_host.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    firsts, lasts, sums = np.zeros(n_out, np.int32), np.zeros(n_out, np.int32), np.zeros(n_out, np.int64)
    for n_in in list(range(1, 8193)) + [16383, 16384]:
        assert lib.yfi_area_axis_host(n_in, n_out, firsts.ctypes.data, lasts.ctypes.data, sums.ctypes.data) == 0, n_in
        assert (sums == n_in).all(), n_in
        assert firsts[0] == 0 and lasts[-1] == n_in - 1 and (firsts <= lasts).all(), n_in
        step = firsts[1:] - lasts[:-1]                      # neighbouring outputs share at most one source, and skip none
        assert ((step == 0) | (step == 1)).all(), n_in
    # the weight itself, against the overlap of the two intervals in Python integers
    rng = np.random.default_rng(160)
    for n_in in (1, 2, 55, 56, 57, 100, 8192, 16384):
        for d, s in zip(rng.integers(0, n_out, 200), rng.integers(0, n_in, 200)):
            d, s = int(d), int(s)
            want = max(0, min((d + 1) * n_in, (s + 1) * n_out) - max(d * n_in, s * n_out))
            assert host_weight(d, s, n_in, n_out)[0] == want and 0 <= want <= min(n_in, n_out)


def test_a_constant_picture_gives_a_constant_frame():
    for h, w in [(1, 1), (3, 5), (57, 55), (300, 167), (1080, 1920)]:
        for value in (0, 1, 127, 128, 254, 255):
            img = np.full((h, w, 3), value, np.uint8)
            for S, f16 in FRAMES:
                st, frame = host_area_packed(img, 1, S, STRETCH, 0, f16)
                assert st == 0 and np.array_equal(frame, as_frame(np.full((S, S, 3), value, np.uint8), f16)), (h, w, value, S, f16)


def test_equal_sizes_are_the_identity_and_integer_ratios_the_rounded_block_mean(ptq):
    for S in (56, 160):
        rgb = seeded_rgb(S, S)
        st, frame = host_area_packed(rgb, 1, S)
        assert st == 0 and np.array_equal(frame, as_frame(rgb))
        for k in (2, 3, 5, 8):
            rgb = seeded_rgb(S * k, S * k)
            total = rgb.astype(np.int64).reshape(S, k, S, k, 3).sum(axis=(1, 3))
            mean = ((2 * total + k * k) // (2 * k * k)).astype(np.uint8)          # half up
            st, frame = host_area_packed(rgb, 1, S)
            assert st == 0 and np.array_equal(frame, as_frame(mean)), (S, k)
            assert np.array_equal(ptq.resize_area_u8(rgb, S, S), mean)


def test_at_exactly_2x_the_bytes_equal_the_linear_prepare():
    for S in (56, 160):
        rgb = seeded_rgb(2 * S, 2 * S)
        for fmt in range(4):
            img = in_format(rgb, fmt)
            st, frame = host_area_packed(img, fmt, S)
            assert st == 0 and np.array_equal(frame, host_linear_frame(img, fmt, S)), (S, fmt)
        total = rgb.astype(np.int64).reshape(S, 2, S, 2, 3).sum(axis=(1, 3))
        assert np.array_equal(frame, as_frame(((total + 2) >> 2).astype(np.uint8)))


def test_a_checkerboard_of_one_pixel_squares_is_a_constant_frame_whatever_its_phase():
    """the issue's picture; what is and is not asserted of the linear frame: the module's docstring"""
    board, shifted = checkerboard(448), checkerboard(448, 1)
    assert not np.array_equal(board, shifted) and set(np.unique(board)) == {0, 255}
    for f16 in (False, True):                                     # at 56: 8 x 8 blocks, 32 pixels of either colour
        st, frame = host_area_packed(board, 1, 56, STRETCH, 0, f16)
        assert st == 0 and np.array_equal(frame, as_frame(np.full((56, 56, 3), 128, np.uint8), f16)), f16      # int8 0: 127.5 rounds up
        st, moved = host_area_packed(shifted, 1, 56, STRETCH, 0, f16)
        assert st == 0 and np.array_equal(moved, frame)
    # the contrast with the linear resize, at the ratio where its sample falls on a pixel
    board, shifted = checkerboard(392), checkerboard(392, 1)
    linear, linear_moved = host_linear_frame(board, 1, 56), host_linear_frame(shifted, 1, 56)
    assert set(np.unique(linear)) == {-128, 127} and len(np.unique(linear[0, :, 0])) == 2          # not constant: the board, aliased
    assert (np.abs(linear.astype(np.int16) - linear_moved) == 255).all()                           # one pixel of shift inverts every byte
    _, area = host_area_packed(board, 1, 56)
    _, area_moved = host_area_packed(shifted, 1, 56)
    assert np.abs(area.astype(np.int16) + 128 - 127.5).max() <= 3                                  # 24 or 25 of 49 pixels white
    assert np.abs(area.astype(np.int16) - area_moved).max() <= 5


def test_the_row_sum_bound_pictures_of_16384_by_3_all_white():
    for h, w in [(16384, 3), (3, 16384)]:
        img = np.full((h, w, 3), 255, np.uint8)
        for S, f16 in FRAMES:
            st, frame = host_area_packed(img, 0, S, STRETCH, 0, f16)
            assert st == 0 and np.array_equal(frame, as_frame(np.full((S, S, 3), 255, np.uint8), f16)), (h, w, S, f16)     # int8: all 127


# ---- letterbox ----
def test_letterbox_of_a_square_picture_is_the_stretch_and_1920x1080_equals_the_restatement(ptq):
    for side in (1, 57, 300):
        rgb = seeded_rgb(side, side)
        for S, f16 in FRAMES:
            a, b = host_area_packed(rgb, 1, S, STRETCH, 7, f16), host_area_packed(rgb, 1, S, LETTERBOX, 200, f16)
            assert a[0] == 0 and b[0] == 0 and np.array_equal(a[1], b[1]), (side, S, f16)
    rgb = seeded_rgb(1080, 1920)
    for fmt, S, f16, pad in [(0, 56, False, 114), (3, 56, True, 0), (1, 160, False, 255)]:
        want = ptq.letterbox_u8(rgb, S, pad, interp="area")
        x0, y0, fw, fh = ptq.letterbox_fit(1080, 1920, S)
        assert (want[:y0] == pad).all() and (want[y0 + fh:] == pad).all() and np.array_equal(want[y0:y0 + fh], ptq.resize_area_u8(rgb, fh, fw))
        st, frame = host_area_packed(in_format(rgb, fmt), fmt, S, LETTERBOX, pad, f16)
        assert st == 0 and np.array_equal(frame, as_frame(want, f16)), (fmt, S, f16)
    assert np.array_equal(ptq.letterbox_u8(rgb, 56, 114), ptq.letterbox_u8(rgb, 56, 114, interp="linear"))      # the default has not moved
    with pytest.raises(ValueError, match="interp"):
        ptq.letterbox_u8(rgb, 56, 114, interp="cubic")


# ---- NV12 / NV21 ----
def test_yuv_surfaces_are_converted_pixel_by_pixel_and_then_averaged():
    shapes = [(2, 2), (2, 400), (400, 2), (58, 56), (56, 58), (112, 112), (362, 410)]
    surfaces = [seeded_surface(h, w) for h, w in shapes]
    buf, desc = lay_out(surfaces)                                 # pitches w + 3 and w + 6, planes in either order, nothing aligned
    for (y, uv), d in zip(surfaces, desc):
        for v_first in (False, True):
            rgb = surface_rgb(y, uv, v_first)                     # ptq.yuv420sp_to_rgb_u8
            for S, f16 in FRAMES:
                for fit in (STRETCH, LETTERBOX):
                    st, frame = host_area_yuv(buf, d, v_first, S, fit, 114, f16)
                    assert st == 0 and np.array_equal(frame, expect_frame_area(rgb, S, fit, 114, f16)), (y.shape, v_first, S, f16, fit)


# ---- descriptors and arguments ----
def test_invalid_descriptors_and_arguments():
    lib = area_host()
    rgb = seeded_rgb(7, 9)
    buf = np.ascontiguousarray(rgb).reshape(-1)
    for im in (YfImage(1, 7, 9, 27), YfImage(0, 8, 9, 27), YfImage(0, 7, 9, 26), YfImage(0, 0, 9, 27), YfImage(0, 7, 16385, 27),
               YfImage(2 ** 63, 7, 9, 27), YfImage(0, 7, 9, -27)):
        for S, f16 in FRAMES:
            frame = np.full((S, S, 3), 0x1111 if f16 else 17, np.uint16 if f16 else np.int8)
            st = lib.yfi_prepare_area_host(buf.ctypes.data, buf.nbytes, 1, ctypes.byref(im), S, 0, 114, int(f16), frame.ctypes.data)
            assert st == 1 and (frame == (0 if f16 else -128)).all()
    frame = np.zeros((160, 160, 3), np.uint16)
    im = YfImage(0, 7, 9, 27)
    for fmt, S, fit, pad, f16 in [(4, 56, 0, 0, 0), (7, 56, 0, 0, 0), (1, 57, 0, 0, 0), (1, 160, 0, 0, 1), (1, 56, 2, 0, 0), (1, 56, -1, 0, 0),
                                  (1, 56, 1, 256, 0), (1, 56, 0, -1, 0)]:
        assert lib.yfi_prepare_area_host(buf.ctypes.data, buf.nbytes, fmt, ctypes.byref(im), S, fit, pad, f16, frame.ctypes.data) == -1
    text = ctypes.create_string_buffer(256)
    ok = dict(yuv=0, f16=0, pixels=64, fmt=1, images=64, n=1, S=56, fit=0, pad=114, frames=64, status=64)

    def check(**kw):
        a = dict(ok, **kw)
        r = lib.yfi_area_check_host(a["yuv"], a["f16"], a["pixels"], a["fmt"], a["images"], a["n"], a["S"], a["fit"], a["pad"], a["frames"],
                                    a["status"], text, 256)
        return r, text.value.decode()

    assert check() == (0, "")
    assert check(n=0, pixels=None, images=None, status=None) == (0, "")
    for kw, word in [(dict(fmt=4), "prepare_area_yuv"), (dict(fmt=9), "format must be"), (dict(yuv=1), "prepare_area_ragged"),
                     (dict(yuv=1, fmt=9), "YF_PIX_NV12 or"), (dict(S=57), "56 or 160"), (dict(f16=1, S=160), "fp16 frames"),
                     (dict(fit=2), "fit must be"), (dict(pad=256), "pad"), (dict(pad=-1), "pad"), (dict(n=-1), "n < 0"),
                     (dict(frames=None), "d_frames"), (dict(frames=72), "d_frames"), (dict(pixels=None), "d_pixels"),
                     (dict(images=68), "d_images"), (dict(status=66), "d_status"), (dict(status=None), "d_status")]:
        r, t = check(**kw)
        assert r == 1 and word in t, (kw, t)
    assert check(fit=2, pad=300)[1].startswith("fit")             # the order is part of the behaviour


def test_the_band_policy():
    lib = area_host()
    lib.yfi_area_band_row_host.restype = ctypes.c_int
    lib.yfi_area_band_row_host.argtypes = [ctypes.c_int] * 3
    for S in (56, 160):
        assert lib.yfi_area_bands_host(1, S) == S // 2 and lib.yfi_area_bands_host(2048, S) == 1 and lib.yfi_area_bands_host(10 ** 9, S) == 1
        assert lib.yfi_area_bands_host(16, S) == S // 2                       # sixteen 4K frames: 448 / 1280 jobs for 256 CUs
        for n in (1, 2, 3, 16, 37, 100, 1000, 2047, 2048, 5000):
            bands = lib.yfi_area_bands_host(n, S)
            assert 1 <= bands <= S // 2 and (bands == S // 2 or n * bands >= 2048)
            rows = [lib.yfi_area_band_row_host(b, bands, S) for b in range(bands + 1)]
            assert rows[0] == 0 and rows[-1] == S and all(b > a and (b - a) % 2 == 0 for a, b in zip(rows, rows[1:])), (n, S, rows)
