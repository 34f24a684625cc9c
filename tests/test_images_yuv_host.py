"""The NV12 / NV21 path without a GPU: the host build of csrc/yf_images_yuv.h (the functions the kernels call) against
ptq.yuv420sp_to_rgb_u8 on every (Y, U, V) triple and against hand-derived triples, the descriptor check against a plain-Python statement,
the host prepare against the restated conversion under the existing BGR frame, pack_yuv_images, and the refusals that need no GPU."""
import ctypes

import numpy as np
import pytest

from images_support import images, last_error, ptq          # noqa: F401 (fixtures)
from images_yuv_support import SHAPES, all_surfaces, expected_frame, f16_table, host_frame, lay_out, restated_rgb, surface, yuv_host_lib

CY, CUB, CUG, CVG, CVR = 1220542, 2116026, -409993, -852492, 1673527


def test_every_triple_equals_the_restatement(ptq):
    """all 2^24 (Y, U, V): one 4096 x 4096 surface whose 2 x 2 block p = 2048 * i + j has U = p & 255, V = (p >> 8) & 255 and the four
    lumas 4 * (p >> 16) + 0..3"""
    p = (np.arange(2048, dtype=np.int64)[:, None] * 2048 + np.arange(2048, dtype=np.int64)[None, :])
    uv = np.stack([p & 255, (p >> 8) & 255], axis=-1).astype(np.uint8).reshape(2048, 4096)
    y4 = (4 * (p >> 16)).astype(np.uint8)
    y = np.repeat(np.repeat(y4, 2, axis=0), 2, axis=1)
    y[1::2, :] += 2
    y[:, 1::2] += 1
    u = np.repeat(np.repeat(uv[:, 0::2], 2, axis=0), 2, axis=1)
    v = np.repeat(np.repeat(uv[:, 1::2], 2, axis=0), 2, axis=1)
    triples = np.ascontiguousarray(np.stack([y, u, v], axis=-1).reshape(-1, 3))
    codes = triples[:, 0].astype(np.int64) << 16 | triples[:, 1].astype(np.int64) << 8 | triples[:, 2]
    assert np.array_equal(np.sort(codes), np.arange(1 << 24)), "the surface does not hold every triple once"
    got = np.empty_like(triples)
    yuv_host_lib().yfi_yuv_rgb_host(triples.ctypes.data, triples.shape[0], got.ctypes.data)
    assert np.array_equal(got.reshape(4096, 4096, 3), ptq.yuv420sp_to_rgb_u8(y, uv))
    # NV21 is the same function of the swapped pair
    vu = np.ascontiguousarray(uv.reshape(2048, 2048, 2)[..., ::-1]).reshape(2048, 4096)
    assert np.array_equal(got.reshape(4096, 4096, 3), ptq.yuv420sp_to_rgb_u8(y, vu, v_first=True))


# Each by hand, with h = 1 << 19 = 524288 and >> 20 a floor division by 1048576:
#   (16, 128, 128):  yy = 0, uu = vv = 0: every channel (0 + h) >> 20 = 0.
#   (235, 128, 128): yy = 219 * CY = 267298698; + h = 267822986; / 1048576 = 255.4 -> 255 on every channel.
#   (81, 90, 240):   yy = 65 * CY = 79335230, + h = 79859518; uu = -38, vv = 112.
#                    R: + CVR * 112 = 187435024 -> 267294542 -> 254.9 -> 254.
#                    G: + CVG * 112 = -95479104, + CUG * -38 = +15579734 -> -39852 -> floor -1 -> clamp 0.
#                    B: + CUB * -38 = -80408988 -> -549470 -> floor -1 -> clamp 0.
#   (255, 0, 0):     yy = 239 * CY = 291709538, + h = 292233826; uu = vv = -128.
#                    R: + CVR * -128 = -214211456 -> 78022370 -> 74.4 -> 74.
#                    G: + 109118976 + 52479104 -> 453831906 -> 432.8 -> clamp 255.
#                    B: + CUB * -128 = -270851328 -> 21382498 -> 20.4 -> 20.
#   (0, 255, 255):   yy = 0 (Y below 16), h = 524288; uu = vv = 127.
#                    R: + CVR * 127 = 212537929 -> 213062217 -> 203.2 -> 203.
#                    G: - 108266484 - 52069111 < 0 -> clamp 0.
#                    B: + CUB * 127 = 268735302 -> 269259590 -> 256.8 -> clamp 255.
PINNED = [((16, 128, 128), (0, 0, 0)), ((235, 128, 128), (255, 255, 255)), ((81, 90, 240), (254, 0, 0)), ((255, 0, 0), (74, 255, 20)),
          ((0, 255, 255), (203, 0, 255))]


def test_pinned_triples(ptq):
    yuv = np.array([t for t, _ in PINNED], np.uint8)
    got = np.empty_like(yuv)
    yuv_host_lib().yfi_yuv_rgb_host(yuv.ctypes.data, len(PINNED), got.ctypes.data)
    assert got.tolist() == [list(rgb) for _, rgb in PINNED]
    for (y, u, v), rgb in PINNED:
        plane_y, plane_uv = np.full((2, 2), y, np.uint8), np.array([[u, v]], np.uint8)
        assert (ptq.yuv420sp_to_rgb_u8(plane_y, plane_uv) == np.array(rgb, np.uint8)).all()
        assert (ptq.yuv420sp_to_rgb_u8(plane_y, plane_uv[:, ::-1], v_first=True) == np.array(rgb, np.uint8)).all()


def _ok_python(off_y, off_uv, h, w, sy, suv, nbytes):
    """the descriptor rule in unbounded integers"""
    if not (2 <= h <= 16384 and 2 <= w <= 16384 and h % 2 == 0 and w % 2 == 0):
        return 0
    if sy < w or suv < w:
        return 0
    return int(off_y + (h - 1) * sy + w <= nbytes and off_uv + (h // 2 - 1) * suv + w <= nbytes)


def test_descriptor_check_against_python():
    lib = yuv_host_lib()
    big = 1 << 63
    cases = []
    for h in (0, 1, 2, 3, 4, 16383, 16384, 16385, 16386, -2):
        for w in (0, 1, 2, 3, 10, 16384, 16386, -4):
            cases.append((0, 1 << 30, h, w, 20000, 20000, 1 << 40))
    h, w, sy, suv = 6, 10, 13, 16
    ext_y, ext_uv = (h - 1) * sy + w, (h // 2 - 1) * suv + w
    for off_y, off_uv in ((0, 100), (100, 0), (7, 7 + ext_y), (ext_uv + 1, 1)):
        need = max(off_y + ext_y, off_uv + ext_uv)
        for nbytes in (need - 1, need, need + 1, 0):
            cases.append((off_y, off_uv, h, w, sy, suv, nbytes))
    cases += [(0, 200, h, w, w - 1, suv, 1000), (0, 200, h, w, sy, w - 1, 1000), (0, 200, h, w, w, w, 1000), (0, 200, h, w, -13, suv, 1000),
              (0, 200, h, w, sy, -16, 1000), (0, 200, h, w, 0, 0, 1000)]
    # each plane alone one byte past the buffer
    cases += [(1000 - ext_y + 1, 0, h, w, sy, suv, 1000), (0, 1000 - ext_uv + 1, h, w, sy, suv, 1000),
              (1000 - ext_y, 0, h, w, sy, suv, 1000), (0, 1000 - ext_uv, h, w, sy, suv, 1000)]
    # offsets and strides near 2^63 and 2^64: the sums wrap in 64 bits, the rule does not
    m64 = (1 << 64) - 1
    for off in (big - 1, big, big + 1, m64, m64 - ext_y, m64 - ext_y + 1):
        for nbytes in (m64, big, 1000):
            cases += [(off, 0, h, w, sy, suv, nbytes), (0, off, h, w, sy, suv, nbytes)]
    for st in (big - 1, (big - 1) // 5, (big - 1) // 5 + 1, (m64 // 5), (1 << 62)):
        for nbytes in (m64, big, 1000):
            cases += [(0, 0, h, w, st, suv, nbytes), (0, 0, h, w, sy, st, nbytes), (3, 5, 16384, 16384, st, st, nbytes)]
    seen = set()
    for off_y, off_uv, hh, ww, a, b, nbytes in cases:
        got = lib.yfi_yuv_image_ok_host(off_y, off_uv, hh, ww, a, b, nbytes)
        want = _ok_python(off_y, off_uv, hh, ww, a, b, nbytes)
        assert got == want, (off_y, off_uv, hh, ww, a, b, nbytes, got, want)
        seen.add(want)
    assert seen == {0, 1}


@pytest.mark.parametrize("out", [56, 160])
def test_host_prepare_equals_the_restatement(out):
    """every shape, the random and the clamp picture, both chroma orders, in the padded layout with filler between the samples; the fp16
    frame at 56 is yfi_f16_of_u8 of the same bytes"""
    items = all_surfaces()
    buf, desc = lay_out([surface(k, c) for k, c in items])
    half = f16_table()
    for v_first in (False, True):
        for i, (k, c) in enumerate(items):
            st, frame = host_frame(buf, desc[i], v_first, out)
            assert st == 0
            assert np.array_equal(frame, expected_frame(k, c, v_first, out)), (SHAPES[k], c, v_first, out)
            if out == 56:
                st, frame = host_frame(buf, desc[i], v_first, 56, f16=True)
                assert st == 0 and np.array_equal(frame, half[restated_rgb(k, c, v_first, 56)]), (SHAPES[k], c, v_first)


def test_host_prepare_flags_invalid_descriptors():
    buf, desc = lay_out([surface(3, False)])
    d = desc[0].copy()
    d["height"] = 5
    st, frame = host_frame(buf, d, False, 56)
    assert st == 1 and (frame == -128).all()
    st, frame = host_frame(buf, d, False, 56, f16=True)
    assert st == 1 and (frame == 0).all()
    st, _ = host_frame(buf[:-1].copy(), desc[0], False, 56)
    assert st == 1
    assert host_frame(buf, desc[0], False, 57)[0] == -1 and host_frame(buf, desc[0], False, 160, f16=True)[0] == -1


def test_pack_yuv_images_layouts(images, ptq):
    rng = np.random.default_rng(4)
    y, uv = rng.integers(0, 256, (6, 10), dtype=np.uint8), rng.integers(0, 256, (3, 10), dtype=np.uint8)
    whole = np.concatenate([y, uv])                                            # cv2's layout
    parent_y, parent_uv = rng.integers(0, 256, (9, 17), dtype=np.uint8), rng.integers(0, 256, (5, 23), dtype=np.uint8)
    parent_y[1:7, 4:14], parent_uv[2:5, 6:16] = y, uv                          # pitched views
    arena = rng.integers(0, 256, 400, dtype=np.uint8)                          # a UV view that precedes its Y view in memory
    uv_first, y_after = arena[5:5 + 30].reshape(3, 10), arena[100:100 + 60].reshape(6, 10)
    uv_first[:], y_after[:] = uv, y
    assert uv_first.ctypes.data < y_after.ctypes.data
    fortran = (np.asfortranarray(y), np.asfortranarray(uv))                    # not along the rows: made contiguous
    buf, desc = images.pack_yuv_images([whole, (parent_y[1:7, 4:14], parent_uv[2:5, 6:16]), (y_after, uv_first), fortran, (y, uv)], "nv12")
    assert desc.dtype == images.YUV_IMAGE_DTYPE and desc.shape == (5,)
    assert desc["stride_y"].tolist() == [10, 17, 10, 10, 10] and desc["stride_uv"].tolist() == [10, 23, 10, 10, 10]
    assert (desc["offset_y"] % 16 == 0).all() and (desc["offset_uv"] % 16 == 0).all()
    want = ptq.yuv420sp_to_rgb_u8(y, uv)
    lib = yuv_host_lib()
    for d in desc:
        assert (d["height"], d["width"]) == (6, 10)
        assert lib.yfi_yuv_image_ok_host(int(d["offset_y"]), int(d["offset_uv"]), 6, 10, int(d["stride_y"]), int(d["stride_uv"]), buf.nbytes) == 1
        gy = np.lib.stride_tricks.as_strided(buf[int(d["offset_y"]):], (6, 10), (int(d["stride_y"]), 1))
        guv = np.lib.stride_tricks.as_strided(buf[int(d["offset_uv"]):], (3, 10), (int(d["stride_uv"]), 1))
        assert np.array_equal(ptq.yuv420sp_to_rgb_u8(gy, guv), want)
    # the planes end inside the buffer, and align=1 packs them back to back
    buf1, desc1 = images.pack_yuv_images([(y, uv)], "nv21", align=1)
    assert buf1.nbytes == 90 and desc1[0].tolist() == (0, 60, 6, 10, 10, 10)
    sizes = images.yuv_sizes(desc)
    assert sizes.dtype == images.IMAGE_DTYPE and sizes["height"].tolist() == [6] * 5 and sizes["width"].tolist() == [10] * 5


def test_pack_yuv_images_refusals(images):
    y, uv = np.zeros((6, 10), np.uint8), np.zeros((3, 10), np.uint8)
    bad = [
        (np.zeros((9, 9), np.uint8), "odd side"),                              # cv2's layout, odd width
        (np.zeros((10, 10), np.uint8), "H \\* 3 / 2"),                         # rows no multiple of 3
        ((np.zeros((5, 10), np.uint8), uv), "odd side"),
        ((y, np.zeros((3, 8), np.uint8)), "uv plane"),
        ((y.astype(np.int8), uv), "uint8"),
        ((y, uv.astype(np.uint16)), "uint8"),
        (np.zeros((9, 10), np.float32), "uint8"),
        ((y[::-1], uv), "negative strides"),
        ((y, uv[:, ::-1]), "negative strides"),
        ((y, uv, uv), "pair"),
        (np.zeros((9, 10, 1), np.uint8), "uint8 \\[H \\* 3 / 2, W\\]"),
    ]
    for img, text in bad:
        with pytest.raises(ValueError, match=text):
            images.pack_yuv_images([img], "nv12")
    with pytest.raises(ValueError, match="nv12"):
        images.pack_yuv_images([(y, uv)], "bgr")
    with pytest.raises(ValueError, match="outside 2\\.\\.16384"):
        images.pack_yuv_images([(np.zeros((2, 16386), np.uint8), np.zeros((1, 16386), np.uint8))], "nv12")
    with pytest.raises(ValueError, match="pack_yuv_images"):
        images.pack_images([np.zeros((4, 4, 3), np.uint8)], "nv12")


def test_existing_entries_name_the_new_ones(images):
    """the packed-pixel entries refuse YF_PIX_NV12 / YF_PIX_NV21 before any launch (no GPU needed) and say where such surfaces go"""
    lib = images.load()
    frames = ctypes.c_void_p(4096)
    for code in (images.YF_PIX_NV12, images.YF_PIX_NV21):
        assert lib.yf_images_prepare_device(None, 0, code, 4, 4, 12, 48, 1, 56, frames, None) == 0
        assert "yf_images_prepare_yuv_device" in last_error(lib) and "yf_images_prepare_yuv_f16_ragged_device" in last_error(lib)
        assert lib.yf_images_prepare_ragged_device(None, 0, code, None, 1, 56, frames, None, None) == 0
        assert "yf_images_prepare_yuv_ragged_device" in last_error(lib)
        assert lib.yf_images_prepare_f16_device(None, 0, code, 4, 4, 12, 48, 1, frames, None) == 0
        assert "yf_images_prepare_yuv_f16_device" in last_error(lib)
    # and the new ones refuse the packed formats, odd sides and short strides on the host, before any launch
    assert lib.yf_images_prepare_yuv_device(None, 0, images.YF_PIX_BGR8, 4, 4, 4, 16, 4, 24, 1, 56, frames, None) == 0
    assert "YF_PIX_NV12" in last_error(lib)
    for args, text in (((5, 4, 4, 20, 4, 28), "even"), ((4, 3, 4, 16, 4, 24), "even"), ((4, 4, 3, 16, 4, 24), "stride_y"),
                       ((4, 4, 4, 16, 3, 24), "stride_uv"), ((4, 4, 4, -1, 4, 24), "uv_offset"), ((0, 4, 4, 16, 4, 24), "16384"),
                       ((4, 16386, 16386, 16, 16386, 24), "16384")):
        assert lib.yf_images_prepare_yuv_device(frames, 1 << 20, images.YF_PIX_NV12, *args, 1, 56, frames, None) == 0
        assert text in last_error(lib), (args, last_error(lib))
    assert lib.yf_images_prepare_yuv_device(frames, 23, images.YF_PIX_NV12, 4, 4, 4, 16, 4, 24, 1, 56, frames, None) == 0
    assert "first surface" in last_error(lib)
    assert lib.yf_images_prepare_yuv_device(frames, 47, images.YF_PIX_NV12, 4, 4, 4, 16, 4, 24, 2, 56, frames, None) == 0
    assert "last surface" in last_error(lib)
    assert lib.yf_images_prepare_yuv_f16_device(frames, 48, images.YF_PIX_NV21, 4, 4, 4, 16, 4, 24, 0, frames, None) == 0       # n = 0: nothing


def test_tiling_refuses_the_new_formats(images):
    y = np.zeros((6, 4), np.uint8)
    for fmt in ("nv12", "nv21", images.YF_PIX_NV12):
        with pytest.raises(ValueError, match="not supported"):
            images.detect_tiled(None, [y], 8, fmt=fmt)
        with pytest.raises(ValueError, match="not supported"):
            images.evaluate(None, [y], [np.zeros((0, 4))], fmt=fmt, tile=8)
        with pytest.raises(ValueError, match="not supported"):
            images.plan_tiles([(4, 4)], fmt, 8)
