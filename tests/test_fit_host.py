"""Letterboxed frames on the host (no GPU): the functions the device kernels call (csrc/yf_images_fit.h), compiled for the host
(csrc/yf_images_host.c), against the restatements -- the fit against `ptq.letterbox_fit`, the frames bit for bit against
`ptq.letterbox_u8`, the decodes against the numpy float32 statement of fit_support.py -- and, for square pictures, against what exists:
the plain resize, the plain decodes and the oracle.  The geometry test stands on the definition alone."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT
from fit_support import (DECODE_SIDES, PADS, SMALL_SHAPES, YUV_SHAPES, decode_f32_restated, decode_int8_restated, expect_frame_fit,
                         fit_host, fit_scales, halves, host_decode_f32, host_decode_int8, host_fit, host_frame_packed, host_frame_yuv,
                         in_format, real_rgb, seeded_rgb, seeded_surface, surface_rgb)
from float_support import special_logits
from images_support import PKG, expect_frame, images, ptq, synthetic_heads, synthetic_heads160          # noqa: F401 (fixtures)
from images_yuv_support import lay_out

FRAMES = [(56, False), (56, True), (160, False)]            # (S, fp16 frames)


# ---- the fit ----
def test_fit_equals_the_restatement(ptq):
    rng = np.random.default_rng(56160)
    pairs = [(h, w) for h in range(1, 65) for w in range(1, 65)]
    pairs += [(int(h), int(w)) for h, w in rng.integers(1, 16385, (2000, 2))]
    pairs += [(1, 16384), (16384, 1), (16384, 16384), (16384, 16383), (16383, 16384)]
    for S in (56, 160):
        for h, w in pairs:
            want = ptq.letterbox_fit(h, w, S)
            assert host_fit(h, w, S) == want, (h, w, S)
            x0, y0, fw, fh = want
            assert 1 <= fw <= S and 1 <= fh <= S and max(fw, fh) == S
            assert x0 == (S - fw) // 2 and y0 == (S - fh) // 2 and x0 + fw <= S and y0 + fh <= S
    # the exact halves: 1080 * 56 / 1920 = 31.5 rounds up
    assert host_fit(1080, 1920, 56) == (0, 12, 56, 32) and host_fit(1920, 1080, 56) == (12, 0, 32, 56)
    assert host_fit(7, 16, 56) == (0, 15, 56, 25)                       # 24.5: half up, where Python's round gives 24
    assert host_fit(1, 16384, 56) == (0, 27, 56, 1) and host_fit(16384, 1, 160) == (79, 0, 1, 160)
    for S in (56, 160):
        for side in (1, 2, 55, 56, 57, 300, 16384):
            assert host_fit(side, side, S) == (0, 0, S, S)


def test_public_fit_entry_checks_and_agrees(images, ptq):
    for h, w, S in [(1080, 1920, 56), (1920, 1080, 160), (1, 1, 56), (16384, 3, 160)]:
        assert images.fit_of(h, w, S) == ptq.letterbox_fit(h, w, S)
    lib = images.load()
    out = np.zeros(4, np.int32)
    for h, w, S, word in [(0, 5, 56, "height and width"), (5, 16385, 56, "height and width"), (5, 5, 57, "out_hw")]:
        assert lib.yf_images_fit(h, w, S, out.ctypes.data) == -1 and word in (lib.yf_images_last_error_text() or b"").decode()
    assert lib.yf_images_fit(5, 5, 56, None) == -1 and "fit is NULL" in (lib.yf_images_last_error_text() or b"").decode()
    with pytest.raises(images.ImagesError, match="height and width"):
        images.fit_of(0, 1, 56)


# ---- frames ----
def _check_packed(rgb, fmts, pads, stride_pad=0):
    for fmt in fmts:
        img = in_format(rgb, fmt)
        rs = img.shape[1] * img.shape[2] + stride_pad if stride_pad else None
        for S, f16 in FRAMES:
            for pad in pads:
                st, frame = host_frame_packed(img, fmt, S, pad, f16, row_stride=rs)
                assert st == 0
                assert np.array_equal(frame, expect_frame_fit(rgb, S, pad, f16)), (rgb.shape, fmt, S, f16, pad)


def test_host_frames_equal_letterbox_u8_on_the_small_shapes():
    for h, w in SMALL_SHAPES:
        _check_packed(seeded_rgb(h, w), range(4), PADS)
    _check_packed(seeded_rgb(57, 56), range(4), PADS, stride_pad=13)         # a row stride with bytes that are no pixels


def test_host_frames_equal_letterbox_u8_on_the_reference_sizes():
    for k, rgb in enumerate(real_rgb()):
        _check_packed(rgb, range(4), PADS)


def test_host_frames_of_square_pictures_equal_the_plain_resize(ptq):
    for side in (1, 2, 56, 57, 160, 300):
        rgb = seeded_rgb(side, side)
        for fmt in range(4):
            img = in_format(rgb, fmt)
            for S, f16 in FRAMES:
                st, frame = host_frame_packed(img, fmt, S, 114, f16)
                plain = expect_frame(ptq, img, fmt, S)
                want = halves()[(plain.astype(np.int16) + 128).astype(np.uint8)] if f16 else plain
                assert st == 0 and np.array_equal(frame, want), (side, fmt, S, f16)


def test_host_yuv_frames_equal_letterbox_u8_of_the_converted_surface():
    surfaces = [seeded_surface(h, w) for h, w in YUV_SHAPES]
    buf, desc = lay_out(surfaces)                                 # pitches w + 3 and w + 6: odd chroma strides, nothing aligned
    for (y, uv), d in zip(surfaces, desc):
        for v_first in (False, True):
            rgb = surface_rgb(y, uv, v_first)
            for S, f16 in FRAMES:
                for pad in PADS:
                    st, frame = host_frame_yuv(buf, d, v_first, S, pad, f16)
                    assert st == 0
                    assert np.array_equal(frame, expect_frame_fit(rgb, S, pad, f16)), (y.shape, v_first, S, f16, pad)
    # an odd chroma stride (and an odd luma stride), the UV plane before the Y plane
    (y, uv), (h, w) = seeded_surface(58, 56), (58, 56)
    sy, suv = w + 1, w + 5
    buf = np.full(3 + (h // 2) * suv + 2 + h * sy, 0x5B, np.uint8)
    off_uv, off_y = 3, 3 + (h // 2) * suv + 2
    np.lib.stride_tricks.as_strided(buf[off_uv:], shape=(h // 2, w), strides=(suv, 1))[:] = uv
    np.lib.stride_tricks.as_strided(buf[off_y:], shape=(h, w), strides=(sy, 1))[:] = y
    d = np.zeros(1, desc.dtype)
    d[0] = (off_y, off_uv, h, w, sy, suv)
    for v_first in (False, True):
        for S, f16 in FRAMES:
            st, frame = host_frame_yuv(buf, d[0], v_first, S, 114, f16)
            assert st == 0 and np.array_equal(frame, expect_frame_fit(surface_rgb(y, uv, v_first), S, 114, f16)), (v_first, S, f16)


def test_host_refuses_invalid_descriptors_without_reading():
    lib = fit_host()
    from fit_support import YfImage, YfImageYuv
    for S, f16 in FRAMES:
        frame = np.full((S, S, 3), 0x1111 if f16 else 17, np.uint16 if f16 else np.int8)
        for im in (YfImage(0, 0, 5, 15), YfImage(0, 5, 5, 14), YfImage(1, 4, 4, 12), YfImage(2 ** 63, 1, 1, 3)):
            assert lib.yfi_prepare_fit_host(None, 48, 1, ctypes.byref(im), S, 114, int(f16), frame.ctypes.data) == 1        # base NULL: never read
            assert (frame == (0 if f16 else -128)).all()
        for im in (YfImageYuv(0, 16, 3, 4, 4, 4), YfImageYuv(0, 16, 4, 4, 4, 3), YfImageYuv(0, 17, 4, 4, 4, 4)):
            assert lib.yfi_prepare_fit_yuv_host(None, 24, ctypes.byref(im), 0, S, 114, int(f16), frame.ctypes.data) == 1
            assert (frame == (0 if f16 else -128)).all()
    im, frame = YfImage(0, 1, 1, 3), np.zeros((56, 56, 3), np.int8)
    px = np.zeros(3, np.uint8)
    for fmt, S, pad, f16 in [(4, 56, 114, 0), (0, 57, 114, 0), (0, 160, 114, 1), (0, 56, -1, 0), (0, 56, 256, 0)]:
        assert lib.yfi_prepare_fit_host(px.ctypes.data, 3, fmt, ctypes.byref(im), S, pad, f16, frame.ctypes.data) == -1


# ---- decodes ----
def test_host_int8_decode_equals_the_restatement_and_the_oracle(oracle, yf):
    rng = np.random.default_rng(2026)
    for S, heads in ((56, synthetic_heads(rng, 66)), (160, synthetic_heads160(rng, 12))):
        cap_all = 3 * (S // 8) ** 2
        for f, head in enumerate(heads):
            h, w = DECODE_SIDES[f % len(DECODE_SIDES)]
            want = decode_int8_restated(head, f, h, w, S, oracle.sig, oracle.ex)
            count, got = host_decode_int8(head, f, h, w, S, cap_all)
            assert count == want.shape[0] and got.tobytes() == want.tobytes(), (S, f, h, w)
            cap = max(1, count // 3)                                     # below the count: the first cap records, the true count
            count2, got2 = host_decode_int8(head, f, h, w, S, cap)
            assert count2 == count and got2.tobytes() == want[:cap].tobytes()
            if h == w:                                                   # the identity that ties the path to the oracle
                scale = float(np.float32(w / float(S)))
                ref = oracle.decode_py(head, f, w_scale=scale, h_scale=scale, max_dets=cap_all)
                assert [tuple(v.item() for v in r) for r in got] == ref, (S, f)
        assert any(h == w for h, w in DECODE_SIDES)
        # status 1 and sides out of range: no record
        for h, w, st in [(5, 5, 1), (0, 5, 0), (5, 16385, 0), (-1, -1, 0)]:
            assert host_decode_int8(heads[0], 0, h, w, S, 8, status=st)[0] == 0
    sq = host_decode_int8(heads[0], 3, 300, 300, 160, 1200)[1]
    buf = np.zeros(1200, yf.DET_DTYPE)
    n = fit_host().yfi_decode160_host(np.ascontiguousarray(heads[0]).ctypes.data, 3, float(np.float32(300 / 160.)), float(np.float32(300 / 160.)),
                                      buf.ctypes.data, 1200)
    assert n == sq.shape[0] and buf[:n].tobytes() == sq.tobytes()


def test_host_f32_decode_equals_the_restatement_and_the_plain_decode():
    logits = special_logits()                                            # NaN, +-inf, huge tw and th, the threshold's neighbours
    logits[0, 3, 3, 2], logits[0, 3, 3, 4] = 88.0, 5.0                   # a firing candidate whose width overflows the int32 range
    lib = fit_host()
    fired = 0
    for f, t in enumerate(logits):
        h, w = DECODE_SIDES[f % len(DECODE_SIDES)]
        want = decode_f32_restated(t, f, h, w)
        count, got = host_decode_f32(t, f, h, w, 147)
        assert count == want.shape[0] and got.tobytes() == want.tobytes(), (f, h, w)
        fired += count
        if count > 1:
            assert host_decode_f32(t, f, h, w, count - 1)[1].tobytes() == want[:count - 1].tobytes()
        if h == w:
            plain = np.frombuffer(bytes(28 * 147), got.dtype).copy()
            scale = float(np.float32(w / 56.))
            n = lib.yfi_decode_f32_host(np.ascontiguousarray(t).ctypes.data, f, scale, scale, plain.ctypes.data, 147)
            assert n == count and plain[:n].tobytes() == got.tobytes(), f
    assert fired > 500
    assert host_decode_f32(logits[0], 0, 5, 5, 8, status=1)[0] == 0 and host_decode_f32(logits[0], 0, 0, 5, 8)[0] == 0


def test_box_centres_map_back_to_the_picture_centre():
    """Independent of the restatement: one firing candidate at cell (3, 3) of a 7x7 grid with tx = ty = tw = th = 0 has its centre at
    (3 + 0.5) * 8 = 28, the centre of the 56 frame, so its box must be centred on the picture: (x1 + x2) / 2 within x_scale / 2 + 1 of
    W / 2 -- half a frame pixel for the odd pixel of padding (x0 is a floor) plus the truncation of two edges (each below 1, halved:
    below 1 together) -- and the same in y."""
    for h, w in [(1080, 1920), (1920, 1080), (362, 410), (56, 57)]:
        t = np.full((7, 7, 18), -20.0, np.float32)
        t[3, 3, 6:12] = [0, 0, 0, 0, 8.0, 0]                             # anchor 1 fires
        count, got = host_decode_f32(t, 0, h, w, 147)
        assert count == 1 and (got["anchor"][0], got["row"][0], got["col"][0]) == (1, 3, 3)
        _, _, xs, ys = fit_scales(h, w, 56)
        cx, cy = (int(got["x1"][0]) + int(got["x2"][0])) / 2, (int(got["y1"][0]) + int(got["y2"][0])) / 2
        assert abs(cx - w / 2) <= float(xs) / 2 + 1, (h, w, cx)
        assert abs(cy - h / 2) <= float(ys) / 2 + 1, (h, w, cy)
        # and the box has the anchor's shape in the picture: 12 x 17 frame pixels through the two scales, within the two truncations
        assert abs((int(got["x2"][0]) - int(got["x1"][0])) - 12 * float(xs)) <= 1 and abs((int(got["y2"][0]) - int(got["y1"][0])) - 17 * float(ys)) <= 1


# ---- argument checks ----
def _check(what, yuv=0, f16=0, a=0x10000, fmt=0, images=0x20000, n=3, out_hw=56, pad=114, frames=0x30000, status=0x40000, counts=0x50000, cap=8):
    text = ctypes.create_string_buffer(256)
    rc = fit_host().yfi_fit_check_host(what, yuv, f16, a, fmt, images, n, out_hw, pad, frames, status, counts, cap, text, 256)
    assert rc == (1 if text.value else 0)
    return text.value.decode()


def test_every_refusal_has_a_text():
    assert _check(0) == "" and _check(0, yuv=1, fmt=4) == "" and _check(0, f16=1) == "" and _check(0, out_hw=160) == ""
    prepare = [(dict(fmt=4), "NV12"), (dict(fmt=9), "format must be"), (dict(fmt=-1), "format must be"), (dict(yuv=1, fmt=0), "packed pixels"),
               (dict(yuv=1, fmt=6), "YF_PIX_NV12 or YF_PIX_NV21"), (dict(out_hw=57), "56 or 160"), (dict(f16=1, out_hw=160), "fp16 frames"),
               (dict(pad=-1), "pad must be"), (dict(pad=256), "pad must be"), (dict(n=-1), "n < 0"), (dict(frames=None), "d_frames"),
               (dict(frames=0x30008), "d_frames"), (dict(a=None), "d_pixels"), (dict(images=None), "d_images"), (dict(images=0x20004), "d_images"),
               (dict(status=None), "d_status"), (dict(status=0x40002), "d_status")]
    for kw, word in prepare:
        assert word in _check(0, **kw), (kw, _check(0, **kw))
    assert _check(0, n=0, a=None, images=None, status=None) == ""        # an empty batch needs no pixels
    assert _check(1) == "" and _check(1, out_hw=160, cap=1200) == "" and _check(1, f16=1, cap=147) == "" and _check(1, status=None) == ""
    decode = [(dict(out_hw=112), "56 or 160"), (dict(f16=1, out_hw=160), "float32 logits"), (dict(n=-1), "n < 0"), (dict(a=None), "d_heads is NULL"),
              (dict(f16=1, a=None), "d_logits is NULL"), (dict(f16=1, a=0x10002), "d_logits is not 4-byte"),
              (dict(out_hw=160, a=0x10008), "d_heads is not 16-byte"), (dict(frames=None), "d_dets is NULL"), (dict(counts=None), "d_counts is NULL"),
              (dict(frames=0x30002), "d_dets is not 4-byte"), (dict(counts=0x50001), "d_counts is not 4-byte"), (dict(cap=0), "[1, 147]"),
              (dict(cap=148), "[1, 147]"), (dict(out_hw=160, cap=1201), "[1, 1200]"), (dict(out_hw=160, cap=0), "[1, 1200]"),
              (dict(images=None), "d_images"), (dict(images=0x20004), "d_images"), (dict(status=0x40001), "d_status")]
    for kw, word in decode:
        assert word in _check(1, **kw), (kw, _check(1, **kw))
    assert _check(1, n=0, images=None) == ""


def test_entry_points_refuse_before_any_launch(images):
    """the nine entries of libyf_images.so with pointers that are never dereferenced: each refusal returns 0 (yf_images_fit: -1) with the
    text of the shared check, and an empty batch returns 0 after the checks"""
    lib = images.load()
    P, F, H, D, C, I, S, NET = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000
    err = lambda: (lib.yf_images_last_error_text() or b"").decode()
    prep = {"prepare_fit_ragged_device": lambda fmt=0, pad=114, n=2, out=56, fr=F: lib.yf_images_prepare_fit_ragged_device(P, 100, fmt, I, n, out, pad, fr, S, None),
            "prepare_fit_yuv_ragged_device": lambda fmt=4, pad=114, n=2, out=56, fr=F: lib.yf_images_prepare_fit_yuv_ragged_device(P, 100, fmt, I, n, out, pad, fr, S, None),
            "prepare_fit_f16_ragged_device": lambda fmt=0, pad=114, n=2, out=56, fr=F: lib.yf_images_prepare_fit_f16_ragged_device(P, 100, fmt, I, n, pad, fr, S, None),
            "prepare_fit_yuv_f16_ragged_device": lambda fmt=4, pad=114, n=2, out=56, fr=F: lib.yf_images_prepare_fit_yuv_f16_ragged_device(P, 100, fmt, I, n, pad, fr, S, None)}
    for name, fn in prep.items():
        yuv = "yuv" in name
        for kw, word in [(dict(fmt=0 if yuv else 4), "go through"), (dict(fmt=17), "format must be"), (dict(pad=256), "pad must be"),
                         (dict(pad=-1), "pad must be"), (dict(n=-1), "n < 0"), (dict(fr=F + 4), "d_frames")]:
            assert fn(**kw) == 0 and word in err(), (name, kw, err())
        if "f16" not in name:
            assert fn(out=100) == 0 and "56 or 160" in err()
        assert fn(n=0) == 0
    dec = lambda out=56, cap=8, n=2, st=S, heads=H: lib.yf_images_decode_fit_ragged_device(heads, I, st, n, out, D, C, cap, None)
    dec32 = lambda cap=8, n=2, st=S, heads=H: lib.yf_images_decode_f32_fit_ragged_device(heads, I, st, n, D, C, cap, None)
    for fn, cases in ((dec, [(dict(out=57), "56 or 160"), (dict(cap=148), "[1, 147]"), (dict(out=160, cap=1201), "[1, 1200]"), (dict(cap=0), "cap must"),
                             (dict(n=-1), "n < 0"), (dict(st=S + 1), "d_status"), (dict(heads=None), "d_heads"), (dict(out=160, heads=H + 8), "16-byte")]),
                      (dec32, [(dict(cap=148), "[1, 147]"), (dict(cap=0), "cap must"), (dict(n=-1), "n < 0"), (dict(st=S + 2), "d_status"),
                               (dict(heads=None), "d_logits"), (dict(heads=H + 2), "d_logits")])):
        for kw, word in cases:
            assert fn(**kw) == 0 and word in err(), (kw, err())
        assert fn(n=0) == 0 and fn(n=0, st=None) == 0
    run = lambda net=NET, fmt=0, out=56, pad=114, cap=8, n=2: lib.yf_images_run_decode_fit_ragged_device(net, P, 100, fmt, I, n, out, pad, F, H, D, C, cap, S, None)
    run16 = lambda net=NET, fmt=0, pad=114, cap=8, n=2: lib.yf_images_run_decode_fit_f16_ragged_device(net, P, 100, fmt, I, n, pad, F, H, D, C, cap, S, None)
    for fn in (run, run16):
        for kw, word in [(dict(net=None), "handle"), (dict(fmt=4), "go through"), (dict(pad=300), "pad must be"), (dict(cap=148), "[1, 147]"), (dict(n=-1), "n < 0")]:
            assert fn(**kw) == 0 and word in err(), (kw, err())
    assert run(out=160, cap=1201) == 0 and "[1, 1200]" in err()
    assert run(out=64) == 0 and "56 or 160" in err()


def test_fit_keyword_is_checked_before_anything_else(images):
    img = [np.zeros((8, 8, 3), np.uint8)]
    for call in (images.detect, images.detect_redacted, images.detect_blurred, images.detect_drawn, images.detect_chips):
        with pytest.raises(ValueError, match="'stretch'"):
            call(None, img, fit="pad")
    with pytest.raises(ValueError, match="'stretch'"):
        images.detect_tiled(None, img, 160, fit="LETTERBOX")
    with pytest.raises(ValueError, match="'stretch'"):
        images.evaluate(None, img, [np.zeros((0, 4))], fit=None)
    assert images.detect(None, [], fit="letterbox") == []


def test_the_new_sources_are_part_of_the_build_id(images):
    for src in ("yf_images_fit.h", "yf_images_fit.hip.h"):
        assert src in images._images_srcs() and os.path.exists(os.path.join(PKG, "csrc", src))
    lib = images.load()
    assert (lib.yf_images_build_id() or b"").decode() == images.expected_build_id()
    header = open(os.path.join(ROOT, "include", "yf_images.h")).read()
    for name in ("yf_images_fit", "yf_images_prepare_fit_ragged_device", "yf_images_prepare_fit_yuv_ragged_device",
                 "yf_images_prepare_fit_f16_ragged_device", "yf_images_prepare_fit_yuv_f16_ragged_device", "yf_images_decode_fit_ragged_device",
                 "yf_images_decode_f32_fit_ragged_device", "yf_images_run_decode_fit_ragged_device", "yf_images_run_decode_fit_f16_ragged_device"):
        assert hasattr(lib, name) and name + "(" in header, name
