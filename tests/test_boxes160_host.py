"""Boxes at 160x160 on the host (no GPU): the per-candidate decode of csrc/yf_images_decode160.h -- the function the device kernel calls,
compiled for the host -- against the oracle's yfo_decode_py on 20x20 heads, the wide order key of the suppression, the argument checks of
the five new entry points (which return before any launch) and the build-id coverage of the new sources."""
import os

import numpy as np
import pytest

from conftest import ROOT
from images_support import PKG, host, images, last_error          # noqa: F401 (host, images: fixtures)

NEW_ENTRIES = ("yf_images_decode160_device", "yf_images_decode160_ragged_device", "yf_images_run_decode160_device",
               "yf_images_run_decode160_ragged_device", "yf_images_nms_wide_device")
NEW_SOURCES = ("yf_images_decode160.h", "yf_images_wide.hip.h")
SCALES = [np.float32(1.0), np.float32(410 / 160.), np.float32(16384 / 160.), np.float32(1 / 160.)]


def _decode_host(yf, lib, head, frame, ws, hs, cap):
    hd = np.ascontiguousarray(head, np.int8)
    buf = np.zeros(cap, yf.DET_DTYPE)
    n = lib.yfi_decode160_host(hd.ctypes.data, frame, float(ws), float(hs), buf.ctypes.data, cap)
    return [tuple(v.item() for v in r) for r in buf[:min(n, cap)]], n


CORNERS = [(0, 0), (0, 19), (19, 0), (19, 19)]


def _walk_heads():
    """heads that walk all 256 byte values through each of the five used channels at the four corners of the grid (row / col 0 and 19): three
    values per head, one per anchor; only the corners fire"""
    heads = []
    for ch in range(5):
        for v0 in range(-128, 128, 3):
            h = np.full((20, 20, 18), -128, np.int16)
            for r, c in CORNERS:
                h[r, c, :] = 0
                h[r, c, 4::6] = 100
                for a in range(3):
                    h[r, c, a * 6 + ch] = min(v0 + a, 127)
            heads.append(h.astype(np.int8))
    return heads


def test_candidate_decode_equals_the_oracle_on_20x20_heads(yf, oracle, host):
    # the byte threshold the kernel compares against is the table's first entry above 0.7f
    q_thr = host.yfi_decode160_q_threshold_host()
    assert -128 < q_thr <= 127
    assert oracle.sig[q_thr + 128] > np.float32(0.7) and not oracle.sig[q_thr + 127] > np.float32(0.7)
    rng = np.random.default_rng(160)
    random_heads = [rng.integers(-128, 128, (20, 20, 18), dtype=np.int16).astype(np.int8) for _ in range(6)]
    walk = _walk_heads()
    seen = [set() for _ in range(5)]
    for k, head in enumerate(random_heads + walk):
        n = None
        for j, ws in enumerate(SCALES):
            hs = SCALES[(j + 1) % len(SCALES)]
            want = oracle.decode_py(head, k, w_scale=float(ws), h_scale=float(hs), max_dets=1200)
            got, n = _decode_host(yf, host, head, k, ws, hs, 1200)
            assert n == len(want), (k, ws)
            assert got == want, (k, ws)
        if k < len(random_heads):
            assert 500 < n < 760, n                                      # about half of the 1200 candidates fire on random bytes
            cap = n // 3                                                 # cap below the count: the first cap records, the true count
            got, n2 = _decode_host(yf, host, head, k, SCALES[1], SCALES[2], cap)
            assert n2 == n and len(got) == cap
            assert got == oracle.decode_py(head, k, w_scale=float(SCALES[1]), h_scale=float(SCALES[2]), max_dets=cap)
        else:
            assert {(r[2], r[3]) for r in got} <= set(CORNERS)
            for (_, a, r, c, *_rest) in got:
                for ch in range(5):
                    seen[ch].add(int(head[r, c, a * 6 + ch]))
    # every value of the four box channels went through a record; of the confidence channel, every value that fires
    assert all(seen[ch] == set(range(-128, 128)) for ch in range(4))
    assert seen[4] == set(range(q_thr, 128))


def test_wide_order_key_is_the_stable_descending_argsort(host):
    rng = np.random.default_rng(4)
    special = np.array([0.0, -0.0, 1.0, 1.0, np.inf, -np.inf, np.nan, -np.nan, 0.7000001, 1e-45, -1e-45, -3.0], np.float32)
    sizes = [1, 2, 63, 64, 65, 256, 257, 1199, 1200] + [int(rng.integers(1, 1201)) for _ in range(40)]
    for trial, k in enumerate(sizes):
        pool = np.concatenate([special, rng.choice(np.float32([0.71, 0.8, 0.9, 0.99, 1.0]), 8), rng.standard_normal(8).astype(np.float32)])
        conf = rng.choice(pool, k)
        keys = np.array([host.yfi_nms_key_wide_host(int(c), i) for i, c in enumerate(conf.view(np.uint32))], np.uint64)
        assert len(set(keys.tolist())) == k
        got = np.argsort(keys)[::-1]
        want = np.argsort(conf.astype(np.float64), kind="stable")[::-1]
        assert np.array_equal(got, want), (trial, k)
    # the same mapping of the conf bits as the 8-bit key
    for c in special.view(np.uint32):
        assert host.yfi_nms_key_wide_host(int(c), 0) >> 11 == host.yfi_nms_key_host(int(c), 0) >> 8


def test_new_entry_points_check_every_argument_before_any_launch(images):
    lib = images.load()
    P, F, H, D, C, I, S, NET = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000      # never dereferenced

    def dec(heads=H, n=4, dets=D, counts=C, cap=1200):
        return lib.yf_images_decode160_device(heads, n, 1.0, 1.0, dets, counts, cap, None), last_error(lib)

    def dec_r(heads=H, imgs=I, status=S, n=4, dets=D, counts=C, cap=1200):
        return lib.yf_images_decode160_ragged_device(heads, imgs, status, n, dets, counts, cap, None), last_error(lib)

    decode_cases = [(dict(n=-1), "n < 0"), (dict(heads=None), "d_heads is NULL"), (dict(heads=H + 8), "d_heads is not 16-byte"),
                    (dict(dets=None), "d_dets is NULL"), (dict(counts=None), "d_counts is NULL"), (dict(dets=D + 2), "d_dets is not 4-byte"),
                    (dict(counts=C + 1), "d_counts is not 4-byte"), (dict(cap=0), "cap must be"), (dict(cap=1201), "cap must be")]
    for fn in (dec, dec_r):
        texts = set()
        for kw, word in decode_cases:
            rc, text = fn(**kw)
            assert rc <= 0 and word in text, (fn.__name__, kw, rc, text)
            texts.add(text)
        assert len(texts) == 8                                # one text per kind of fault (cap 0 and cap 1201 are one kind)
        assert fn(n=0)[0] == 0
    for kw, word in [(dict(imgs=None), "d_images"), (dict(imgs=I + 4), "d_images"), (dict(status=S + 2), "d_status")]:
        rc, text = dec_r(**kw)
        assert rc <= 0 and word in text, (kw, rc, text)
    assert dec_r(status=None, n=0)[0] == 0                    # d_status may be NULL

    good = dict(net=NET, d_pixels=P, pixels_bytes=362 * 1230 * 4, format=0, height=362, width=410, row_stride=1230, frame_stride=362 * 1230,
                n=4, d_frames=F, heads=H, dets=D, counts=C, cap=1200)

    def run(**kw):
        a = dict(good, **kw)
        rc = lib.yf_images_run_decode160_device(a["net"], a["d_pixels"], a["pixels_bytes"], a["format"], a["height"], a["width"], a["row_stride"],
                                                a["frame_stride"], a["n"], a["d_frames"], a["heads"], a["dets"], a["counts"], a["cap"], None)
        return rc, last_error(lib)

    run_cases = [(dict(net=None), "handle"), (dict(format=4), "format"), (dict(n=-1), "n < 0"), (dict(d_frames=F + 4), "16-byte"),
                 (dict(d_frames=None), "d_frames"), (dict(height=0), "height and width"), (dict(width=16385, row_stride=16385 * 3), "height and width"),
                 (dict(row_stride=1229), "row_stride"), (dict(frame_stride=-1), "frame_stride < 0"), (dict(d_pixels=None), "d_pixels"),
                 (dict(pixels_bytes=1000), "first image"), (dict(pixels_bytes=362 * 1230 * 4 - 1), "last image"),
                 (dict(heads=None), "d_heads is NULL"), (dict(heads=H + 4), "d_heads is not 16-byte"), (dict(dets=None), "d_dets is NULL"),
                 (dict(counts=C + 2), "d_counts is not 4-byte"), (dict(cap=0), "cap must be"), (dict(cap=1201), "cap must be")]
    texts = set()
    for kw, word in run_cases:
        rc, text = run(**kw)
        assert rc <= 0 and word in text, (kw, rc, text)
        texts.add(text)
    assert len(texts) == 15
    assert run(n=0, d_pixels=None, pixels_bytes=0)[0] == 0

    def run_r(net=NET, d_pixels=P, fmt=0, imgs=I, n=3, d_frames=F, heads=H, dets=D, counts=C, cap=1200, status=S):
        rc = lib.yf_images_run_decode160_ragged_device(net, d_pixels, 100, fmt, imgs, n, d_frames, heads, dets, counts, cap, status, None)
        return rc, last_error(lib)
    for kw, word in [(dict(net=None), "handle"), (dict(fmt=7), "format"), (dict(n=-1), "n < 0"), (dict(d_frames=F + 8), "16-byte"),
                     (dict(imgs=None), "d_images"), (dict(status=None), "d_status"), (dict(d_pixels=None), "d_pixels"),
                     (dict(heads=H + 1), "d_heads is not 16-byte"), (dict(dets=D + 1), "d_dets is not 4-byte"), (dict(counts=None), "d_counts is NULL"),
                     (dict(cap=0), "cap must be"), (dict(cap=1201), "cap must be")]:
        rc, text = run_r(**kw)
        assert rc <= 0 and word in text, (kw, rc, text)
    assert run_r(n=0)[0] == 0

    goodn = dict(dets=D, counts=C, n=4, cap=1200, thr=0.4, out=P, out_counts=F)

    def nms(**kw):
        a = dict(goodn, **kw)
        rc = lib.yf_images_nms_wide_device(a["dets"], a["counts"], a["n"], a["cap"], a["thr"], a["out"], a["out_counts"], None)
        return rc, last_error(lib)
    cases = [(dict(n=-1), "n < 0"), (dict(cap=0), "cap must be"), (dict(cap=-3), "cap must be"), (dict(cap=images.NMS_WIDE_MAX_CAP + 1), "cap must be"),
             (dict(thr=float("nan")), "NaN"), (dict(dets=None), "d_dets is NULL"), (dict(counts=None), "d_counts is NULL"),
             (dict(out=None), "d_out is NULL"), (dict(out_counts=None), "d_out_counts is NULL"), (dict(dets=D + 2), "d_dets is not 4-byte"),
             (dict(out=P + 1), "d_out is not 4-byte"), (dict(counts=C + 2), "d_counts or d_out_counts"), (dict(out_counts=F + 3), "d_counts or d_out_counts")]
    texts = set()
    for kw, word in cases:
        rc, text = nms(**kw)
        assert rc <= 0 and word in text, (kw, rc, text)
        texts.add(text)
    assert len(texts) == 10
    assert images.NMS_WIDE_MAX_CAP == 1200 and images.NMS_MAX_CAP == 256
    for thr in (0.0, 0.4, 1.0, 1e300, -1.0, float("inf")):
        assert nms(n=0, thr=thr)[0] == 0
    assert nms(n=0, cap=images.NMS_WIDE_MAX_CAP)[0] == 0
    with pytest.raises(images.ImagesError, match="NaN"):
        images.nms_wide_device(D, C, 4, 1200, float("nan"))
    with pytest.raises(images.ImagesError, match="cap must be"):
        images.decode160_device(H, 4, D, C, 1201)


def test_detect_refuses_other_sizes(images):
    img = [np.zeros((8, 8, 3), np.uint8)]
    for size in (112, 0, 159, "160"):
        with pytest.raises(ValueError, match="56 or 160"):
            images.detect(None, img, size=size)                          # before the network or the GPU is touched


def test_the_new_sources_are_part_of_the_companion_library_only(images):
    flags = open(os.path.join(PKG, "csrc", "flags.mk")).read()
    for src in NEW_SOURCES:
        assert src in images._images_srcs() and src not in flags, src
        assert os.path.exists(os.path.join(PKG, "csrc", src))
    lib = images.load()
    assert (lib.yf_images_build_id() or b"").decode() == images.expected_build_id()
    ours = open(os.path.join(ROOT, "include", "yf_images.h")).read()
    theirs = open(os.path.join(ROOT, "include", "yf_network.h")).read()
    for name in NEW_ENTRIES:
        assert hasattr(lib, name), name
        assert name in ours and name not in theirs, name
    assert "is not offered" not in ours
