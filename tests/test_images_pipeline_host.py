"""The pipeline layer of images.py without a GPU (`detect`, `detect_tiled`, `detect_chips`, `detect_redacted`, `detect_tracked`, `evaluate`
with network=None): the arguments each call refuses before a picture is packed or the library is loaded, with the texts it refuses them
in; what each returns for an empty batch; the names and codes that `order`, `mode` and `layout` take; and that a tiled call packs its
pixels once before it reaches the device."""
import types

import numpy as np
import pytest

from images_support import images          # noqa: F401 (fixture)

IMG = [np.zeros((8, 8, 3), np.uint8)]
TRACKER = types.SimpleNamespace(streams=2)


@pytest.fixture
def no_staging(images, monkeypatch):
    """packing a picture or loading the library from here on fails the test: the refusals come first"""
    def reached(*args, **kwargs):
        raise AssertionError("the call went on to pack the pictures or to load the library")
    for name in ("pack_images", "pack_yuv_images", "load"):
        monkeypatch.setattr(images, name, reached)
    return images


def test_detect_chips_refusals(no_staging):
    images = no_staging
    for kw, text in ((dict(margin=1.5), r"margin 1\.5: 0 to 1"), (dict(margin=-0.1), r"margin -0\.1: 0 to 1"),
                     (dict(order="yuv"), "order 'yuv': 'rgb' or 'bgr'"), (dict(out=(16.5, 16)), r"out \(16\.5, 16\): an integer or \(y, x\) integers")):
        with pytest.raises(ValueError, match=text):
            images.detect_chips(None, IMG, **kw)


def test_detect_redacted_refusals(no_staging):
    images = no_staging
    for kw, text in ((dict(mode="blur"), "mode 'blur': 'mosaic' or 'fill'"), (dict(block=5), "block 5: 4, 8, 16, 32 or 64"),
                     (dict(colour=(0, 0, 256)), r"colour \(0, 0, 256\): three bytes"), (dict(colour=0x1000000), "colour 16777216: 0x00RRGGBB"),
                     (dict(margin=2), "margin 2: 0 to 1")):
        with pytest.raises(ValueError, match=text):
            images.detect_redacted(None, IMG, **kw)


def test_detect_tracked_refusals(no_staging):
    images = no_staging
    with pytest.raises(ValueError, match="1 images: 2 streams x 1 steps"):
        images.detect_tracked(None, IMG, TRACKER, 1)
    with pytest.raises(ValueError, match="2 images: 2 streams x -1 steps"):
        images.detect_tracked(None, IMG * 2, TRACKER, -1)
    with pytest.raises(ValueError, match="iou_threshold None: the tracker takes suppressed records"):
        images.detect_tracked(None, IMG * 2, TRACKER, 1, iou_threshold=None)
    with pytest.raises(ValueError, match=r"layout 'space': 'time' \(frame t \* streams \+ s\) or 'stream' \(frame s \* steps \+ t\)"):
        images.detect_tracked(None, IMG * 2, TRACKER, 1, layout="space")


def test_evaluate_and_detect_refusals(no_staging):
    images = no_staging
    with pytest.raises(ValueError, match="1 images, 0 lists of ground truths"):
        images.evaluate(None, IMG, [])
    with pytest.raises(ValueError, match="1 images, 2 lists of ground truths"):
        images.evaluate(None, IMG, [np.zeros((0, 4))] * 2)
    with pytest.raises(ValueError, match="dtype 'fp32': 'int8' or 'fp16'"):
        images.detect(None, IMG, dtype="fp32")
    with pytest.raises(ValueError, match="dtype 'fp16': the fp16 network has 56x56 frames only"):
        images.detect(None, IMG, dtype="fp16", size=160)
    with pytest.raises(ValueError, match="size 112: 56 or 160"):
        images.detect(None, [], size=112)                                 # ... and before the empty batch is returned


def test_empty_batches(no_staging):
    images = no_staging
    assert images.detect(None, []) == []
    assert images.detect_tiled(None, [], 160) == []
    assert images.detect_chips(None, []) == ([], [], [])
    assert images.detect_redacted(None, []) == ([], [])
    assert images.detect_tracked(None, [], TRACKER, 0) == []
    assert images.evaluate(None, [], []) == {"ap": 0.0, "detections": 0, "ground_truths": 0, "true_positives": 0, "precision": 0.0, "recall": 0.0}


def test_names_and_codes_of_order_mode_and_layout(no_staging):
    """each table's names in any letter case and its integer codes pass (an empty batch comes back); another string and a bool do not.
    `order=True` used to pass as RGB, the only one of the three checks that let a bool through."""
    images = no_staging
    chips = lambda v: images.detect_chips(None, [], order=v)
    redacted = lambda v: images.detect_redacted(None, [], mode=v)
    tracked = lambda v: images.detect_tracked(None, [], TRACKER, 0, layout=v)
    for call, table, empty, text in ((chips, images.ORDERS, ([], [], []), "order {!r}: 'rgb' or 'bgr'"),
                                     (redacted, images.REDACT_MODES, ([], []), "mode {!r}: 'mosaic' or 'fill'"),
                                     (tracked, images.TRACK_LAYOUTS, [], "layout {!r}: 'time' (frame t * streams + s) or 'stream' (frame s * steps + t)")):
        assert sorted(table.values()) == [0, 1]
        for name, code in table.items():
            for v in (name, name.upper(), name.capitalize(), code, np.int32(code)):
                assert call(v) == empty, v
        for v in ("", "other", next(iter(table)) + " ", 2, -1, None, True, False):
            with pytest.raises(ValueError) as e:
                call(v)
            assert str(e.value) == text.format(v), v


def test_a_tiled_call_packs_its_pixels_once_before_the_device(images, monkeypatch):
    """as far as the host goes: with no network the call ends where the device or the network is first needed, after the tiles are planned
    (tests/test_images_pipeline_gpu.py counts the packs of a whole call)"""
    packs, plans = [], []
    pack_images, plan_tiles = images.pack_images, images.plan_tiles
    monkeypatch.setattr(images, "pack_images", lambda *a, **k: packs.append(1) or pack_images(*a, **k))
    monkeypatch.setattr(images, "plan_tiles", lambda *a, **k: plans.append(1) or plan_tiles(*a, **k))
    picture = [np.zeros((40, 56, 3), np.uint8)]
    for call in (lambda: images.detect_tiled(None, picture, 32, device=0), lambda: images.detect_chips(None, picture, tile=32, device=0),
                 lambda: images.detect_redacted(None, picture, tile=32, device=0),
                 lambda: images.evaluate(None, picture, [np.zeros((0, 4))], tile=32, device=0)):
        del packs[:], plans[:]
        with pytest.raises(Exception):
            call()
        assert (len(packs), len(plans)) == (1, 1)
