"""The pipeline layer of images.py on the MI355X: every `detect_*` call stages its batch as `detect` does, so the boxes that `detect_chips`
and `detect_redacted` report are the boxes of `detect`, and with a tile those of `detect_tiled`, array for array -- at both frame sizes,
int8 and fp16, packed pictures and NV12 surfaces.  Every comparison is exact.  What the chips and the redacted pictures hold is the subject
of tests/test_crops_gpu.py and tests/test_redact_gpu.py."""
import numpy as np
import pytest

from images_support import images_after_network, ptq, real_images, torch_cuda      # noqa: F401 (fixtures; `images` is images_after_network)
from images_yuv_support import bgr_to_nv12

pytestmark = pytest.mark.gpu

PICTURES = 3                                # the first of the 27 real images: every configuration below finds a box in them


@pytest.fixture(scope="module")
def fp16_network(network):
    network.fp16_init()
    return network


@pytest.fixture(scope="module")
def batches(ptq):
    """fmt -> the pictures: BGR as cv2.imread gives them, and the same pictures cropped to even sides as NV12 surfaces (y, uv)"""
    bgr = real_images(ptq)[:PICTURES]
    return {"bgr": bgr, "nv12": [bgr_to_nv12(img[:img.shape[0] & ~1, :img.shape[1] & ~1]) for img in bgr]}


def _same(got, want):
    return len(got) == len(want) and all(g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("fmt", ["bgr", "nv12"])
@pytest.mark.parametrize("size,dtype", [(56, "int8"), (160, "int8"), (56, "fp16")])
def test_chips_and_redaction_report_the_boxes_of_detect(fp16_network, torch_cuda, images, batches, size, dtype, fmt):
    pictures = batches[fmt]
    want = images.detect(fp16_network, pictures, fmt=fmt, iou_threshold=0.4, size=size, dtype=dtype)
    found = sum(w.shape[0] for w in want)
    print(f"{fmt} {size} {dtype}: {[w.shape[0] for w in want]} boxes")
    assert found >= 1, "detect reports no box: the comparison shows nothing"
    assert all(w.dtype == np.int32 and w.ndim == 2 and w.shape[1] == 4 for w in want)
    boxes, chips, info = images.detect_chips(fp16_network, pictures, out=16, fmt=fmt, size=size, dtype=dtype)
    assert _same(boxes, want)
    assert [c.shape for c in chips] == [(w.shape[0], 16, 16, 3) for w in want] and [i.shape for i in info] == [(w.shape[0],) for w in want]
    assert _same(images.detect_chips(fp16_network, pictures, out=16, fmt=fmt, size=size, dtype=dtype, chips_cap=found)[0], want)
    redacted, boxes = images.detect_redacted(fp16_network, pictures, mode="fill", fmt=fmt, size=size, dtype=dtype)
    assert _same(boxes, want) and len(redacted) == len(pictures)


def test_tiled_chips_and_redaction_report_the_boxes_of_detect_tiled(network, torch_cuda, images, batches, monkeypatch):
    """... and a tiled call copies its pictures into one buffer once: the parents' descriptors are those the tiles were planned on"""
    pictures = batches["bgr"]
    want = images.detect_tiled(network, pictures, 160, stride=120)
    print(f"tiled: {[w.shape[0] for w in want]} boxes")
    assert sum(w.shape[0] for w in want) >= 1, "detect_tiled reports no box: the comparison shows nothing"
    packs, pack_images = [], images.pack_images
    monkeypatch.setattr(images, "pack_images", lambda *a, **k: packs.append(1) or pack_images(*a, **k))
    assert _same(images.detect_chips(network, pictures, tile=160, stride=120, out=16)[0], want) and len(packs) == 1
    assert _same(images.detect_redacted(network, pictures, mode="fill", tile=160, stride=120)[1], want) and len(packs) == 2
    assert _same(images.detect_tiled(network, pictures, 160, stride=120), want) and len(packs) == 3
