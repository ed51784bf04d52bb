"""``cvsd_amd.crops``: the rectangle a box becomes (``crop_rects``: save_one_box's steps in float32) by known answers worked out by
hand, what ``crops=`` accepts (``CropSpec`` / ``as_spec``), and how ``Results`` carries crops.  Pure numpy and torch on the CPU, no GPU."""
import numpy as np
import pytest

from cvsd_amd.crops import CropSpec, as_spec, crop_rects


def one(box, shape=(100, 200), **kw):
    return crop_rects(np.array([box], np.float32), shape, **kw)[0].tolist()


def test_a_box_inside_the_frame():
    # centre (60, 45), size 40 x 30 -> 40 * 1.02 + 10 = 50.8, 30 * 1.02 + 10 = 40.6 -> corners 34.6, 24.7, 85.4, 65.3 -> truncated
    assert one((40, 30, 80, 60)) == [34, 24, 85, 65]
    # gain 1, pad 0: the box itself, truncated toward zero
    assert one((40.9, 30.2, 80.7, 60.99), gain=1.0, pad=0) == [40, 30, 80, 60]
    r = crop_rects(np.zeros((0, 4), np.float32), (10, 10))
    assert r.shape == (0, 4) and r.dtype == np.int32


def test_overhang_truncates_toward_zero_before_the_clip():
    # left / top: centre (5, 4), size 20.2 x 18.16 -> x1 = -5.1 -> -5 (toward zero, not -6) -> 0; y1 = -5.08 -> -5 -> 0
    assert one((0, 0, 10, 8)) == [0, 0, 15, 13]
    # -0.6 truncates to 0, which a floor would make -1: with a frame that allowed it the two would differ, here both clip to 0
    assert one((-0.6 + 0.0, 10, 19.4, 20), gain=1.0, pad=0) == [0, 10, 19, 20]
    # right / bottom: centre (195, 96), size 20.2 x 18.16 -> x2 = 205.1 -> 205 -> 200; y2 = 105.08 -> 105 -> 100
    assert one((190, 92, 200, 100)) == [184, 86, 200, 100]
    # every edge at once
    assert one((-50, -50, 400, 300)) == [0, 0, 200, 100]


def test_square():
    # 40 x 30 -> 40 x 40 -> 50.8 x 50.8 -> 34.6, 19.6, 85.4, 70.4
    assert one((40, 30, 80, 60), square=True) == [34, 19, 85, 70]
    assert one((40, 30, 70, 70), square=True) == one((35, 30, 75, 70))          # 30 x 40 and 40 x 40 around the same centre


def test_a_box_wholly_outside_is_empty():
    for box in [(300, 10, 340, 50), (-90, 10, -50, 50), (10, 150, 50, 190), (10, -80, 50, -40)]:
        x1, y1, x2, y2 = one(box)
        assert x2 <= x1 or y2 <= y1, box
        assert 0 <= x1 <= 200 and 0 <= x2 <= 200 and 0 <= y1 <= 100 and 0 <= y2 <= 100
    assert one((300, 10, 340, 50)) == [200, 4, 200, 55]


def test_float32_where_it_differs_from_float64():
    # 2^24 + 1 is not a float32: the box's corner becomes 16777216 before any step
    big = crop_rects(np.array([[0, 0, 16777217, 10]], np.float64), (20, 1 << 25), gain=1.0, pad=0)[0].tolist()
    assert big == [0, 0, 16777216, 10]
    # both corners ARE float32 values.  In exact arithmetic (and in float64) x2 = cx + (w * 1.02 + 10) / 2 = 1033.99999939, which
    # truncates to 1033; float32 has 6.1e-5 between neighbours at 1034, so every step's result is rounded and the sum lands on 1034.0
    x1, x2 = 787.2140502929688, 1026.6060791015625
    assert float(np.float32(x1)) == x1 and float(np.float32(x2)) == x2
    exact = (x1 + x2) / 2 + ((x2 - x1) * 1.02 + 10) / 2
    assert 1033.9999 < exact < 1034 and int(exact) == 1033
    assert one((x1, 10, x2, 40), shape=(2000, 2000)) == [779, 4, 1034, 45]


def test_spec():
    assert as_spec(None) is None and as_spec(False) is None
    assert as_spec(True) == CropSpec() and CropSpec().size is None and CropSpec().gain == 1.02 and CropSpec().pad == 10
    s = as_spec({"size": [256, 128], "fit": "pad", "fill": 0})
    assert s == CropSpec(size=(256, 128), fit="pad", fill=0) and as_spec(s) is s and s.size == (256, 128)
    for bad in [dict(fit="cover"), dict(size=(0, 4)), dict(size=(4,)), dict(size=(2.5, 4)), dict(fill=256), dict(source="plot"), dict(out="torch")]:
        with pytest.raises(ValueError):
            CropSpec(**bad)
    with pytest.raises(TypeError):
        as_spec("yes")


def test_results_keep_crops_aligned_with_boxes(tmp_path):
    import torch
    from cvsd_amd import Results
    boxes = torch.tensor([[0, 0, 4, 4, 0.9, 0], [1, 1, 5, 5, 0.8, 0], [2, 2, 6, 6, 0.7, 0]], dtype=torch.float32)
    r = Results(np.zeros((8, 8, 3), np.uint8), "x.jpg", {0: "person"}, boxes=boxes)
    assert r.crops is None and r.crop_jpegs is None and r[1].crops is None and r.numpy().crops is None
    r.crops = [np.full((1, 1, 3), k, np.uint8) for k in range(3)]
    r.crop_jpegs = [b"a", None, b"c"]
    assert [int(c[0, 0, 0]) for c in r[1].crops] == [1] and r[1].crop_jpegs == [None]
    assert [int(c[0, 0, 0]) for c in r[1:].crops] == [1, 2] and r[np.array([2, 0])].crop_jpegs == [b"c", b"a"]
    assert [int(c[0, 0, 0]) for c in r[torch.tensor([True, False, True])].crops] == [0, 2]
    assert r.numpy().crops is r.crops and r.numpy().crop_jpegs is r.crop_jpegs
    r.crops = torch.arange(3, dtype=torch.uint8).reshape(3, 1, 1, 1).expand(3, 2, 2, 3)
    assert r[2].crops.shape == (1, 2, 2, 3) and int(r[2].crops[0, 0, 0, 0]) == 2 and r[np.array([2, 0])].crops[:, 0, 0, 0].tolist() == [2, 0]
    # save_crop writes the streams it holds, one file per non-empty crop, numbered the way increment_path numbers them
    paths = r.save_crop(tmp_path, file_name="p")
    assert [p.split("/")[-2:] for p in paths] == [["person", "p.jpg"], ["person", "p2.jpg"]]
    assert [open(p, "rb").read() for p in paths] == [b"a", b"c"]
    assert [p.split("/")[-1] for p in r[:1].save_crop(tmp_path, file_name="p")] == ["p3.jpg"]
