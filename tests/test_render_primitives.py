"""``cvsd_amd.render.primitives`` on hand-made ``Results``: which records a result turns into (pure numpy, no GPU), and
``Results.plot`` / ``rendered`` as far as they can be checked without one."""
import numpy as np
import pytest
import torch

from cvsd_amd import RenderSpec, Results
from cvsd_amd import render as RD

NAMES = {0: "person", 1: "bicycle"}


def _result(boxes, kpts=None, shape=(240, 320), img=False):
    boxes = torch.tensor(boxes, dtype=torch.float32).reshape(-1, len(boxes[0]) if boxes else 6)
    kp = None if kpts is None else torch.tensor(np.asarray(kpts, np.float32))
    return Results(np.zeros((*shape, 3), np.uint8) if img else None, "x.jpg", NAMES, boxes=boxes, keypoints=kp, orig_shape=shape)


def _pose(conf=0.9):
    """17 joints on a diagonal, all with confidence `conf`"""
    k = np.zeros((17, 3), np.float32)
    k[:, 0] = 50 + 5 * np.arange(17)
    k[:, 1] = 40 + 7 * np.arange(17)
    k[:, 2] = conf
    return k


def _of(p, t):
    return p[p[:, 0] == t]


def test_line_width_rule():
    assert RD.line_width(240, 320) == 2                       # 280 * 0.003 = 0.84 -> 1 -> at least 2
    assert RD.line_width(1080, 1920) == 4                     # 1500 * 0.003 = 4.5 -> Python's round: 4
    assert RD.line_width(2160, 3840) == 9
    p = RD.primitives(_result([[10, 20, 110, 220, 0.9, 0]], shape=(1080, 1920)))
    assert _of(p, RD.RECT)[0].tolist() == [RD.RECT, 10, 20, 110, 220, 4, RD.PALETTE[0], 0]
    p = RD.primitives(_result([[10, 20, 110, 220, 0.9, 0]]), RenderSpec(line_width=7))
    assert _of(p, RD.RECT)[0, 5] == 7


def test_limbs_need_both_joints_and_joints_their_own_confidence():
    k = _pose()
    r = _result([[40, 30, 150, 170, 0.8, 0]], [k])
    p = RD.primitives(r)
    assert len(_of(p, RD.LINE)) == 19 and len(_of(p, RD.DISC)) == 17
    first = _of(p, RD.LINE)[0]                                # limb (15, 13), thickness = line width, the box's colour
    assert first.tolist() == [RD.LINE, 50 + 75, 40 + 105, 50 + 65, 40 + 91, 2, RD.PALETTE[0], 0]
    assert _of(p, RD.DISC)[3].tolist() == [RD.DISC, 65, 61, 0, 0, 2, RD.WHITE, 0]
    k2 = k.copy()
    k2[5, 2] = 0.49                                           # the left shoulder drops out: its four limbs go, one joint goes
    p = RD.primitives(_result([[40, 30, 150, 170, 0.8, 0]], [k2]))
    assert len(_of(p, RD.LINE)) == 19 - sum(5 in l for l in RD.SKELETON) == 15 and len(_of(p, RD.DISC)) == 16
    k2[5, 2] = 0.5                                            # the threshold itself is drawn
    assert len(_of(RD.primitives(_result([[40, 30, 150, 170, 0.8, 0]], [k2])), RD.LINE)) == 19
    p = RD.primitives(_result([[40, 30, 150, 170, 0.8, 0]], [k]), RenderSpec(kpt_conf=0.95))
    assert not len(_of(p, RD.LINE)) and not len(_of(p, RD.DISC))
    p = RD.primitives(_result([[40, 30, 150, 170, 0.8, 0]], [k]), RenderSpec(skeleton=False, kpt_radius=4))
    assert not len(_of(p, RD.LINE)) and not len(_of(p, RD.DISC))
    assert _of(RD.primitives(r, RenderSpec(kpt_radius=4)), RD.DISC)[0, 5] == 4


def test_head_box_from_five_two_and_one_joints():
    box = [100.0, 50.0, 200.0, 350.0, 0.9, 0.0]
    k = _pose(0.0)
    k[:5] = [[150, 80, 0.9], [156, 76, 0.9], [144, 76, 0.9], [164, 80, 0.9], [136, 80, 0.9]]
    # five joints: x in [136, 164], y in [76, 80]: larger side 28 -> a square of side 56 (>= a quarter of the box's width, 25) around (150, 78)
    assert RD.head_box(k, box, 0.5) == (122.0, 50.0, 178.0, 106.0)
    p = RD.primitives(_result([box], [k]), RenderSpec(anonymize="head", mosaic=8))
    assert _of(p, RD.MOSAIC)[0].tolist() == [RD.MOSAIC, 122, 50, 178, 106, 8, 0, 0]
    k[2:5, 2] = 0.1                                           # two joints: nose and one eye, 6 x 4 -> the minimum side, 25
    assert RD.head_box(k, box, 0.5) == (153 - 12.5, 78 - 12.5, 153 + 12.5, 78 + 12.5)
    k[1, 2] = 0.1                                             # one joint: the top quarter of the box
    assert RD.head_box(k, box, 0.5) == (100.0, 50.0, 200.0, 125.0)
    p = RD.primitives(_result([box], [k]), RenderSpec(anonymize="head"))
    assert _of(p, RD.MOSAIC)[0].tolist() == [RD.MOSAIC, 100, 50, 200, 125, 16, 0, 0]
    assert p[0, 0] == RD.MOSAIC                               # a box's mosaic precedes its outline


def test_detect_model_falls_back_to_the_top_quarter_and_box_mode_takes_the_box():
    r = _result([[10.4, 20.6, 110.5, 220.49, 0.9, 0]])
    assert _of(RD.primitives(r, RenderSpec(anonymize="head")), RD.MOSAIC)[0].tolist() == [RD.MOSAIC, 10, 21, 111, 71, 16, 0, 0]
    assert _of(RD.primitives(r, RenderSpec(anonymize="box", mosaic=32)), RD.MOSAIC)[0].tolist() == [RD.MOSAIC, 10, 21, 111, 220, 32, 0, 0]
    assert not len(_of(RD.primitives(r), RD.MOSAIC)) and not len(_of(RD.primitives(r), RD.LINE))


def _text(p):
    return "".join(chr(c) for c in _of(p, RD.GLYPH)[:, 3])


def test_label_text_for_ids_and_scores():
    assert RD.label_text(12, 0.8749) == "#12 0.87" and RD.label_text(None, 0.5) == "0.50" and RD.label_text(3.0, 1.0) == "#3 1.00"
    tracked = _result([[40, 60, 150, 170, 12, 0.874, 0]])
    p = RD.primitives(tracked)
    assert _text(p) == "#120.87"                              # the space advances the pen and draws nothing
    g = _of(p, RD.GLYPH)
    # scale 1 (line width 2): background 9 rows high above the box, glyphs one pixel inside it, 6 pixels apart
    fill = _of(p, RD.FILL)[0]
    assert fill.tolist() == [RD.FILL, 40, 51, 40 + 8 * 6 - 1 + 2 - 1, 59, 0, RD.PALETTE[12], 0]
    assert g[:, 1].tolist() == [41 + 6 * i for i in (0, 1, 2, 4, 5, 6, 7)] and set(g[:, 2]) == {52} and set(g[:, 6]) == {RD.WHITE}
    assert _text(RD.primitives(_result([[40, 60, 150, 170, 0.874, 1]]))) == "0.87"
    top = RD.primitives(_result([[40, 3, 150, 170, 7, 0.5, 0]]))   # no room above: the label moves inside the box's top edge
    assert _of(top, RD.FILL)[0, 2] == 3
    assert not len(_of(RD.primitives(tracked, RenderSpec(labels=False)), RD.GLYPH)) and not len(_of(RD.primitives(tracked, RenderSpec(labels=False)), RD.FILL))
    assert not len(_of(RD.primitives(tracked, RenderSpec(boxes=False)), RD.RECT))
    for ch in _text(p) + " ":
        assert ch in RD.FONT_CHARS


def test_colour_by_id_and_by_class():
    r = _result([[0, 0, 9, 9, 3, 0.9, 1], [20, 20, 29, 29, 23, 0.9, 0]])
    by_id = _of(RD.primitives(r), RD.RECT)[:, 6].tolist()
    assert by_id == [RD.PALETTE[3], RD.PALETTE[23 % len(RD.PALETTE)]] and len(RD.PALETTE) == 20
    assert _of(RD.primitives(r, RenderSpec(color_by="class")), RD.RECT)[:, 6].tolist() == [RD.PALETTE[1], RD.PALETTE[0]]
    untracked = _result([[0, 0, 9, 9, 0.9, 1]])               # no ids: the class decides either way
    assert _of(RD.primitives(untracked), RD.RECT)[0, 6] == RD.PALETTE[1]


def test_no_boxes_no_primitives():
    for r in (_result([]), Results(None, "x.jpg", NAMES, boxes=torch.zeros((0, 7)), keypoints=torch.zeros((0, 17, 3)), orig_shape=(48, 64))):
        p = RD.primitives(r, RenderSpec(anonymize="head"))
        assert p.shape == (0, 8) and p.dtype == np.int32


def test_three_hundred_people_fit_the_limit():
    n = 300
    boxes = [[i, i, i + 50, i + 90, 1000 + i, 0.875, 0] for i in range(n)]
    p = RD.primitives(_result(boxes, [_pose()] * n, shape=(1080, 1920)), RenderSpec(anonymize="head"))
    assert len(p) == n * (1 + 1 + 19 + 17 + 1 + len("#1000 0.88") - 1) <= RD.MAX_PRIMS


def test_spec_is_validated():
    for bad in (dict(anonymize="face"), dict(mosaic=5), dict(color_by="track"), dict(line_width=0), dict(kpt_radius=-1)):
        with pytest.raises(ValueError):
            RenderSpec(**bad)
    with pytest.raises(TypeError):
        RD.as_spec("yes")
    assert RD.as_spec(None) is None and RD.as_spec(False) is None and RD.as_spec(True) == RenderSpec()
    assert RD.as_spec({"anonymize": "box"}).anonymize == "box"


def test_coordinates_are_rounded_and_kept_in_range():
    assert [RD._px(v) for v in (0.49, 0.5, -0.5, -0.51, 1e9, -1e9, float("nan"))] == [0, 1, 0, -1, 1 << 20, -(1 << 20), 0]


def test_plot_without_an_image_asks_for_render_at_call_time():
    r = _result([[1, 2, 30, 40, 0.9, 0]])
    assert r.rendered is None
    with pytest.raises(ValueError, match="render="):
        r.plot()
    with pytest.raises(TypeError):
        _result([[1, 2, 30, 40, 0.9, 0]], img=True).plot(colour="red")
    assert r[0].rendered is None and r.numpy().rendered is None
