"""The evidence-frame rasteriser's host twin (``ops.render(..., device=-1)``: the routine of csrc/render_raster.h in host loops) against
the sequential numpy checker of tests/_render_numpy.py, bit for bit over the case table, plus known answers derived by hand.  No GPU is
touched."""
import ctypes as C

import numpy as np
import pytest

import _render_cases as K
import _render_numpy as R
from cvsd_amd import _lib, ops


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_host_twin_matches_checker(name):
    f, p = K.CASES[name]
    keep = f.copy()
    got = ops.render(f, p, device=-1)
    assert got.dtype == np.uint8 and got.shape == f.shape
    assert np.array_equal(f, keep), "the source frame was written"
    want = K.reference(name)
    bad = np.argwhere((got != want).any(axis=2))
    assert not len(bad), f"{len(bad)} pixels differ, first (y, x) = {bad[0]}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"


def test_cases_draw_something():
    """a table whose pictures all equal their sources would check nothing"""
    for name in ("mosaic", "rect", "fill", "line", "disc", "glyph", "33x70", "1x1", "1x40", "corners", "off_frame", "200_on_a_tile"):
        assert not np.array_equal(K.reference(name), K.CASES[name][0]), name
    for name in ("empty_list", "empty_rects", "1x1_untouched"):
        assert np.array_equal(K.reference(name), K.CASES[name][0]), name


def test_empty_list_and_none_copy_the_frame():
    f = K.frame(33, 70)
    assert np.array_equal(ops.render(f, np.zeros((0, 8), np.int32), device=-1), f)
    assert np.array_equal(ops.render(f, None, device=-1), f)


def test_pitched_source_and_several_frames():
    big = K.frame(40, 100)
    view = big[3:36, 7:77]                                       # 33 x 70, rows 300 bytes apart
    p = K.CASES["33x70"][1]
    names = ["corners", "1x40", "mosaic_edge_16"]
    got = ops.render([view] + [K.CASES[n][0] for n in names], [p] + [K.CASES[n][1] for n in names], device=-1)
    assert np.array_equal(got[0], R.render(np.ascontiguousarray(view), p))
    for g, n in zip(got[1:], names):
        assert np.array_equal(g, K.reference(n))


def _raw_call(f, p, out):
    fd = _lib.RenderFrame(f.ctypes.data, f.shape[0], f.shape[1], f.strides[0], 0)
    od = _lib.RenderOut(out.ctypes.data, out.strides[0], 0)
    ptrs = (C.c_void_p * 1)(p.ctypes.data)
    cnt = (C.c_int * 1)(len(p))
    return _lib.lib().mi355_render(-1, C.byref(fd), 1, ptrs, cnt, C.byref(od), None, None)


def test_limit_plus_one_is_an_error_and_nothing_is_written():
    f = K.frame(48, 64)
    p = np.tile(K.P((K.DISC, 5, 5, 0, 0, 2, 0xFFFFFF)), (_lib.RENDER_MAX_PRIMS + 1, 1))
    out = np.full_like(f, 0xA5)
    rc = _raw_call(f, p, out)
    assert rc == -1 and b"16384" in _lib.lib().mi355_last_error()
    assert (out == 0xA5).all(), "the output was touched"
    with pytest.raises(ValueError, match="16384"):
        ops.render(f, p, device=-1)
    assert _raw_call(f, p[:-1], out) == 0                         # the limit itself is drawn
    assert np.array_equal(out, R.render(f, p[:1]))


@pytest.mark.parametrize("bad", [(0, 1, 1, 2, 2, 1, 0), (7, 1, 1, 2, 2, 1, 0), (K.M, 0, 0, 9, 9, 5, 0), (K.LINE, 0, 0, 9, 9, 0, 0), (K.LINE, 0, 0, 9, 9, 256, 0),
                                 (K.DISC, 0, 0, 0, 0, -1, 0), (K.GLYPH, 0, 0, ord("A"), 0, 1, 0), (K.GLYPH, 0, 0, ord("1"), 0, 0, 0),
                                 (K.FILL, (1 << 20) + 1, 0, 5, 5, 0, 0), (K.FILL, 0, 0, 5, 5, 0, 1 << 24)])
def test_bad_records_are_refused_before_any_write(bad):
    f = K.frame(8, 8)
    out = np.full_like(f, 0xA5)
    assert _raw_call(f, K.P((K.FILL, 0, 0, 7, 7, 0, 0), bad), out) == -1
    assert (out == 0xA5).all()


# ---- known answers, derived by hand ------------------------------------------------------------------------------------------------
def _set(img, bg):
    return {(int(x), int(y)) for y, x in np.argwhere((img != bg).any(axis=2))}


def test_disc_of_radius_one_and_of_three_pixels_across():
    z = np.zeros((9, 9, 3), np.uint8)
    # r = 1: dx^2 + dy^2 <= 1 -> the centre and its four neighbours, three pixels across
    got = ops.render(z, K.P((K.DISC, 4, 4, 0, 0, 1, 0x0000FF)), device=-1)
    assert _set(got, 0) == {(4, 4), (3, 4), (5, 4), (4, 3), (4, 5)}
    assert (got[4, 4] == (255, 0, 0)).all()                       # colour = B | G << 8 | R << 16: 0x0000FF is blue
    # r = 0: one pixel
    assert _set(ops.render(z, K.P((K.DISC, 2, 7, 0, 0, 0, 0x00FF00)), device=-1), 0) == {(2, 7)}
    # r = 2: dx^2 + dy^2 <= 4 -> 13 pixels: the 3 x 3 block and the four at distance 2 on the axes
    want = {(4 + dx, 4 + dy) for dx in (-1, 0, 1) for dy in (-1, 0, 1)} | {(2, 4), (6, 4), (4, 2), (4, 6)}
    assert _set(ops.render(z, K.P((K.DISC, 4, 4, 0, 0, 2, 1)), device=-1), 0) == want


def test_horizontal_line_of_thickness_one():
    z = np.zeros((5, 12, 3), np.uint8)
    # t = 1: 4 dist^2 <= 1 holds for dist = 0 only -> exactly the pixels of the segment, ends included, nothing above or below
    got = ops.render(z, K.P((K.LINE, 2, 3, 8, 3, 1, 0xFF0000)), device=-1)
    assert _set(got, 0) == {(x, 3) for x in range(2, 9)}
    assert (got[3, 5] == (0, 0, 255)).all()
    # t = 2: dist <= 1 -> one row above and below as well, and one pixel beyond each end on the line's row
    got = ops.render(z, K.P((K.LINE, 2, 2, 8, 2, 2, 1)), device=-1)
    assert _set(got, 0) == {(x, y) for x in range(2, 9) for y in (1, 2, 3)} | {(1, 2), (9, 2)}


def test_glyph_one():
    z = np.zeros((9, 8, 3), np.uint8)
    got = ops.render(z, K.P((K.GLYPH, 1, 1, ord("1"), 0, 1, 0xFFFFFF)), device=-1)
    rows = ["..#..", ".##..", "..#..", "..#..", "..#..", "..#..", ".###."]
    assert _set(got, 0) == {(1 + c, 1 + r) for r in range(7) for c in range(5) if rows[r][c] == "#"}
    # scale 2: every font pixel a 2 x 2 square
    z = np.zeros((16, 12, 3), np.uint8)
    got = ops.render(z, K.P((K.GLYPH, 0, 0, ord("1"), 0, 2, 0xFFFFFF)), device=-1)
    assert _set(got, 0) == {(2 * c + i, 2 * r + j) for r in range(7) for c in range(5) if rows[r][c] == "#" for i in (0, 1) for j in (0, 1)}


def test_every_font_character_matches_the_checker_table():
    for ch in "0123456789#.:%- ":
        z = np.zeros((7, 5, 3), np.uint8)
        got = ops.render(z, K.P((K.GLYPH, 0, 0, ord(ch), 0, 1, 0xFFFFFF)), device=-1)
        want = {(c, r) for r in range(7) for c in range(5) if R.FONT[ch][r][c] == "#"}
        assert _set(got, 0) == want, ch


def test_mosaic_mean_of_a_2x2_frame_rounds_halves_up():
    f = np.zeros((2, 2, 3), np.uint8)
    f[..., 0] = [[1, 2], [3, 4]]          # sum 10 / 4 = 2.5 -> 3
    f[..., 1] = [[1, 1], [1, 2]]          # sum 5 / 4 = 1.25 -> 1
    f[..., 2] = [[255, 255], [255, 254]]  # sum 1019 / 4 = 254.75 -> 255
    for B in (4, 8, 16, 32):              # the frame cuts every block down to its 2 x 2 pixels
        got = ops.render(f, K.P((K.M, 0, 0, 0, 0, B, 0)), device=-1)
        assert (got[0, 0] == (3, 1, 255)).all()
        assert np.array_equal(got[0, 1], f[0, 1]) and np.array_equal(got[1], f[1])       # only the rectangle's pixel changes
