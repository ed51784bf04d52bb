"""The tile grid of predict(tile=..., overlap=...): mi355_tile_grid through ops.tile_grid against its known answers, the sequential
statement in tests/_tile_merge_numpy.py, and the two properties a grid must have (inside the frame, covering every pixel).  Host
arithmetic only: no GPU."""
import ctypes as C

import numpy as np
import pytest

from cvsd_amd import _lib, ops

from _tile_merge_numpy import axis_positions, tile_grid

# (L, tile, overlap) -> positions along one axis; the extent is min(tile, L)
AXIS = [
    (1920, 640, 0.2, [0, 512, 1024, 1280]),
    (1080, 640, 0.2, [0, 440]),
    (3840, 640, 0.2, [0, 512, 1024, 1536, 2048, 2560, 3072, 3200]),
    (2160, 640, 0.2, [0, 512, 1024, 1520]),
    (224, 96, 0.25, [0, 72, 128]),
    (160, 96, 0.25, [0, 64]),
    (50, 96, 0.25, [0]),
    (96, 96, 0.25, [0]),
    (97, 96, 0.25, [0, 1]),
    (1281, 640, 0, [0, 640, 641]),
]


@pytest.mark.parametrize("L,t,ov,want", AXIS)
def test_axis_known_answers(L, t, ov, want):
    assert axis_positions(L, t, int(ov * t)) == want                     # the checker states the same rule
    gx = ops.tile_grid(40, L, (32, t), ov)                               # L as the width: one row of tiles (height 40 > 32 gives two)
    xs = gx[gx[:, 1] == 0]
    assert xs[:, 0].tolist() == want and set(xs[:, 2].tolist()) == {min(t, L)}
    gy = ops.tile_grid(L, 32, (t, 32), ov)                               # L as the height: one column
    assert gy[:, 1].tolist() == want and set(gy[:, 3].tolist()) == {min(t, L)} and set(gy[:, 0].tolist()) == {0}


def test_full_lists():
    g = ops.tile_grid(1080, 1920, 640, 0.2)
    assert g.dtype == np.int32 and g.tolist() == [[x, y, 640, 640] for y in (0, 440) for x in (0, 512, 1024, 1280)]
    g = ops.tile_grid(160, 224, 96, 0.25)
    assert g.tolist() == [[x, y, 96, 96] for y in (0, 64) for x in (0, 72, 128)]
    assert ops.tile_grid(50, 60, 96, 0.25).tolist() == [[0, 0, 60, 50]]          # a frame smaller than the tile: one tile, the frame
    assert ops.tile_grid(160, 224, (96, 128), 0.25).tolist() == [[x, y, 128, 96] for y in (0, 64) for x in (0, 96)]


def test_inside_and_covering_sweep():
    rng = np.random.default_rng(20240917)
    for _ in range(300):
        H, W = (int(v) for v in rng.integers(1, 301, 2))
        th, tw = (int(v) for v in rng.integers(32, 129, 2))
        ov = float(rng.choice([0.0, 0.1, 0.25, 0.5, 0.75, 0.9]))
        g = ops.tile_grid(H, W, (th, tw), ov)
        assert np.array_equal(g, tile_grid(H, W, th, tw, int(ov * th), int(ov * tw))), (H, W, th, tw, ov)
        assert (g[:, 0] >= 0).all() and (g[:, 1] >= 0).all() and (g[:, 2] > 0).all() and (g[:, 3] > 0).all()
        assert (g[:, 0] + g[:, 2] <= W).all() and (g[:, 1] + g[:, 3] <= H).all(), (H, W, th, tw, ov)
        cover = np.zeros((H, W), bool)
        for x, y, w, h in g:
            cover[y:y + h, x:x + w] = True
        assert cover.all(), (H, W, th, tw, ov)
        assert len({tuple(r) for r in g.tolist()}) == len(g)            # no tile twice


def test_refusals():
    with pytest.raises(ValueError, match="tile"):
        ops.tile_grid(100, 100, 31)
    with pytest.raises(ValueError, match="tile"):
        ops.tile_grid(100, 100, (64, 16))
    with pytest.raises(TypeError, match="tile"):
        ops.tile_grid(100, 100, 64.0)
    with pytest.raises(TypeError, match="tile"):
        ops.tile_grid(100, 100, "64")
    for ov in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError, match="overlap"):
            ops.tile_grid(100, 100, 64, ov)
    with pytest.raises(TypeError, match="overlap"):
        ops.tile_grid(100, 100, 64, "0.2")
    # the C entry point itself: pixels, refused with MI355_EINVAL
    lib, cnt = _lib.lib(), C.c_int()
    for args in ((0, 100, 64, 64, 0, 0), (100, 0, 64, 64, 0, 0), (100, 100, 0, 64, 0, 0), (100, 100, 64, 64, 64, 0), (100, 100, 64, 64, 0, -1)):
        assert lib.mi355_tile_grid(*args, None, 0, C.byref(cnt)) == -1, args
    out = np.zeros((2, 4), np.int32)
    assert lib.mi355_tile_grid(160, 224, 96, 96, 24, 24, out.ctypes.data, 2, C.byref(cnt)) == -1 and cnt.value == 6      # cap too small
    with pytest.raises(ValueError, match="overlap"):
        _lib.check(lib.mi355_tile_grid(100, 100, 64, 64, 64, 0, None, 0, C.byref(cnt)))
