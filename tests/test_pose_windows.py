"""Pose windows without a GPU: the kernel's per-window routine compiled for the host (``ops.pose_windows(device=-1)``, the same
``__host__ __device__`` template the kernel runs) against the numpy path it replaces, bit for bit, and the Python layer above it
(the vectorised window cut, ``score_poselift(on_device=True)``, ``score_poselift_many``, ``MultiStreamScorer``) with stub models."""
import numpy as np
import pytest

import _pose_window_cases as K
from cvsd_amd import ops
from cvsd_amd import shopformer as SF


@pytest.fixture(scope="module")
def clip():
    return K.fixture_clip()


def test_fixture_in_float32_gives_the_reference_loaders_windows(clip):
    pf, data, T, stride = clip
    poses, starts, index = SF.pack_poselift(data, T, stride)
    assert poses.dtype == np.float32 and poses.shape[1:] == (17, 2) and len(starts) == len(index) == len(pf["train_xy_x"]) > 0
    w17 = ops.pose_windows(poses, starts, T, 17, device=-1)
    assert K.same_bits(w17, pf["train_xy_x"]) and K.same_bits(w17, pf["test_xy_x"])
    assert K.same_bits(ops.pose_windows(poses, starts, T, 18, neck=True, device=-1), pf["s2_train_xy_x"])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("V,neck", [(17, False), (18, True), (18, False)])
def test_fixture_equals_windows_from_poselift(clip, dtype, V, neck):
    _, data, T, stride = clip
    cast = {f: {p: [b, np.asarray(k, dtype)] for p, (b, k) in people.items()} for f, people in data.items()}
    poses, starts, index = SF.pack_poselift(cast, T, stride)
    want, want_index = SF.windows_from_poselift(cast, seq_len=T, stride=stride, num_keypoints=V, neck=neck)
    assert poses.dtype == dtype and index == want_index
    assert K.same_bits(ops.pose_windows(poses, starts, T, V, neck=neck, device=-1), want)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("T", [12, 24])
@pytest.mark.parametrize("v_src,V,neck", K.CONFIGS)
def test_edge_windows_equal_window_tensor(dtype, T, v_src, V, neck):
    wins = K.edge_set(T, v_src, dtype)
    poses, starts = K.flatten(wins)
    got, want = ops.pose_windows(poses, starts, T, V, neck=neck, device=-1), K.host_windows(wins, V, neck)
    bad = [K.MODES[i // 3] for i in range(len(wins)) if not K.same_bits(got[i], want[i])]
    assert not bad, bad
    assert not (got.view(np.uint32) == ops.SENTINEL_BITS).any()


def test_overlapping_and_unordered_starts_are_windows_of_their_own():
    rng = np.random.default_rng(3)
    poses = rng.uniform(1, 640, (40, 17, 2)).astype(np.float32)
    starts = np.array([5, 0, 6, 28, 5, 11], np.int32)
    got = ops.pose_windows(poses, starts, 12, 17, device=-1)
    for g, s in zip(got, starts):
        assert K.same_bits(g, SF._window_tensor([np.c_[p, np.ones(17, np.float32)] for p in poses[s:s + 12]], 17))


def test_refusals_and_the_empty_call():
    poses = np.ones((20, 17, 2), np.float32)
    for starts in ([-1], [9], [0, 3, 2**31 - 5]):
        with pytest.raises(ValueError, match="starts"):
            ops.pose_windows(poses, starts, 12, 17, device=-1)
    assert ops.pose_windows(poses, [8], 12, 17, device=-1).shape == (1, 2, 12, 17)          # the last window that fits
    with pytest.raises(ValueError, match="neck"):
        ops.pose_windows(poses, [0], 12, 17, neck=True, device=-1)
    with pytest.raises(ValueError, match="neck"):
        ops.pose_windows(poses[:, :6], [0], 12, 18, neck=True, device=-1)
    with pytest.raises(ValueError, match="V_src"):
        ops.pose_windows(np.ones((20, 0, 2), np.float32), [0], 12, 17, device=-1)
    with pytest.raises(ValueError, match="float32 or float64"):
        ops.pose_windows(poses.astype(np.int32), [0], 12, 17, device=-1)
    with pytest.raises(ValueError, match="V_src, 2"):
        ops.pose_windows(np.ones((20, 17, 3), np.float32), [0], 12, 17, device=-1)
    empty = ops.pose_windows(poses, [], 12, 17, device=-1)
    assert empty.shape == (0, 2, 12, 17) and empty.dtype == np.float32
    with pytest.raises(ValueError, match="neck"):                                              # an empty call is still checked
        ops.pose_windows(poses, [], 12, 17, neck=True, device=-1)


def test_the_vectorised_cut_gives_the_loaders_index(clip):
    _, data, T, stride = clip
    assert SF.pack_poselift(data, T, stride)[2] == SF.windows_from_poselift(data, seq_len=T, stride=stride)[1]
    for s, g in ((1, 0), (5, 1), (12, 5)):                                                  # other strides and gap limits cut alike
        assert SF.pack_poselift(data, T, s, g)[2] == SF.windows_from_poselift(data, seq_len=T, stride=s, max_gap=g)[1]
    gap = K.gap_dict()
    poses, starts, index = SF.pack_poselift(gap)
    assert index == SF.windows_from_poselift(gap)[1] and [i[1:] for i in index] == [(0, 11), (30, 41)]   # none straddles the hole
    assert len(poses) == 24 and K.same_bits(ops.pose_windows(poses, starts, 12, 17, device=-1), SF.windows_from_poselift(gap)[0])
    gap[5][1][1] = np.full((17, 3), np.nan, np.float32)                                     # the NaN pose is left out before the cut
    poses, starts, index = SF.pack_poselift(gap)
    assert len(poses) == 23 and index == SF.windows_from_poselift(gap)[1] and (0, 11) not in [i[1:] for i in index]
    k = np.ones((17, 3), np.float32)
    k[:, 0] = np.arange(17)
    flat = {f: {1: [np.zeros(4, np.float32), (k * (1 + 0.01 * f)).reshape(-1)]} for f in range(20)}
    poses, starts, index = SF.pack_poselift(flat)
    want, want_index = SF.windows_from_poselift(flat)
    assert poses.shape == (20, 17, 2) and index == want_index and len(index) == 2
    assert K.same_bits(ops.pose_windows(poses, starts, 12, 17, device=-1), want)


@pytest.mark.parametrize("V,neck", [(17, False), (18, True)])
def test_score_poselift_on_device_is_the_host_path(clip, V, neck):
    _, data, _, _ = clip
    model = K.TwinModel(V, neck)
    want, want_index = SF.score_poselift(model, data)
    assert model.pose_calls == 0                                                              # the keyword defaults to the present behaviour
    got, index = SF.score_poselift(model, data, on_device=True)
    assert model.pose_calls == 1 and index == want_index and np.array_equal(got, want) and len(got) > 0
    many = SF.score_poselift_many(model, [data, {}, K.gap_dict()])
    assert model.pose_calls == 2 and len(many) == 3 and many[1][1] == [] and many[1][0].shape == (0,)
    for (s, i), d in zip(many, (data, {}, K.gap_dict())):
        ws, wi = SF.score_poselift(model, d)
        assert i == wi and np.array_equal(s, ws)


def test_dicts_the_device_path_does_not_cover_take_the_host_path(clip):
    _, data, _, _ = clip
    frames = sorted(data)
    mixed = {f: {p: [b, np.asarray(k, np.float64 if f % 2 else np.float32)] for p, (b, k) in data[f].items()} for f in frames}
    ragged = {f: {p: [b, k[:12] if p % 2 else k] for p, (b, k) in data[f].items()} for f in frames}
    ints = {f: {p: [b, np.asarray(k, np.int64)] for p, (b, k) in data[f].items()} for f in frames}
    for d in (mixed, ragged, ints):
        model = K.TwinModel()
        assert SF.pack_poselift(d)[0] is None
        got, index = SF.score_poselift(model, d, on_device=True)
        want, want_index = SF.score_poselift(model, d)
        assert model.pose_calls == 0 and index == want_index and np.array_equal(got, want) and len(got) > 0
        many = SF.score_poselift_many(model, [data, d])                                      # one such dict sends the whole tree to the host
        assert model.pose_calls == 0 and np.array_equal(many[1][0], want) and many[1][1] == want_index
    short = {f: {p: [b, k[:12]] for p, (b, k) in data[f].items()} for f in frames}            # a neck model fed 12 rows: numpy promotes
    neck = K.TwinModel(18, True)
    got, index = SF.score_poselift(neck, short, on_device=True)
    want, want_index = SF.score_poselift(neck, short)
    assert neck.pose_calls == 0 and index == want_index and np.array_equal(got, want) and len(got) > 0
    plain = K.TwinModel()                                                                     # without a neck 12 rows are zero-padded in F
    got, _ = SF.score_poselift(plain, short, on_device=True)
    assert plain.pose_calls == 1 and np.array_equal(got, SF.score_poselift(plain, short)[0])
    stub = K.StubModel()                                                                      # a model without score_poses
    assert np.array_equal(SF.score_poselift(stub, data, on_device=True)[0], SF.score_poselift(stub, data)[0])


@pytest.mark.parametrize("model", [K.StubModel(), K.TwinModel(), K.TwinModel(18, True)], ids=["host", "twin17", "twin18neck"])
def test_multi_stream_scorer_equals_one_stream_scorer_per_camera(clip, model):
    _, data, _, _ = clip
    ticks = K.camera_ticks(data)
    got, want = K.play(model, ticks)
    assert got == want
    per_cam = [sum(len(t[c]) for t in want) for c in range(3)]
    assert min(per_cam) > 0 and per_cam[2] < per_cam[0]                                      # the hole cost camera 2 windows
    if isinstance(model, K.TwinModel):                                                         # one call per tick that completes a window
        assert model.pose_calls == sum(1 for t in want if any(t)) > 0


def test_multi_stream_scorer_takes_one_frame_number_and_checks_its_arguments(clip):
    _, data, _, _ = clip
    ticks = K.camera_ticks(data, n_ticks=14)
    multi, single = SF.MultiStreamScorer(K.TwinModel(), 3), SF.StreamScorer(K.StubModel())
    n = 0
    for t, (_, cams) in enumerate(ticks):
        got = multi.update(t, [cams[0], None, cams[0]])
        want = single.update(t, *cams[0])
        assert got == [want, [], want]
        n += len(want)
    assert n > 0 and len(multi.cameras[0]._ring) > 0 and not multi.cameras[1]._ring
    with pytest.raises(ValueError, match="per camera"):
        multi.update(99, [None])
    with pytest.raises(ValueError, match="per camera"):
        multi.update([99, 100], [None, None, None])
