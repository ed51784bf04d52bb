"""Every Shopformer score entry point against every other (reads only the repository): each valid subset of the six outputs through
``mi355_shopformer_score_ex``, ``mi355_shopformer_score_ex_device_async`` (on a stream of its own) and ``mi355_shopformer_score_poses``
gives the bits of ONE all-outputs call, writes nothing it was not asked for, and enqueues the launches it should; the handle's buffers
grow call by call; a device / async call and a blocking call on one handle do not disturb each other; a refused call launches nothing.
The all-outputs ``forward(x, poses=True)`` that serves as the expected value is what test_gpu_shopformer*.py check against the
reference.  n = 21 windows: a ragged last group at every group size in use (8 or fewer, 16, 4)."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import _shopformer_decoder_numpy as RD
from cvsd_amd import _lib, ops
from cvsd_amd.shopformer import ShopformerOutputs

pytestmark = pytest.mark.gpu
N = 21
NAMES = ("default", "paper")                                                     # the decoder fixtures of variant 1 and variant 2
FIELDS = ("scores", "token_scores", "tokens", "recon", "poses", "pose_error")    # mi355_shopformer_outputs_t, in its order
KEY = dict(zip(FIELDS, ("normality_score", "token_scores", "tokens", "reconstructed_tokens", "gcae_reconstructed", "pose_error")))
ENTRIES = ("ex", "ex_device_async", "score_poses")
SENT = np.float32(-7777.25)                                                       # what a buffer nobody asked for must still hold
EINVAL = -1


def subsets(variant):
    """every valid set of outputs: variant 1 always has scores, pose_error only beside poses, never empty: 12 and 47"""
    out = []
    for sc, ts, tk, rc in itertools.product((True, False), repeat=4):
        if (variant == 1 and (ts or not sc)):
            continue
        for pose in ((), ("poses",), ("poses", "pose_error")):
            s = tuple(f for f, on in zip(FIELDS[:4], (sc, ts, tk, rc)) if on) + pose
            if s:
                out.append(s)
    return out


def shapes(m, n):
    tok, win = (m.n_tokens, m.token_dim), (m.seq_len, m.num_keypoints)
    return {"scores": (n,), "token_scores": (n, m.n_tokens), "tokens": (n,) + tok, "recon": (n,) + tok, "poses": (n, 2) + win,
            "pose_error": (n,) + win}


def same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


class Case:
    """one model with the decoder, its 21 windows, 21 windows' worth of poses and starts, and the expected outputs of both"""

    def __init__(self, name):
        from cvsd_amd import Shopformer
        self.cfg, self.sd, x = RD.fixture_model(name)
        self.new = lambda: Shopformer.from_state_dict(self.sd, self.cfg, device=0, decoder=True)
        self.m = m = self.new()
        self.x = np.ascontiguousarray(x[:N])
        self.dev = torch.device("cuda:0")
        self.xd = torch.from_numpy(self.x).to(self.dev)
        self.stream = torch.cuda.Stream(device=self.dev)
        full = m.forward(self.x, poses=True)
        self.want = {f: full[KEY[f]] for f in FIELDS if KEY[f] in full}
        rng = np.random.default_rng(11)
        self.poses = rng.uniform(1, 640, (5 * m.seq_len, 17, 2)).astype(np.float32)
        self.starts = rng.integers(0, len(self.poses) - m.seq_len + 1, N).astype(np.int32)
        self.all = tuple(f for f in FIELDS if f in self.want)
        rc, got, _ = self.call("score_poses", self.all)
        assert rc == 0
        self.want_poses = {f: got[f] for f in self.all}
        # ... which are the bits of the blocking call on the windows the host twin of the window kernel builds from those poses
        wins = ops.pose_windows(self.poses, self.starts, m.seq_len, m.num_keypoints, neck=m.neck, device=-1)
        twin = m.forward(wins, poses=True)
        assert all(same(self.want_poses[f], twin[KEY[f]]) for f in self.all)

    def call(self, entry, asked, n=N, m=None, struct_size=None):
        """-> (return code, {field: array} for ALL six fields, launches enqueued); fields not asked for were pre-filled with SENT"""
        m = m or self.m
        L = _lib.lib()
        host = {f: np.full(s, SENT, np.float32) for f, s in shapes(m, n).items()}
        size = C.sizeof(ShopformerOutputs) if struct_size is None else struct_size
        c0 = m.launches
        if entry == "ex_device_async":
            bufs = {f: torch.from_numpy(a).to(self.dev) for f, a in host.items()}
            torch.cuda.synchronize()
            o = ShopformerOutputs(size, 0, *(bufs[f].data_ptr() if f in asked else None for f in FIELDS))
            with torch.cuda.stream(self.stream):
                rc = L.mi355_shopformer_score_ex_device_async(m._h, self.xd.data_ptr(), n, C.byref(o), self.stream.cuda_stream)
            self.stream.synchronize()
            host = {f: b.cpu().numpy() for f, b in bufs.items()}
        else:
            o = ShopformerOutputs(size, 0, *(host[f].ctypes.data if f in asked else None for f in FIELDS))
            if entry == "ex":
                rc = L.mi355_shopformer_score_ex(m._h, self.x.ctypes.data, n, C.byref(o))
            else:
                rc = L.mi355_shopformer_score_poses(m._h, self.poses.ctypes.data, _lib.POSE_F32, len(self.poses), self.poses.shape[1],
                                                    self.starts.ctypes.data, n, int(m.neck), C.byref(o))
        return rc, host, m.launches - c0

    def expected(self, entry, n=N):
        return {f: a[:n] for f, a in (self.want_poses if entry == "score_poses" else self.want).items()}


@pytest.fixture(scope="module")
def cases():
    return {name: Case(name) for name in NAMES}


def check(case, entry, asked, n=N, m=None):
    rc, got, launched = case.call(entry, asked, n, m)
    assert rc == 0, (entry, asked, _lib.lib().mi355_last_error().decode())
    want = case.expected(entry, n)
    for f in FIELDS:
        if f in asked:
            assert same(got[f], want[f]), (entry, asked, f)
        else:
            assert (got[f] == SENT).all(), (entry, asked, f, "was written although nobody asked for it")
    variant = (m or case.m).variant
    assert launched == (2 if variant == 2 else 1) + ("poses" in asked) + (entry == "score_poses"), (entry, asked, launched)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", NAMES)
def test_every_subset_of_outputs_gives_the_bits_of_the_all_outputs_call(cases, name, entry):
    case = cases[name]
    sets = subsets(case.m.variant)
    assert len(sets) == (47 if case.m.variant == 2 else 12) and len(set(sets)) == len(sets)
    for asked in sets:
        check(case, entry, asked)


@pytest.mark.parametrize("name", NAMES)
def test_buffers_grow_call_by_call(cases, name):
    """fresh handles; n = 3, 21, 3 with another subset each time, the decoder alone as the very first call, then the device form"""
    case = cases[name]
    ts = ("token_scores",) if case.m.variant == 2 else ()
    tokens = case.want["tokens"]
    m = case.new()
    assert same(m.decode(tokens[:3]), case.want["poses"][:3])                     # nothing but the token and pose buffers exist yet
    check(case, "ex", ("scores", "recon"), 21, m)
    check(case, "ex", ("scores", "tokens", "poses", "pose_error") + ts, 3, m)
    assert same(m.decode(tokens), case.want["poses"])
    check(case, "score_poses", ("scores", "poses"), 21, m)
    m = case.new()
    check(case, "ex", ("scores",), 3, m)
    check(case, "ex", ("scores", "tokens", "poses"), 21, m)
    check(case, "score_poses", ("scores", "recon") + ts, 3, m)
    check(case, "ex_device_async", ("scores", "poses"), 3, m)                     # no tokens output: the handle's scratch, grown twice
    check(case, "ex_device_async", ("scores", "poses", "pose_error") + ts, 21, m)
    check(case, "ex_device_async", ("scores", "recon"), 3, m)
    check(case, "ex", case.all, 21, m)


@pytest.mark.parametrize("name", NAMES)
def test_a_blocking_call_may_follow_a_device_call_at_once(cases, name):
    """the device call keeps its tokens in the handle's scratch on ITS stream while the blocking call stages tokens on the handle's"""
    case = cases[name]
    m = case.m
    sh = shapes(m, N)
    sc, pose, err = (torch.full(sh[f], float(SENT), device=case.dev) for f in ("scores", "poses", "pose_error"))
    torch.cuda.synchronize()
    o = ShopformerOutputs(C.sizeof(ShopformerOutputs), 0, sc.data_ptr(), None, None, None, pose.data_ptr(), err.data_ptr())
    with torch.cuda.stream(case.stream):
        rc = _lib.lib().mi355_shopformer_score_ex_device_async(m._h, case.xd.data_ptr(), N, C.byref(o), case.stream.cuda_stream)
    full = m.forward(case.x, poses=True)                                          # at once: nothing waited for the device call
    case.stream.synchronize()
    assert rc == 0
    assert all(same(full[KEY[f]], case.want[f]) for f in case.all)
    assert same(sc.cpu().numpy(), case.want["scores"]) and same(pose.cpu().numpy(), case.want["poses"])
    assert same(err.cpu().numpy(), case.want["pose_error"])


# the phrases are those of csrc/shopformer_host.hip before its entry points were restated, word for word
REFUSALS = (("every output null", (), None, "every output pointer is null"),
            ("token_scores on variant 1", ("scores", "token_scores"), None, "token_scores exist only for the shopformer_2 variant (version-2 images)"),
            ("pose_error without poses", ("scores", "pose_error"), None, "pose_error is written beside poses: set the poses output too"),
            ("struct_size", ("scores",), C.sizeof(ShopformerOutputs) - 4, "mi355_shopformer_outputs_t: null or struct_size is not sizeof"))


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", NAMES)
def test_refused_calls_launch_nothing(cases, name, entry):
    case = cases[name]
    for what, asked, size, phrase in REFUSALS:
        if what.startswith("token_scores") and case.m.variant == 2:
            continue                                                              # valid there
        rc, got, launched = case.call(entry, asked, struct_size=size)
        msg = _lib.lib().mi355_last_error().decode()
        assert rc == EINVAL and launched == 0 and phrase in msg, (what, rc, launched, msg)
        assert all((a == SENT).all() for a in got.values()), what
