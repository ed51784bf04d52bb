"""The memory plan of an engine with object features (mi355_opts.obj_feats, csrc/engine_memory.hip), host-only: the three Detect-input
buffers get bytes of their own -- the gather reads them behind the chunk's NMS, after the last op of the pass -- every other buffer
still satisfies the sharing rule of tests/test_memory_plan.py, and with the option off nothing moves."""
import itertools

import numpy as np
import pytest

from cvsd_amd import ops
from cvsd_amd.graph import engine_program, parse_model_name
from test_memory_plan import _blob, _dag

MODELS = ["yolov8n", "yolov8s-pose", "yolov8m", "yolov5mu", "yolo11n"]      # yolov8m: 192 / 384 / 576, the g = 3 level


def _detect_inputs(prog):
    """(buffer, channel offset, channels) of each level's Detect input, by NAME: the source slice of the conv that is, or begins
    with, cv2.<level>.0 -- independent of the loader's walk back from the box-logit writer"""
    out = {}
    for o in prog.ops:
        if o.conv is None or o.conv < 0:
            continue
        first = prog.convs[o.conv].name.split("+")[0].split(".")
        if len(first) >= 3 and first[-3] == "cv2" and first[-1] == "0":
            out[int(first[-2])] = (o.src.buf, o.src.choff, o.src.c)
    return [out[l] for l in range(len(prog.levels))]


@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("n,size", [(1, 640), (4, 640), (64, 320)])
def test_option_off_is_the_plain_plan(name, n, size):
    blob = _blob(name)
    for reuse in (True, False):
        o0, s0, a0, p0 = ops.memory_plan(blob, n, size, size, imgsz=size, reuse=reuse)
        o1, s1, a1, p1, det = ops.memory_plan_ex(blob, n, size, size, imgsz=size, reuse=reuse, obj_feats=False)
        assert np.array_equal(o0, o1) and np.array_equal(s0, s1) and (a0, p0) == (a1, p1)


@pytest.mark.parametrize("name", MODELS)
def test_detect_inputs_keep_bytes_of_their_own(name):
    prog = engine_program(*parse_model_name(name))
    blob = _blob(name)
    want = _detect_inputs(prog)
    off0, size0, arena0, plain0 = ops.memory_plan(blob, 4, 640, 640)
    off, size, arena, plain, det = ops.memory_plan_ex(blob, 4, 640, 640, obj_feats=True)
    assert det == [b for b, _, _ in want], "the loader found other buffers than cv2.<level>.0 reads"
    assert np.array_equal(size, size0) and plain == plain0 and arena == int((off + size).max())
    overlaps = lambda a, b: off[a] < off[b] + size[b] and off[b] < off[a] + size[a]
    for d in det:
        assert not [b for b in range(len(off)) if b != d and overlaps(d, b)], f"{name}: Detect input {d} shares bytes"
    # every other pair that shares bytes still obeys the rule (every user of the earlier buffer is a RAW ancestor of every writer of the later)
    anc, users, writers = _dag(prog)
    head = {lv.buf for lv in prog.levels}
    shared = 0
    for a, b in itertools.combinations(range(len(off)), 2):
        if not overlaps(a, b):
            continue
        shared += 1
        assert a not in head and b not in head and a not in det and b not in det
        first, second = (a, b) if min(writers[a]) < min(writers[b]) else (b, a)
        for w in writers[second]:
            assert not users[first] - anc[w], f"{name}: buffer {second} overlaps buffer {first}, still in use"
    assert shared > 0 and (off % 256 == 0).all()
    maps = int(sum(size[d] for d in det))
    print(f"[obj_feats plan] {name}, 4 x 640x640: arena {arena0 / 2**20:.1f} -> {arena / 2**20:.1f} MiB (+{(arena - arena0) / 2**20:.1f} MiB); "
          f"the three Detect-input maps are {maps / 2**20:.1f} MiB")
    assert arena0 <= arena <= arena0 + maps, "keeping three maps alive costs at most those maps"


def test_loader_finds_the_detect_inputs_of_every_width():
    """s = min(C_l) and g_l = C_l / s of SURVEY.md Appendix A.8's table, as the LOADER finds them: the buffers ``mi355_memory_plan_ex``
    reports (its walk back from the box-logit writers) hold these channel counts and are the ones cv2.<level>.0 reads"""
    table = {"yolov8n": (64, 128, 256), "yolo11n": (64, 128, 256), "yolov8s-pose": (128, 256, 512), "yolov8m": (192, 384, 576),
             "yolov5mu": (192, 384, 768)}
    for name, chans in table.items():
        prog = engine_program(*parse_model_name(name))
        det = ops.memory_plan_ex(_blob(name), 1, 320, 320, imgsz=320, obj_feats=True)[4]
        assert det == [b for b, _, _ in _detect_inputs(prog)]
        assert tuple(prog.buffers[d][0] for d in det) == chans and all(off == 0 and c == prog.buffers[b][0] for b, off, c in _detect_inputs(prog))
        assert all(c % min(chans) == 0 for c in chans)
