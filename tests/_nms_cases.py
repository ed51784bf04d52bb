"""Inputs with planted edges, and the reference, for the isolated tests of the detector's tail (csrc/post_kernels.hip: candidate
filter, the three sorts, greedy suppression, scale-back, rows, row compaction) through cvsd_amd.ops.postprocess.

The reference is oracle.yolo_oracle.non_max_suppression(..., max_nms=..., return_idxs=True), scale_boxes on the boxes and
scale_coords on the keypoints.  A case is a POOL of distinct frames [4+nc+extra, A] plus the batch sizes it runs at: frame i of a
batch of n is pool[order[i]] (cycled, or drawn with a fixed seed), so the oracle runs once per pool frame whatever n is, and which
launch path a run takes follows from (n, A) alone:

    A > 16384 (Apow2 > 16384): multi-launch sort + nms_greedy_kernel (8 waves), any n
    A <= 16384, n <= 16:        nms_sort_greedy_kernel (one launch, greedy pass on 16 waves)
    A <= 16384, n > 16:         nms_sort_kernel + nms_greedy_kernel (8 waves)
    inside a sort kernel: up to 4096 candidates the LDS sort, above it bitonic_sort_hybrid (n2 = 8192: one merge stage, 16384: two)

tests/test_nms_cases.py checks on the CPU that every planted edge is really there and that the inputs tell the reference from
eleven wrong variants (restate(..., flaw=...)); tests/test_gpu_nms.py compares the kernels' words with the reference's."""
import functools

import numpy as np
import torch

from oracle import yolo_oracle as O

F32 = np.float32
ROW_WORDS = 58
CANVAS = (640, 640)
CONF = float(F32(0.3))           # exactly representable: the kernel takes conf and iou as fp32
IOU = float(F32(0.7))

# (h0, w0): 333x500 has box pad 107 (rounded) against keypoint pad 106.88, 200x300 has gain 2.13, 1080x1920 gain 1/3 and equal
# pads, 500x333 is the portrait twin (the x pads differ)
GEOMS = ((333, 500), (200, 300), (1080, 1920), (500, 333))


def geom7(h0, w0, canvas=CANVAS):
    """gain, pad_x, pad_y (scale_boxes: rounded), kpad_x, kpad_y (scale_coords: unrounded), orig_w, orig_h -- in float64 as those
    functions compute them, then cast to fp32 as the engine does when it fills the kernel's arguments"""
    gain = min(canvas[0] / h0, canvas[1] / w0)
    pad_x = round((canvas[1] - w0 * gain) / 2 - 0.1)
    pad_y = round((canvas[0] - h0 * gain) / 2 - 0.1)
    kpad_x, kpad_y = (canvas[1] - w0 * gain) / 2, (canvas[0] - h0 * gain) / 2
    return np.array([gain, pad_x, pad_y, kpad_x, kpad_y, w0, h0], np.float64).astype(F32)


class Case:
    def __init__(self, name, pool, nc, ns, conf=CONF, iou=IOU, classes=None, max_det=300, max_nms=30000, kdim=0, hw=None,
                 table=False, draw_seed=None, pack=False, notes=None):
        self.name, self.pool, self.nc, self.ns = name, [np.ascontiguousarray(p, F32) for p in pool], nc, tuple(ns)
        self.conf, self.iou, self.classes, self.max_det, self.max_nms, self.kdim = conf, iou, classes, max_det, max_nms, kdim
        self.hw, self.table, self.draw_seed, self.pack = hw, table, draw_seed, pack
        self.notes = notes or {}
        self.no, self.A = self.pool[0].shape
        self.extra = self.no - 4 - nc
        assert all(p.shape == (self.no, self.A) and np.isfinite(p).all() for p in self.pool)
        assert hw is None or len(hw) == (len(pool) if table else 1)

    def order(self, n):
        """which pool frame sits at each batch position"""
        if self.draw_seed is None:
            return np.arange(n) % len(self.pool)
        return np.random.default_rng(self.draw_seed + n).integers(0, len(self.pool), n)

    def batch(self, n):
        o = self.order(n)
        return np.ascontiguousarray(np.stack(self.pool)[o]), o

    def geom(self, n, as_table=None):
        """None, the seven scalars, or the [n, 7] table of a batch of n"""
        if self.hw is None:
            return None
        if not (self.table if as_table is None else as_table):
            return geom7(*self.hw[0])
        o = self.order(n)
        return np.stack([geom7(*self.hw[i if self.table else 0]) for i in o])

    def kwargs(self):
        return dict(nc=self.nc, conf=self.conf, iou=self.iou, classes=self.classes, max_det=self.max_det, max_nms=self.max_nms,
                    kdim=self.kdim)

    @functools.lru_cache(maxsize=None)
    def ref(self):
        """per pool frame: (rows [k, 58] uint32, kept anchors [k]) -- the oracle, once"""
        return reference(self)

    def expected_rows(self, n, sentinel):
        """[n, max_det, 58] uint32: the oracle's rows in the first count slots, the sentinel in every other"""
        ref, o = self.ref(), self.order(n)
        want = np.full((n, self.max_det, ROW_WORDS), sentinel, np.uint32)
        counts = np.zeros(n, np.int32)
        for i, f in enumerate(o):
            r = ref[f][0]
            want[i, :len(r)] = r
            counts[i] = len(r)
        return want, counts


def rows_from(x, idx, extra):
    """oracle rows [k, 6+extra] + anchors -> the 58 words of mi355_det: box, score, class as int, anchor, keypoints, zeros"""
    x = np.ascontiguousarray(x, F32)
    rows = np.zeros((len(x), ROW_WORDS), np.uint32)
    rows[:, :5] = x[:, :5].view(np.uint32)
    rows[:, 5] = x[:, 5].astype(np.int32).view(np.uint32)
    rows[:, 6] = np.asarray(idx, np.int32).view(np.uint32)
    if extra:
        rows[:, 7:7 + extra] = np.ascontiguousarray(x[:, 6:6 + extra]).view(np.uint32)
    return rows


def reference(c):
    out, idx = O.non_max_suppression(torch.from_numpy(np.stack(c.pool)), c.conf, c.iou, classes=c.classes, max_det=c.max_det,
                                     nc=c.nc, max_nms=c.max_nms, return_idxs=True)
    res = []
    for f, (x, k) in enumerate(zip(out, idx)):
        x = x.clone()
        if c.hw is not None and len(x):
            hw = c.hw[f if c.table else 0]
            x[:, :4] = O.scale_boxes(CANVAS, x[:, :4].clone(), hw)
            if c.kdim:
                kp = x[:, 6:].reshape(len(x), -1, c.kdim).clone()
                x[:, 6:] = O.scale_coords(CANVAS, kp, hw).reshape(len(x), -1)
        res.append((rows_from(x.numpy(), k.numpy(), c.extra), k.numpy().astype(np.int64)))
    return res


# ------------------------------------------------------------------------------------------------------------ wrong variants
FLAWS = ("iou_ge", "conf_ge", "tie_desc", "no_offset", "transitive", "trunc_after", "max_det_plus", "div_first", "kpt_box_pad",
         "no_clip", "kconf_scaled")


def sorted_candidates(pred, nc, conf, classes=None, max_nms=30000, flaw=None):
    """anchors in the order the greedy pass walks them (stable descending score, cut at max_nms), their scores and classes"""
    p = np.ascontiguousarray(pred.T)
    cls = p[:, 4:4 + nc]
    score, c = cls.max(1), cls.argmax(1)
    cand = score >= F32(conf) if flaw == "conf_ge" else score > F32(conf)
    if classes is not None:
        cand &= np.isin(c, classes)
    an = np.nonzero(cand)[0]
    s = score[an]
    if flaw == "tie_desc":
        order = len(an) - 1 - np.argsort(-s[::-1], kind="stable")
    else:
        order = np.argsort(-s, kind="stable")
    if flaw != "trunc_after":
        order = order[:max_nms]
    an = an[order]
    return an, score[an], c[an]


def xyxy_of(pred, an):
    x = np.ascontiguousarray(pred.T)[an]
    half = x[:, 2:4] / F32(2)
    return np.concatenate([x[:, :2] - half, x[:, :2] + half], 1)


def iou_row(b, area, i, js):
    """fp32 IoU of box i against boxes js, in the kernel's and torchvision's operation order"""
    w = np.maximum(np.minimum(b[i, 2], b[js, 2]) - np.maximum(b[i, 0], b[js, 0]), F32(0))
    h = np.maximum(np.minimum(b[i, 3], b[js, 3]) - np.maximum(b[i, 1], b[js, 1]), F32(0))
    inter = w * h
    with np.errstate(divide="ignore", invalid="ignore"):
        return inter / (area[i] + area[js] - inter)


def restate(pred, nc, conf, iou, classes=None, max_det=300, max_nms=30000, kdim=0, hw=None, flaw=None, trace=None):
    """plain numpy statement of the tail for ONE frame; flaw=None is the reference's arithmetic, every other value one wrong
    variant of it.  -> (rows [k, 58] uint32, kept anchors).  trace (a dict) receives the walk: sorted anchors, kept positions."""
    an, score, c = sorted_candidates(pred, nc, conf, classes, max_nms, flaw)
    box = xyxy_of(pred, an)
    b = box + c.astype(F32)[:, None] * F32(0 if flaw == "no_offset" else 7680)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    m, thr = len(an), F32(iou)
    dead, keep = np.zeros(m, bool), []
    for i in range(m):
        if dead[i] and flaw != "transitive":
            continue
        if not dead[i]:
            keep.append(i)
        if i + 1 == m:
            break
        ovr = iou_row(b, area, i, slice(i + 1, None))
        dead[i + 1:] |= (ovr >= thr) if flaw == "iou_ge" else (ovr > thr)
    if trace is not None:
        trace.update(an=an, b=b, area=area, kept_all=np.asarray(keep, np.int64))
    keep = keep[:max_det + (1 if flaw == "max_det_plus" else 0)]
    if flaw == "trunc_after":
        keep = keep[:max_nms]
    keep = np.asarray(keep, np.int64)
    extra = pred.shape[0] - 4 - nc
    x = np.concatenate([box[keep], score[keep, None], c[keep, None].astype(F32), np.ascontiguousarray(pred.T)[an[keep], 4 + nc:]], 1)
    if hw is not None and len(x):
        gain, pad_x, pad_y, kpad_x, kpad_y, ow, oh = geom7(*hw)

        def back(v, pad, lim):
            v = v / gain - pad if flaw == "div_first" else (v - pad) / gain
            return v if flaw == "no_clip" else np.minimum(np.maximum(v, F32(0)), lim)
        for q, (pad, lim) in enumerate(((pad_x, ow), (pad_y, oh), (pad_x, ow), (pad_y, oh))):
            x[:, q] = back(x[:, q], pad, lim)
        if kdim:
            kp = x[:, 6:].reshape(len(x), -1, kdim)
            px, py = (pad_x, pad_y) if flaw == "kpt_box_pad" else (kpad_x, kpad_y)
            kp[..., 0] = back(kp[..., 0], px, ow)
            kp[..., 1] = back(kp[..., 1], py, oh)
            if kdim == 3 and flaw == "kconf_scaled":
                kp[..., 2] = back(kp[..., 2], px, ow)
            x[:, 6:] = kp.reshape(len(x), -1)
    return rows_from(x.astype(F32), an[keep], extra), an[keep]


# ------------------------------------------------------------------------------------------------------------------ frames
def _blank(rng, A, nc, extra=0):
    """no anchor is a candidate: every class score lies below 0.2; boxes and extras are arbitrary finite values"""
    p = np.empty((4 + nc + extra, A), F32)
    p[0:2] = rng.uniform(20, 620, (2, A))
    p[2:4] = rng.uniform(4, 80, (2, A))
    p[4:4 + nc] = rng.uniform(0.001, 0.2, (nc, A))
    if extra:
        p[4 + nc:] = rng.uniform(-30, 670, (extra, A))
    return p


def _scores(k, lo=0.31, hi=0.99):
    s = np.linspace(hi, lo, k).astype(F32)
    assert len(np.unique(s)) == k
    return s


def cluster_frame(seed, A, ncand, nc=2, spread=6.0):
    """ncand candidates at random anchors, boxes jittered around 49 centres so that most die and the oracle's walk stays short"""
    rng = np.random.default_rng(seed)
    p = _blank(rng, A, nc)
    an = rng.choice(A, ncand, replace=False)
    k = rng.integers(0, 49, ncand)
    p[0, an] = 50 + 90 * (k % 7) + rng.uniform(-spread, spread, ncand)
    p[1, an] = 50 + 90 * (k // 7) + rng.uniform(-spread, spread, ncand)
    p[2, an] = 60 + rng.uniform(-4, 4, ncand)
    p[3, an] = 60 + rng.uniform(-4, 4, ncand)
    p[4 + rng.integers(0, nc, ncand), an] = rng.permutation(_scores(ncand)) if ncand else 0
    return p


def ranked_frame(seed, A, ncand, isolated=(), ties=(), nc=1):
    """candidates by RANK (position in the sorted order): distinct descending scores except inside the tie blocks [a, b); the ranks
    in `isolated` and in the tie blocks are 6x6 boxes alone on a grid (always kept), every other rank falls into one of 8 tight
    clusters (one survivor each).  Anchors are a random permutation, so anchor order and rank order are unrelated."""
    rng = np.random.default_rng(seed)
    p = _blank(rng, A, nc)
    s = _scores(ncand)
    alone = set(r for r in isolated if r < ncand)
    for a, b in ties:
        s[a:b] = s[a]
        alone |= set(range(a, b))
    an = rng.permutation(A)[:ncand]
    k = rng.integers(0, 8, ncand)
    p[0, an] = 60 + 75 * k + rng.uniform(-1, 1, ncand)
    p[1, an] = 100 + rng.uniform(-1, 1, ncand)
    p[2:4, an] = 60 + rng.uniform(-0.5, 0.5, (2, ncand))
    for slot, r in enumerate(sorted(alone)):
        p[:4, an[r]] = (20.25 + 12 * (slot % 50), 400.5 + 12 * (slot // 50), 6, 6)
    p[4, an] = s
    return p, an


def sole_frame(seed=41, A=2048):
    """iou 0.5, one class.  48 kept boxes K_i (ranks 0..47, 40 px apart), 192 fillers that K_(j mod 48) kills, then 48 victims V_i
    (ranks 240..287, K_i shifted by 5 px: IoU 0.6 with K_i, 0 with everything else alive), a chain A > B > C inside one chunk
    (ranks 300..302), one across chunks (ranks 303, 330, 400), fillers between, ten survivors at the end."""
    rng = np.random.default_rng(seed)
    p = _blank(rng, A, 1)
    ncand = 420
    an = rng.permutation(A)[:ncand]
    s = _scores(ncand)
    kbox = lambda i: np.array([30.0 + 40 * (i % 12), 30.0 + 40 * (i // 12), 20, 20], F32)
    special = {300: (120, 320, 40, 40), 301: (130, 320, 40, 40), 302: (140, 320, 40, 40),
               303: (320, 320, 40, 40), 330: (330, 320, 40, 40), 400: (340, 320, 40, 40)}
    for r in range(ncand):
        if r < 48:
            box = kbox(r)
        elif 240 <= r < 288:
            box = kbox(r - 240) + F32([5, 0, 0, 0])
        elif r in special:
            box = F32(special[r])
        elif r >= 410:
            box = F32([30 + 30 * (r - 410), 500, 12, 12])
        else:
            box = kbox(r % 48) + np.concatenate([rng.uniform(-0.5, 0.5, 2), [0, 0]]).astype(F32)
        p[:4, an[r]] = box
    p[4, an] = s
    return p


def maxdet_frame(seed, dup_every=0, A=2048, alone=1100):
    """1100 boxes of 4x4, 8 px apart (each kept); with dup_every = 3 every third candidate in rank order is an exact copy of an
    earlier one (dies), so the kept count and the chunk position run apart"""
    rng = np.random.default_rng(seed)
    p = _blank(rng, A, 1)
    boxes, src = [], []
    while len(src) < alone:
        if dup_every and len(boxes) % dup_every == dup_every - 1:
            boxes.append(boxes[rng.integers(0, len(boxes))])
        else:
            i = len(src)
            boxes.append((10.5 + 8 * (i % 75), 10.25 + 8 * (i // 75), 4, 4))
            src.append(i)
    an = rng.permutation(A)[:len(boxes)]
    p[:4, an] = np.asarray(boxes, F32).T
    p[4, an] = _scores(len(boxes))
    return p


def threshold_frame(A=256):
    """iou 0.5, conf 0.3, two classes; integer coordinates so every IoU is exact"""
    rng = np.random.default_rng(7)
    p = _blank(rng, A, 2)
    plan = {}                                     # name -> anchor
    items = [  # name, (cx, cy, w, h), score, class
        ("exact_a", (115, 105, 30, 10), 0.95, 0), ("exact_b", (125, 105, 30, 10), 0.94, 0),          # shifted by 10: IoU 200/400
        ("exact1_a", (115, 135, 30, 10), 0.93, 1), ("exact1_b", (125, 135, 30, 10), 0.92, 1),        # the same under the class offset
        ("close_a", (215, 105, 30, 10), 0.91, 0), ("close_b", (224, 105, 30, 10), 0.90, 0),          # shifted by 9: IoU 210/390
        ("at_conf", (300, 300, 20, 20), CONF, 0),
        ("above_conf", (340, 300, 20, 20), float(np.nextafter(F32(CONF), F32(1))), 0),
        ("two_cls_a", (400, 100, 40, 40), 0.80, 0), ("two_cls_b", (400, 100, 40, 40), 0.79, 1),
        ("one_cls_a", (500, 100, 40, 40), 0.78, 1), ("one_cls_b", (500, 100, 40, 40), 0.77, 1),
        ("zero_a", (100, 400, 0, 0), 0.70, 0), ("zero_b", (100, 400, 0, 0), 0.69, 0),                # 0/0: NaN > thr is false
        ("flat_a", (200, 400, 0, 30), 0.68, 0), ("flat_b", (200, 400, 0, 30), 0.67, 0),
    ]
    for (name, box, sc, cls), an in zip(items, rng.permutation(A)):
        p[:4, an] = box
        p[4 + cls, an] = sc
        plan[name] = int(an)
    return p, plan


def class_frame(nc, A=256, seed=9, skip=()):
    """two isolated candidates of every class but those in `skip`"""
    rng = np.random.default_rng(seed)
    p = _blank(rng, A, nc)
    an = rng.permutation(A)[:2 * nc]
    s = rng.permutation(_scores(2 * nc))
    for i, a in enumerate(an):
        p[:4, a] = (20.5 + 30 * (i % 20), 20.5 + 30 * (i // 20), 10, 10)
        if i % nc not in skip:
            p[4 + i % nc, a] = s[i]
    return p


def scale_frame(seed, hw, extra, kdim, A=256, ncand=40):
    """isolated candidates whose boxes and keypoints fall below 0, above the frame, exactly on the pads and inside it"""
    rng = np.random.default_rng(seed)
    p = _blank(rng, A, 1, extra)
    gain, pad_x, pad_y, kpad_x, kpad_y, ow, oh = (float(v) for v in geom7(*hw))
    an = rng.permutation(A)[:ncand]
    s = rng.permutation(_scores(ncand))
    right, bottom = pad_x + ow * gain, pad_y + oh * gain
    for i, a in enumerate(an):
        cell = i + 12                                                             # 75 x 90 cells from y = 190 on, boxes at most 60: alone
        cx, cy = 40.5 + 75 * (cell % 8), 40.25 + 90 * (cell // 8)
        w, h = rng.uniform(20, 60, 2)
        if i == 0:
            cx, cy, w, h = pad_x + 20, 40.25, 40, 40                              # x1 exactly on the box pad
        if i == 1:
            cx, cy, h = 300.5, pad_y + 15, 30                                     # y1 exactly on the box pad
        if i == 2:
            cx, cy, w, h = right + 5, bottom + 5, 50, 50                          # x2, y2 beyond the frame
        if i == 3:
            cx, cy, w, h = pad_x - 5, pad_y - 5, 40, 40                           # x1, y1 below 0
        p[:4, a] = (cx, cy, w, h)
        p[4, a] = s[i]
        if kdim:
            kp = p[5:, a].reshape(-1, kdim)
            kp[:, 0] = rng.uniform(pad_x - 40, right + 40, len(kp))
            kp[:, 1] = rng.uniform(pad_y - 40, bottom + 40, len(kp))
            if kdim == 3:
                kp[:, 2] = rng.uniform(0.01, 0.99, len(kp))
            kp[0, :2] = (F32(kpad_x), F32(kpad_y))                                # exactly on the keypoint pads
            if len(kp) > 1:
                kp[1, :2] = (pad_x, pad_y)                                        # on the BOX pads: 0 only where the two agree
            p[5:, a] = kp.reshape(-1)
    return p


def compaction_pool(A=32):
    """frames that keep 0, 1, .. 8 rows at max_det 8, one with 12 live boxes (cut at 8), one whose duplicates die"""
    pool = []
    for k in (0, 1, 2, 3, 5, 7, 8, 12):
        rng = np.random.default_rng(100 + k)
        p = _blank(rng, A, 1)
        an = rng.permutation(A)[:k]
        p[:4, an] = np.asarray([(20.5 + 40 * i, 30.5, 10, 10) for i in range(k)], F32).reshape(k, 4).T
        p[4, an] = rng.permutation(_scores(12))[:k]
        pool.append(p)
    rng = np.random.default_rng(99)
    p = _blank(rng, A, 1)
    p[:4, :20] = np.asarray([(20.5 + 40 * (i % 4), 30.5, 10, 10) for i in range(20)], F32).T     # 4 kept, 16 die
    p[4, :20] = rng.permutation(_scores(20))
    pool.append(p)
    return pool


# ------------------------------------------------------------------------------------------------------------------- cases
NS = (1, 16, 17, 33)
PATH_POOLS = {2048: (2048, 0, 1, 63, 64, 65), 5000: (5000, 4097, 0, 100), 16384: (9000, 0, 5000), 16385: (16385, 0, 100, 4096, 4097)}
MAX_DETS = (1, 7, 64, 300, 1024)
TRUNC = {2048: 2048, 5000: 5000, 16385: 9000}            # A -> candidates: LDS sort, hybrid, multi-launch
CUT_RANKS = (63, 64, 999, 1000, 4095, 4096)
TIES = {2048: ((56, 72), (1016, 1033)), 5000: ((56, 72), (4088, 4105)), 16385: ((56, 72), (4088, 4105), (8190, 8195))}


def _paths(A):
    return Case(f"paths_{A}", [cluster_frame(1000 + A + i, A, k) for i, k in enumerate(PATH_POOLS[A])], 2, NS,
                notes=dict(counts=PATH_POOLS[A]))


def _order(A):
    p, an = ranked_frame(2000 + A, A, TRUNC[A], ties=TIES[A])
    return Case(f"order_{A}", [p], 1, (1, 17), notes=dict(ties=TIES[A], ranked=an))


def _trunc(A, max_nms):
    p, an = ranked_frame(3000 + A, A, TRUNC[A], isolated=CUT_RANKS)
    return Case(f"trunc_{A}_{max_nms}", [p], 1, (1, 17), max_nms=max_nms, notes=dict(ranked=an))


def _maxdet(kind, max_det):
    return Case(f"maxdet_{kind}_{max_det}", [maxdet_frame(50, 0 if kind == "plain" else 3)], 1, (1, 17), max_det=max_det)


def _thresholds():
    p, plan = threshold_frame()
    return Case("thresholds", [p], 2, (1, 17), iou=0.5, notes=dict(plan=plan))


def _scale(name, extra, kdim, hw_i=0, table=False):
    if table:
        hw = GEOMS
        pool = [scale_frame(600 + i, g, extra, kdim) for i, g in enumerate(GEOMS)]
    else:
        hw = (GEOMS[hw_i],)
        pool = [scale_frame(500 + extra + s, GEOMS[hw_i], extra, kdim) for s in range(2)]
    return Case(name, pool, 1, (4, 17), kdim=kdim, hw=hw, table=table)


BUILDERS = {}
for _A in PATH_POOLS:
    BUILDERS[f"paths_{_A}"] = functools.partial(_paths, _A)
for _A in TRUNC:
    BUILDERS[f"order_{_A}"] = functools.partial(_order, _A)
    for _m in (64, 1000, 4096):
        BUILDERS[f"trunc_{_A}_{_m}"] = functools.partial(_trunc, _A, _m)
BUILDERS["sole"] = lambda: Case("sole", [sole_frame()], 1, (1, 16, 17), iou=0.5)
for _k in ("plain", "dups"):
    for _m in MAX_DETS:
        BUILDERS[f"maxdet_{_k}_{_m}"] = functools.partial(_maxdet, _k, _m)
BUILDERS["thresholds"] = _thresholds
BUILDERS["classes_70"] = lambda: Case("classes_70", [class_frame(70)], 70, (1, 17), classes=[0, 31, 32, 69])
BUILDERS["classes_80"] = lambda: Case("classes_80", [class_frame(80)], 80, (1,), classes=[31, 32, 79])
BUILDERS["classes_none"] = lambda: Case("classes_none", [class_frame(70, skip=(40,))], 70, (1, 17), classes=[40])
BUILDERS["scale_pose51"] = functools.partial(_scale, "scale_pose51", 51, 3, 0)
BUILDERS["scale_pose34_gain2"] = functools.partial(_scale, "scale_pose34_gain2", 34, 2, 1)
BUILDERS["scale_kpt4"] = functools.partial(_scale, "scale_kpt4", 4, 2, 3)
BUILDERS["scale_extra4_no_kpts"] = functools.partial(_scale, "scale_extra4_no_kpts", 4, 0, 0)
BUILDERS["scale_detect"] = functools.partial(_scale, "scale_detect", 0, 0, 2)
BUILDERS["scale_table"] = functools.partial(_scale, "scale_table", 51, 3, 0, True)
COMPACT_NS = (1, 2, 1023, 1024, 1025, 2500)
BUILDERS["compact"] = lambda: Case("compact", compaction_pool(), 1, COMPACT_NS, max_det=8, draw_seed=77, pack=True)

CASES = tuple(BUILDERS)
# (case, n) of every GPU run, known without building a case
RUN_NS = {name: (NS if name.startswith("paths_") else (1, 16, 17) if name == "sole" else COMPACT_NS if name == "compact" else
                 (1,) if name == "classes_80" else (4, 17) if name.startswith("scale_") else (1, 17)) for name in CASES}
RUNS = tuple((name, n) for name in CASES for n in RUN_NS[name])
# what the wrong variants are tried on: every case whose walk is short
SMALL = ("thresholds", "sole", "order_2048", "trunc_2048_64", "maxdet_dups_7", "scale_pose51", "scale_table")


@functools.lru_cache(maxsize=None)
def case(name):
    c = BUILDERS[name]()
    assert c.name == name and c.ns == RUN_NS[name], (name, c.ns)
    return c
