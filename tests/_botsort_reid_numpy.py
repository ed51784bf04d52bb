"""Checker of BoT-SORT's appearance half (csrc/tracker_host.cpp with ``with_reid``): ``oracle.tracker_oracle.BYTETracker``, imported
unchanged, plus the feature bookkeeping of ``BOTrack`` and the cost of ``BOTSORT.get_dists`` (ultralytics 8.3.225, restated; SURVEY.md
Appendix A.8).

The arithmetic orders are the ones the C++ states, written out in plain Python floats (= IEEE float64) so that nothing depends on how
numpy or BLAS associates a reduction:

- ``sum_sq(f)`` / ``dot(a, b)``: ascending index, each fp32 value widened to float64 (every product is then exact), a float64 accumulator.
- ``curr_feat = f / float32(sqrt(sum_sq(f)))`` in fp32; a zero-norm feature stays zeros.
- ``smooth_feat``: the first ``curr_feat``; after every later match ``float32(0.9) * smooth + float32(1 - 0.9) * curr`` in fp32 (two
  products, one sum), then brought back to unit length as above.
- ``emb = max(0, 1 - dot / (sqrt(sum_sq(a)) * sqrt(sum_sq(b)))) / 2`` in float64; 1 when either vector is missing or has no length.
- ``get_dists``: ``mask = iou_cost > float32(1 - proximity_thresh)`` on the fp32 IoU cost before the fusion; the fused cost as the oracle
  computes it; ``emb > 1 - appearance_thresh -> 1``; ``emb[mask] = 1``; ``min(fused, emb)``.  Stages 1 and 3 only (the ones that fuse).

How it hooks into the oracle without touching it: ``update`` calls ``self._cost(tracks, dets, fuse)`` once per stage, with ``fuse`` true
exactly in stages 1 and 3, and ``self._detections`` for the strong and the weak set; both are overridden here.  A track's feature
update is applied after the oracle's ``update`` returns: a track matched (or born) on this frame has ``seen == frame`` and ``idx`` = the
row of the detection it absorbed.  That is equivalent to updating inside each stage because the pool (stages 1, 2) and the tracks
awaiting confirmation (stage 3) are disjoint and a track is matched at most once per frame, so no cost of this frame reads a feature
this frame wrote.
"""
import math

import numpy as np

from oracle import tracker_oracle as O

ALPHA = np.float32(0.9)
ONE_MINUS_ALPHA = np.float32(1.0 - 0.9)


def sum_sq(f) -> float:
    acc = 0.0
    for v in f:
        acc += float(v) * float(v)
    return acc


def dot(a, b) -> float:
    acc = 0.0
    for x, y in zip(a, b):
        acc += float(x) * float(y)
    return acc


def unit_length(f: np.ndarray) -> np.ndarray:
    f = np.asarray(f, np.float32)
    norm = np.float32(math.sqrt(sum_sq(f)))
    return (f / norm).astype(np.float32) if norm > 0 else f.copy()


def embedding_cost(a, b) -> float:
    if a is None or b is None:
        return 1.0
    na, nb = sum_sq(a), sum_sq(b)
    if na == 0.0 or nb == 0.0:
        return 1.0
    return max(0.0, 1.0 - dot(a, b) / (math.sqrt(na) * math.sqrt(nb))) / 2.0


def smooth_update(smooth, curr: np.ndarray) -> np.ndarray:
    if smooth is None:
        return curr.copy()
    mixed = (ALPHA * smooth).astype(np.float32) + (ONE_MINUS_ALPHA * curr).astype(np.float32)
    return unit_length(mixed.astype(np.float32))


class BOTSORT(O.BYTETracker):
    def __init__(self, frame_rate: int = 30, gmc_method=None, with_reid: bool = True, proximity_thresh: float = 0.5,
                 appearance_thresh: float = 0.8):
        super().__init__(frame_rate, gmc_method)
        self.with_reid, self.proximity_thresh, self.appearance_thresh = with_reid, float(proximity_thresh), float(appearance_thresh)
        self._curr = None                     # this frame's curr_feat per detection row, or None

    def _detections(self, det, keep):
        out = super()._detections(det, keep)
        for d in out:
            d.feat = None if self._curr is None else self._curr[int(d.idx)]
        return out

    def _cost(self, tracks, dets, fuse):
        iou = O._iou_cost([t.xyxy for t in tracks], [d.xyxy for d in dets])
        cost = O.BYTETracker._cost(tracks, dets, fuse)
        if not (fuse and self._curr is not None and cost.size):
            return cost
        cost = np.array(cost, dtype=np.float64)
        gate = np.float32(1.0 - self.proximity_thresh)
        for i, t in enumerate(tracks):
            for j, d in enumerate(dets):
                emb = embedding_cost(getattr(t, "smooth_feat", None), d.feat)
                if emb > 1.0 - self.appearance_thresh:
                    emb = 1.0
                if np.float32(iou[i, j]) > gate:
                    emb = 1.0
                cost[i, j] = min(float(cost[i, j]), emb)
        return cost

    def update(self, det, img=None, warp=None, feats=None):
        det = np.asarray(det, dtype=np.float32).reshape(-1, 6)
        self._curr = None
        if self.with_reid and feats is not None:
            self._curr = [unit_length(f) for f in np.asarray(feats, np.float32)]
        rows = super().update(det, img, warp)
        if self._curr is not None:
            for t in self._live:              # every track matched or born on this frame is in the new live list
                if t.seen == self.frame_id:
                    t.smooth_feat = smooth_update(getattr(t, "smooth_feat", None), self._curr[int(t.idx)])
        return rows
