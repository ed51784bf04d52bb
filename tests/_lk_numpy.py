"""The float64 statement of pyramidal Lucas-Kanade (oracle/gmc_oracle.py:calc_optical_flow_pyr_lk), traced: the same helpers, the same
expressions in the same order -- (next, status) are the committed function's bit for bit, which tests/test_lk_cases.py asserts on
every case -- and per point what the committed function does not say:

    exit    how the point left level 0 (START_OUTSIDE .. FINAL_OUT below)
    iters   iterations it ran at level 0
    skipped whether a level above 0 rejected its window (the point goes on at the level below, from where it stood)
    walk    its longest walk inside one level, in whole pixels of the window's corner: max over levels and iterations of
            |floor(clip(q) - half) - floor(clip(q_first) - half)| (Chebyshev).  The kernel's LDS region holds kMargin = 3 pixels round
            the corner it was filled at, so walk > 3 means the region was refilled.
    margin  the smallest relative margin over every decision that depends on a window sum or an iterated position, at every level
            (an upper level's decision moves the point's path): mineig >= min_eig, det >= FLT_EPSILON, dx^2 + dy^2 <= eps^2, the
            oscillation conjunction against 0.01, floor(q - half) against -win / w / h for iterated q, and the final in-frame test of a
            point that is still kept and has moved.

The margin of ``a`` against threshold ``t`` is |a - t| / max(|a|, |t|) for the sums, and |a - t| / max(|a|, |t|, 1) for positions in
pixels (against 0 the pure ratio is 1 for every a, which says nothing).  A conjunction that holds has the smaller of its terms' margins;
one that fails has the LARGEST margin among its failing terms (all of them must flip to change it).  Decisions on start positions
(p0 / 2^l - half: an exact division by a power of two) are exact in float64 and carry no margin; so do the decisions of an iteration
whose difference patch is zero in every element (zero motion): its sums are exact zeros in any association.

``assoc=1`` forms the five window sums over the reversed, transposed window -- another association of the same terms, to probe
conditioning only; so does ``nudge``, which moves every start position by that many pixels in x and y."""
import numpy as np

from oracle import gmc_oracle as G

START_OUTSIDE, REJECTED, LEFT_WINDOW, CONVERGED, OSCILLATION, MAX_ITERS, FINAL_OUT = range(7)
EXIT_NAMES = ("start outside", "rejected window", "left the window", "converged", "oscillation", "max_iters", "final position out of frame")
# REJECTED covers both window tests.  det >= FLT_EPSILON cannot fail alone at min_eig >= 1e-4: mineig = l2 / win^2 with l2 <= l1 the
# eigenvalues of the 2x2 matrix, so mineig >= 1e-4 means det = l1 l2 >= (9e-4)^2 = 8.1e-7 > FLT_EPSILON for every window >= 3.
FLT_EPSILON = float(np.finfo(np.float32).eps)


def _rel(a, t, floor=0.0):
    a = np.asarray(a, np.float64)
    den = np.maximum(np.maximum(np.abs(a), abs(t)), floor)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(den > 0, np.abs(a - t) / den, 0.0)


def _wsum(x, assoc):
    if assoc == 0:
        return x.sum((1, 2))
    return np.ascontiguousarray(x[:, ::-1, ::-1].transpose(0, 2, 1)).sum((1, 2))


def _window_margin(v, win, n):
    """floor(v) >= -win and floor(v) < n  <=>  -win <= v < n: v's distance to both ends, relative (positions: floor 1)"""
    return np.minimum(_rel(v, -win, 1.0), _rel(v, n, 1.0))


def lk_traced(prev, cur, pts, win=G.LK_WIN, levels=G.LK_LEVELS, max_iters=G.LK_MAX_ITERS, eps=G.LK_EPS, min_eig=G.LK_MIN_EIG, assoc=0,
              nudge=0.0):
    """-> dict(next float32 [n, 2], next64 (before the cast), status bool [n], exit, iters, walk int [n], margin float64 [n],
    skipped bool [n], top int)"""
    n = len(pts)
    pyr_p, pyr_c = [prev], [cur]
    for _ in range(levels):
        nh, nw = (pyr_p[-1].shape[0] + 1) // 2, (pyr_p[-1].shape[1] + 1) // 2
        if nh <= win or nw <= win:
            break
        pyr_p.append(G._pyr_down(pyr_p[-1]))
        pyr_c.append(G._pyr_down(pyr_c[-1]))
    top = len(pyr_p) - 1
    pad = win + 2
    half = win // 2
    status = np.ones(n, bool)
    nxt = np.zeros((n, 2), np.float64)
    p0 = pts.astype(np.float64) + nudge
    exit_ = np.full(n, -1, np.int64)
    iters = np.zeros(n, np.int64)
    walk = np.zeros(n, np.int64)
    margin = np.full(n, np.inf)
    skipped = np.zeros(n, bool)

    def lower(idx, m):
        margin[idx] = np.minimum(margin[idx], m)

    for lvl in range(top, -1, -1):
        ip, ic = pyr_p[lvl], pyr_c[lvl]
        h, w = ip.shape
        dx, dy = G._scharr(ip)
        ipp, dxp, dyp, icp = (G._pad101(a.astype(np.float64), pad) for a in (ip, dx, dy, ic))
        pl = p0 / (1 << lvl)
        nl = pl.copy() if lvl == top else nxt * 2.0
        tl = np.floor(pl - half)
        inside = (tl[:, 0] >= -win) & (tl[:, 0] < w) & (tl[:, 1] >= -win) & (tl[:, 1] < h)
        if lvl == 0:
            status &= inside
            exit_[~inside] = START_OUTSIDE
        act = np.nonzero(inside)[0]
        if len(act):
            lo, hi = [-half, -half], [w - 1 + half, h - 1 + half]
            plc = np.clip(pl[act], lo, hi)
            I = G._patches(ipp, plc, pad, win)
            Ix = G._patches(dxp, plc, pad, win)
            Iy = G._patches(dyp, plc, pad, win)
            s = 1.0 / (1 << 20)
            a11, a12, a22 = _wsum(Ix * Ix, assoc) * s, _wsum(Ix * Iy, assoc) * s, _wsum(Iy * Iy, assoc) * s
            det = a11 * a22 - a12 * a12
            mineig = (a22 + a11 - np.sqrt((a11 - a22) ** 2 + 4 * a12 * a12)) / (2 * win * win)
            ok_e, ok_d = mineig >= min_eig, det >= FLT_EPSILON
            good = ok_e & ok_d
            m_e, m_d = _rel(mineig, min_eig), _rel(det, FLT_EPSILON)
            lower(act, np.where(good, np.minimum(m_e, m_d), np.maximum(np.where(ok_e, 0.0, m_e), np.where(ok_d, 0.0, m_d))))
            if lvl == 0:
                status[act[~good]] = False
                exit_[act[~good]] = REJECTED
            else:
                skipped[act[~good]] = True
            idx = act[good]
            I, Ix, Iy = I[good], Ix[good], Iy[good]
            a11, a12, a22, det = a11[good], a12[good], a22[good], det[good]
            cur_pts = nl[idx].copy()
            prev_delta = np.zeros((len(idx), 2))
            live = np.ones(len(idx), bool)
            first = np.floor(np.clip(cur_pts, lo, hi) - half)
            if lvl == 0:
                exit_[idx] = MAX_ITERS                              # unless one of the loop's exits is taken
            for it in range(max_iters):
                if not live.any():
                    break
                li = np.nonzero(live)[0]
                q = cur_pts[li]
                tlq = np.floor(q - half)
                inq = (tlq[:, 0] >= -win) & (tlq[:, 0] < w) & (tlq[:, 1] >= -win) & (tlq[:, 1] < h)
                m_w = np.minimum(_window_margin(q[:, 0] - half, win, w), _window_margin(q[:, 1] - half, win, h))
                exact = (q == pl[idx[li]]).all(1)                   # still the start position: the test above, exact
                lower(idx[li], np.where(exact, np.inf, m_w))
                if lvl == 0:
                    status[idx[li[~inq]]] = False
                    exit_[idx[li[~inq]]] = LEFT_WINDOW
                live[li[~inq]] = False
                li = li[inq]
                if not len(li):
                    break
                qc = np.clip(cur_pts[li], lo, hi)
                walk[idx[li]] = np.maximum(walk[idx[li]], np.abs(np.floor(qc - half) - first[li]).max(1).astype(np.int64))
                diff = (G._patches(icp, qc, pad, win) - I[li]) * 32.0
                b1, b2 = _wsum(diff * Ix[li], assoc) * s, _wsum(diff * Iy[li], assoc) * s
                dxy = np.stack([(a12[li] * b2 - a22[li] * b1) / det[li], (a12[li] * b1 - a11[li] * b2) / det[li]], axis=1)
                cur_pts[li] += dxy
                zero = ~diff.any((1, 2))                            # every element zero: the sums are exact in any association
                d2 = (dxy * dxy).sum(1)
                done = d2 <= eps * eps
                m = _rel(d2, eps * eps)
                if it > 0:
                    t = np.abs(dxy + prev_delta[li])
                    below = t < 0.01
                    m_t = np.stack([_rel(t[:, 0], 0.01), _rel(t[:, 1], 0.01)], axis=1)
                    both = below.all(1)
                    m_o = np.where(both, m_t.min(1), np.where(below, 0.0, m_t).max(1))
                    osc = both & ~done
                    cur_pts[li[osc]] -= dxy[osc] * 0.5
                    m = np.where(done, m, np.minimum(m, m_o))       # the conjunction is read only when the step was not small enough
                    done |= osc
                    if lvl == 0:
                        exit_[idx[li[osc]]] = OSCILLATION
                lower(idx[li], np.where(zero, np.inf, m))
                if lvl == 0:
                    exit_[idx[li[done & (exit_[idx[li]] != OSCILLATION)]]] = CONVERGED
                    iters[idx[li]] = it + 1
                prev_delta[li] = dxy
                live[li[done]] = False
            nl[idx] = cur_pts
        nxt = nl
    if status.any():
        h, w = prev.shape
        out = (nxt[:, 0] < 0) | (nxt[:, 1] < 0) | (nxt[:, 0] >= w) | (nxt[:, 1] >= h)
        judged = status & (nxt != p0).any(1)                    # a point that never moved is judged on its start position: exact
        m_f = np.minimum(np.minimum(_rel(nxt[:, 0], 0.0, 1.0), _rel(nxt[:, 0], w, 1.0)), np.minimum(_rel(nxt[:, 1], 0.0, 1.0), _rel(nxt[:, 1], h, 1.0)))
        lower(np.nonzero(judged)[0], m_f[judged])
        exit_[status & out] = FINAL_OUT
        status &= ~out
    return {"next": nxt.astype(np.float32), "next64": nxt, "status": status, "exit": exit_, "iters": iters, "walk": walk, "margin": margin, "skipped": skipped,
            "top": top}
