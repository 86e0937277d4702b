"""Float64 restatement of openmpl_amd.triangulate_rays_robust and the inputs of its tests (TEST INFRASTRUCTURE ONLY).

numpy float64 on the float32 inputs the kernel reads, item by item, in the three stages of the call: candidates (the view selection
of the reference's multiviews/triangulate.py:94-102, pinned by tests/golden/triangulate_select.npz, which the reference's own
triangulate_poses produced), pair consensus, refit (tests/geometry_cases.triangulate on the inlier set).

The consensus takes discrete decisions -- is a view within tau, which hypothesis wins -- that a last-bit difference between two
float64 implementations could turn round.  outlier_case() therefore asserts margins on its own data: every candidate's distance
to every hypothesis is further than 1e-8 tau from tau, and two hypotheses of one item with the same count differ in cost by more
than 1e-8 (relative).  Two fp64 implementations differ near 1e-12, so `inliers` can be compared exactly.  No item is left out: a
seed whose case misses a margin is not used.  The cost margin is asked of hypotheses that count two views or more.  Below that
no output depends on the order (min_inliers is at least 2: whichever of them wins, the joint is NaN and its inliers are 0), and
without confidences every hypothesis that counts no view costs exactly n tau^2, a tie no data can avoid.
"""
import os

import numpy as np

from tests import geometry_cases as gc

TAU = 0.08               # metres; the detections of outlier_case carry 0.02 m of noise
MARGIN = 1e-8


def golden_select():
    g = np.load(os.path.join(gc.GOLD, "triangulate_select.npz"))
    return {k: g[k] for k in g.files}


def participation(w):
    """(..., ) float64 -> bool: a view with conf <= 0 or a non-finite conf never takes part"""
    with np.errstate(invalid="ignore"):
        return np.isfinite(w) & (w > 0)


def select(conf, conf_threshold):
    """triangulate.py:94-102 on the V confidences of one joint, literally (the threshold comes down by repeated subtraction)"""
    th = float(conf_threshold)
    with np.errstate(invalid="ignore"):
        while True:
            sel = conf > th
            if th < -1:
                break
            if sel.sum() <= 1:
                th -= 0.05
            else:
                break
    return sel


def pair_point(c, d, i, k):
    """the equal-weight least-squares point of lines i and k (the midpoint of their common perpendicular), solved about the mean
    of the two centres; None where det(A / 2) < DET_MIN"""
    cm = 0.5 * (c[i] + c[k])
    M = [np.eye(3) - np.outer(d[v], d[v]) for v in (i, k)]
    A = M[0] + M[1]
    if not np.linalg.det(A / 2.0) >= gc.DET_MIN:
        return None
    return cm + np.linalg.solve(A, M[0] @ (c[i] - cm) + M[1] @ (c[k] - cm))


def consensus(c, d, w, cand, tau, margins=None):
    """c, d (V,3), w (V,), cand bool (V,) -> (count, inlier mask) of the winning hypothesis, (-1, zeros) without one"""
    V = len(w)
    idx = np.nonzero(cand)[0]
    best, scored = None, []
    for a, i in enumerate(idx):
        for k in idx[a + 1:]:
            x = pair_point(c, d, i, k)
            if x is None:
                continue
            dist = gc.point_line_distance(x, c[idx], d[idx])
            inl = dist <= tau
            count, cost = int(inl.sum()), float(np.sum(w[idx] * np.minimum(dist * dist, tau * tau)))
            scored.append((count, cost))
            if margins is not None:
                margins["dist"] = min(margins["dist"], float(np.abs(dist - tau).min() / tau))
            key = (-count, cost, i, k)                    # highest count, lowest cost, lowest i, lowest k
            if best is None or key < best[0]:
                mask = np.zeros(V, bool)
                mask[idx[inl]] = True
                best = (key, count, mask)
    if margins is not None:
        scored.sort()
        for (n0, c0), (n1, c1) in zip(scored, scored[1:]):
            if n0 == n1 and n0 >= 2:
                margins["cost"] = min(margins["cost"], abs(c1 - c0) / max(c0, c1) if max(c0, c1) > 0 else 0.0)
    return (-1, np.zeros(V, bool)) if best is None else best[1:]


def robust(rays, centers, conf=None, threshold=None, conf_threshold=None, min_inliers=2, margins=None):
    """-> points (B,J,3), residual (B,J) float64, inliers (B,V,J) float32 of 0 / 1.  `margins`: a dict(dist=inf, cost=inf) that
    receives the smallest relative distance of a decision to its threshold"""
    c, d = gc.lines(rays, centers)
    V, B, J, _ = d.shape
    w_all = gc.confidence(conf, V, B, J)
    if conf_threshold is not None and conf is None:
        raise RuntimeError("conf_threshold needs conf")
    part = participation(w_all)
    inl = np.zeros((V, B, J), bool)
    for b in range(B):
        for j in range(J):
            cand = part[:, b, j].copy()
            if conf_threshold is not None:
                cand &= select(w_all[:, b, j], conf_threshold)
            if cand.sum() < 2:
                continue
            if threshold is not None:
                count, mask = consensus(c[:, b, 0], d[:, b, j], w_all[:, b, j], cand, float(threshold), margins)
                if count < min_inliers:
                    continue
                cand = mask
            inl[:, b, j] = cand
    w = np.where(inl, w_all, 0.0)                          # the refit: the same normal equations over the inlier set
    x, res = gc.triangulate(rays, centers, [w[v] for v in range(V)])
    inl &= ~np.isnan(res)[None]                            # a degenerate refit leaves no inliers either
    return x, res, np.ascontiguousarray(np.transpose(inl, (1, 0, 2))).astype(np.float32)


def outlier_case(B, V, J, n_out, seed=0, exact=False, n_zero=0, configs=((False, None), (True, None), (True, 0.5))):
    """geometry_cases.ring_case (0.02 m of noise, or exact lines) with n_out views of every item redirected: they look at a point
    0.4 .. 1.0 m from the item's point, perpendicular to their own line of sight (so the line misses the point by that much).
    n_zero confidences (at random places) are 0.  -> the ring_case dict + out (B,V,J) bool, tau.
    Asserts the margins of the module docstring for every (with conf, conf_threshold) of `configs`."""
    case = gc.ring_case(B, V, J, seed=seed, exact=exact)
    rs = np.random.RandomState(seed * 104729 + B * 1009 + V * 31 + J)
    out = np.zeros((B, V, J), bool)
    for b in range(B):
        for j in range(J):
            out[b, rs.permutation(V)[:n_out], j] = True
    for v in range(V):
        cen = case["centers"][v].astype(np.float64)                   # (B,1,3)
        los = case["points"] - cen
        los /= np.linalg.norm(los, axis=-1, keepdims=True)
        off = rs.randn(B, J, 3)
        off -= np.sum(off * los, axis=-1, keepdims=True) * los
        off *= rs.uniform(0.4, 1.0, size=(B, J, 1)) / np.linalg.norm(off, axis=-1, keepdims=True)
        u = case["points"] + off - cen
        u = u / np.linalg.norm(u, axis=-1, keepdims=True) * rs.uniform(1.0, 2.0, size=(B, J, 1))
        case["rays"][v] = np.where(out[:, v, :, None], (cen + u).astype(np.float32), case["rays"][v])
    if n_zero:
        flat = case["conf"].reshape(-1)
        flat[rs.permutation(flat.size)[:n_zero]] = 0.0
    case.update(out=out, tau=TAU)
    for with_conf, cth in configs:
        m = dict(dist=np.inf, cost=np.inf)
        robust(case["rays"], case["centers"], [case["conf"][v] for v in range(V)] if with_conf else None, TAU, cth, margins=m)
        assert m["dist"] > MARGIN and m["cost"] > MARGIN, ("seed %d of (%d,%d,%d) misses a margin" % (seed, B, V, J), with_conf, cth, m)
        case.setdefault("margins", []).append((with_conf, cth, m["dist"], m["cost"]))
    return case
