"""Float64 restatement of openmpl_amd/geometry.py and the inputs of its tests (TEST INFRASTRUCTURE ONLY).

numpy float64 on the float32 inputs the kernels read.  The epipolar part is pinned by tests/golden/geometry.npz, which the
reference's own find_3_points_on_ray, cam_to_world, distance_between_two_skew_lines and smart_pseudo_remove_weight produced
(tests/golden/make_golden_geometry.py); the triangulation is the weighted least-squares point of the lines, stated directly.
"""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DET_MIN = 1e-10          # det(A / sum w) below this: degenerate (two views: sin^2(angle) / 4)
PARALLEL = 1e-20         # |d_i x d_k|^2 below this: the pair takes the point-to-line distance


def golden():
    g = np.load(os.path.join(GOLD, "geometry.npz"))
    return {k: g[k] for k in g.files}


def golden_case(g, tag):
    """-> dict(rays, centers: lists of V float32 arrays; conf (V,B,J); weight (V,B,J); pairs, err, weights_out, threshold)"""
    V = int(tag[1:])
    rays, centers = g[tag + "_rays"], g[tag + "_centers"]
    return dict(rays=[rays[v] for v in range(V)], centers=[centers[v] for v in range(V)], conf=g[tag + "_conf"],
                weight=g[tag + "_weight"], pairs=g[tag + "_pairs"], err=g[tag + "_err"], weights_out=g[tag + "_weights_out"],
                threshold=float(g[tag + "_threshold"]))


def confidence(conf, V, B, J):
    """conf: None, or a list of V arrays (B,J) or (B,J,3) (channel 2) -> (V,B,J) float64 (ones without confidences)"""
    if conf is None:
        return np.ones((V, B, J))
    return np.stack([np.asarray(c, dtype=np.float64)[..., 2] if np.ndim(c) == 3 else np.asarray(c, dtype=np.float64) for c in conf])


def lines(rays, centers):
    """-> c (V,B,1,3), d (V,B,J,3): centres and unit directions in float64"""
    r = np.stack([np.asarray(x, dtype=np.float64) for x in rays])
    c = np.stack([np.asarray(x, dtype=np.float64) for x in centers])
    u = r - c
    with np.errstate(invalid="ignore", divide="ignore"):
        return c, u / np.linalg.norm(u, axis=-1, keepdims=True)


def point_line_distance(x, c, d):
    """distance of x to the line through c along the unit vector d: the perpendicular part of x - c, formed as a vector (the form
    |p|^2 - (p.d)^2 cancels where the point lies on the line)"""
    p = x - c
    return np.linalg.norm(p - np.sum(p * d, axis=-1, keepdims=True) * d, axis=-1)


def triangulate(rays, centers, conf=None):
    """-> points (B,J,3), residual (B,J) float64; NaN where fewer than two views take part or det(A / sum w) < DET_MIN"""
    c, d = lines(rays, centers)
    V, B, J, _ = d.shape
    w = confidence(conf, V, B, J)
    with np.errstate(invalid="ignore"):
        w = np.where(np.isfinite(w) & (w > 0), w, 0.0)          # a view with w <= 0 or a non-finite w does not take part
    cm = c.mean(axis=0)                                          # (B,1,3) origin shift
    M = np.eye(3) - d[..., :, None] * d[..., None, :]            # (V,B,J,3,3)
    A = np.sum(w[..., None, None] * M, axis=0)
    b = np.sum(w[..., None] * np.einsum("vbjxy,vbjy->vbjx", M, np.broadcast_to(c - cm, d.shape)), axis=0)
    W = w.sum(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        bad = ((w > 0).sum(axis=0) < 2) | ~(np.linalg.det(A / W[..., None, None]) >= DET_MIN)
    A[bad] = np.eye(3)
    x = cm + np.linalg.solve(A, b[..., None])[..., 0]
    dist = np.stack([point_line_distance(x, c[v], d[v]) for v in range(V)])
    with np.errstate(invalid="ignore", divide="ignore"):
        res = np.sqrt(np.sum(w * dist * dist, axis=0) / W)
    x[bad] = np.nan
    res[bad] = np.nan
    return x, res


def pair_distance(ci, di, ck, dk):
    """calib.py:94-113 on centres and unit directions: |(c_k - c_i) . (d_i x d_k)| / |d_i x d_k|; where |d_i x d_k|^2 < PARALLEL
    (the reference divides 0 by 0) the distance of c_k to line i"""
    n = np.cross(di, dk)
    nn = np.sum(n * n, axis=-1)
    dc = np.broadcast_to(ck - ci, di.shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        skew = np.abs(np.sum(dc * n, axis=-1)) / np.sqrt(nn)
    return np.where(nn < PARALLEL, np.linalg.norm(np.cross(dc, di), axis=-1), skew)


def epipolar(rays, centers, conf=None):
    """calib.py:131-165 -> (B,V,J) float64: every pair counts, the confidence scales only the view's own total"""
    c, d = lines(rays, centers)
    V, B, J, _ = d.shape
    cf = confidence(conf, V, B, J)
    err = np.zeros((V, B, J))
    for i in range(V):
        for k in range(V):
            if k != i:
                err[i] += pair_distance(c[i], d[i], c[k], d[k])
    return np.transpose(cf * err / (V - 1), (1, 0, 2))


def thresholded(err, weight, threshold):
    """calib.py:167-168; err (B,V,J), weight a list of V (B,J) -> list of V (B,J)"""
    return [np.where(err[:, v] > threshold, 0.0, np.asarray(weight[v])).astype(np.float32) for v in range(len(weight))]


def rel_errors(got, ref):
    """the parity rule of DESIGN.md section 2: (max|d| / max|ref|, ||d||_2 / ||ref||_2) over the finite entries of ref;
    NaN must sit in the same places"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN in other places than the restatement"
    ok = ~np.isnan(ref)
    d = got[ok] - ref[ok]
    if d.size == 0 or np.abs(ref[ok]).max() == 0:
        return float(np.abs(d).max(initial=0.0)), 0.0
    return float(np.abs(d).max() / np.abs(ref[ok]).max()), float(np.linalg.norm(d) / np.linalg.norm(ref[ok]))


def ring_centres(V, seed=0):
    """V camera centres looking inward from three rings of about 6 m radius at elevations 15, 38 and 60 degrees (view v sits on
    ring v % 3): all above the horizon, so no two cameras face each other through the origin, and no two lines of sight of one
    point within 0.3 m of the origin come closer than 12 degrees to parallel, up to 32 views (the rig jitter of ring_case included)."""
    rs = np.random.RandomState(1000 + seed)
    v = np.arange(V)
    k, m = v % 3, v // 3
    n = np.array([len(range(r, V, 3)) for r in range(3)])[k]
    az = np.deg2rad(70.0) * v if V <= 3 else 2 * np.pi * (m + 0.37 * k) / n
    el = np.deg2rad(np.array([15.0, 38.0, 60.0]))[k]
    rad = 6.0 + 0.2 * rs.rand(V)
    return np.stack([rad * np.cos(el) * np.cos(az), rad * np.cos(el) * np.sin(az), rad * np.sin(el)], axis=1)


def min_pair_angle(rays, centers):
    """smallest angle (degrees) between two lines of one joint"""
    _, d = lines(rays, centers)
    cosmax = 0.0
    for i in range(d.shape[0]):
        for k in range(i):
            cosmax = max(cosmax, float(np.abs(np.sum(d[i] * d[k], axis=-1)).max()))
    return float(np.degrees(np.arccos(min(1.0, cosmax))))


def ring_case(B, V, J, seed=0, noise=0.02, exact=False):
    """Points within 0.3 m (per axis) of the origin seen from ring_centres: rays[v] = a point at 1 .. 2 m along the line of sight of
    (point + noise), float32.  -> dict(rays, centers, points (B,J,3) float64, conf (V,B,J) float32 in [0.05, 1])"""
    rs = np.random.RandomState(seed * 7919 + B * 131 + V * 17 + J)
    cen = ring_centres(V, seed)
    pts = rs.uniform(-0.3, 0.3, size=(B, J, 3))
    rays, centers = [], []
    for v in range(V):
        c32 = (cen[v] + rs.uniform(-0.2, 0.2, size=(B, 1, 3))).astype(np.float32)       # a rig that moves from sample to sample
        aim = pts + (0.0 if exact else noise) * rs.randn(B, J, 3)
        u = aim - c32.astype(np.float64)
        u = u / np.linalg.norm(u, axis=-1, keepdims=True) * rs.uniform(1.0, 2.0, size=(B, J, 1))
        rays.append((c32.astype(np.float64) + u).astype(np.float32))
        centers.append(c32)
    conf = rs.uniform(0.05, 1.0, size=(V, B, J)).astype(np.float32)
    assert min_pair_angle(rays, centers) > 10.0
    return dict(rays=rays, centers=centers, points=pts, conf=conf)
