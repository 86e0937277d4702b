"""Float64 restatement of the lens model of csrc/views.hpp and of every call that takes distortion=, and the scenes of their tests
(TEST INFRASTRUCTURE ONLY).

numpy float64 on the float32 inputs the kernels read, nothing rounded: the tests round once to float32 where they compare.  The
projection is pinned by tests/golden/distortion.npz, which the reference's own project_pose (lib/multiviews/cameras.py:22-51)
produced (tests/golden/make_golden_distortion.py).  The inverse is Newton's iteration under the rule of include/mpl_hip.h: from
y = y_d, at most MAX_ITER iterations, an iterate with det J <= 0 or a non-finite value is not invertible, done when
max |step| <= TOL * max(1, |y|_inf).
"""
import functools
import os

import numpy as np

from tests import synth_cases as sc

GOLD = sc.GOLD
MAX_ITER, TOL = 20, 1e-14
H36M = (-0.2075, 0.2476, -0.0031, -0.00098, -0.00142)         # k1 k2 k3 p1 p2: the magnitudes of Human3.6M's calibration
CMU = (-0.30, 0.0, 0.0, 0.0, 0.0)
STRONG = (-0.4, 0.2, -0.05, 0.0, 0.0)
POSITIVE = (0.12, 0.03, 0.0, 0.0008, -0.0011)
ZEROS = (0.0,) * 5
SETS = ("zeros", "h36m", "cmu", "strong", "per_view")
FOCAL = 1145.0
DET_MIN = 0.05             # every item meant to be valid has det J >= this throughout its iteration
REACH_FACTOR = 1.1         # every item meant to be invalid has |y_d| >= this times the largest |y_d| the lens can produce


def table(name, V):
    """the (V,5) float64 distortion table of a named set"""
    rows = {"zeros": [ZEROS], "h36m": [H36M], "cmu": [CMU], "strong": [STRONG], "per_view": [H36M, CMU, STRONG, ZEROS, POSITIVE]}[name]
    return np.array([rows[v % len(rows)] for v in range(V)], dtype=np.float64)


# ------------------------------------------------------------------------------------------------------- the model and its inverse
def distort(y0, y1, d):
    """normalised pinhole coordinates -> the same after the lens; d (..., 5) broadcasts against y"""
    k1, k2, k3, p1, p2 = (d[..., i] for i in range(5))
    r2 = y0 * y0 + y1 * y1
    g = 1.0 + (k1 * r2 + k2 * (r2 * r2) + k3 * (r2 * r2 * r2)) + (2.0 * p1 * y1 + 2.0 * p2 * y0)
    return y0 * g + p2 * r2, y1 * g + p1 * r2


def jacobian(y0, y1, d):
    """-> (j00, j01, j10, j11, det) of distort at y"""
    k1, k2, k3, p1, p2 = (d[..., i] for i in range(5))
    r2 = y0 * y0 + y1 * y1
    g = 1.0 + (k1 * r2 + k2 * (r2 * r2) + k3 * (r2 * r2 * r2)) + (2.0 * p1 * y1 + 2.0 * p2 * y0)
    gr = k1 + 2.0 * k2 * r2 + 3.0 * k3 * (r2 * r2)
    g0, g1 = 2.0 * (gr * y0 + p2), 2.0 * (gr * y1 + p1)
    j00, j01 = g + y0 * g0 + 2.0 * p2 * y0, y0 * g1 + 2.0 * p2 * y1
    j10, j11 = y1 * g0 + 2.0 * p1 * y0, g + y1 * g1 + 2.0 * p1 * y1
    return j00, j01, j10, j11, j00 * j11 - j01 * j10


def undistort(yd0, yd1, d):
    """The Newton inverse, item by item in lockstep -> (y0, y1, valid, iterations, min_det): iterations is the number of steps an
    item took (MAX_ITER + 1 where the cap ran out), min_det the smallest det J among its iterates."""
    yd0, yd1 = np.asarray(yd0, dtype=np.float64), np.asarray(yd1, dtype=np.float64)
    d = np.broadcast_to(np.asarray(d, dtype=np.float64), yd0.shape + (5,))
    y0, y1 = yd0.copy(), yd1.copy()
    live = np.ones(yd0.shape, bool)
    valid = np.zeros(yd0.shape, bool)
    iters = np.zeros(yd0.shape, int)
    min_det = np.full(yd0.shape, np.inf)
    with np.errstate(all="ignore"):
        for it in range(MAX_ITER):
            if not live.any():
                break
            f0, f1 = distort(y0, y1, d)
            f0, f1 = f0 - yd0, f1 - yd1
            j00, j01, j10, j11, det = jacobian(y0, y1, d)
            min_det = np.where(live, np.fmin(min_det, np.where(np.isnan(det), -np.inf, det)), min_det)
            ok = live & (det > 0.0)
            s0, s1 = (j11 * f0 - j01 * f1) / det, (j00 * f1 - j10 * f0) / det
            y0, y1 = np.where(ok, y0 - s0, y0), np.where(ok, y1 - s1, y1)
            iters = np.where(ok, it + 1, iters)
            ok &= np.isfinite(y0) & np.isfinite(y1)
            done = ok & (np.fmax(np.abs(s0), np.abs(s1)) <= TOL * np.fmax(1.0, np.fmax(np.abs(y0), np.abs(y1))))
            valid |= done
            live = ok & ~done
        iters = np.where(live, MAX_ITER + 1, iters)
    return y0, y1, valid, iters, min_det


def reach(d5):
    """_reach of one coefficient set, computed once per set"""
    return _reach(tuple(float(x) for x in d5))


@functools.lru_cache(maxsize=None)
def _reach(d5):
    """the largest |y_d| the lens of one coefficient set produces on the part of the plane connected to the axis where det J > 0
    (inf where some direction has no fold within radius 3): a polar scan, fine enough for the factor it is used with"""
    d5 = np.asarray(d5, dtype=np.float64)
    if not d5.any():
        return np.inf
    th = np.linspace(0.0, 2 * np.pi, 720, endpoint=False)[:, None]
    r = np.arange(1, 3001)[None, :] * 1e-3
    y0, y1 = r * np.cos(th), r * np.sin(th)
    det = jacobian(y0, y1, d5)[4]
    inside = np.cumprod(det > 0.0, axis=1).astype(bool)
    if inside[:, -1].any():
        return np.inf
    f0, f1 = distort(y0, y1, d5)
    return float(np.where(inside, np.hypot(f0, f1), 0.0).max())


# ----------------------------------------------------------------------------------------------------------- the calls, restated
def _intrinsics(cams):
    cams = np.asarray(cams, dtype=np.float64)
    return tuple(cams[:, k][None, :, None] for k in range(4))


def project(points3d, cams, dist):
    """project_points(distortion=): -> pixels (B,V,J,2), depth (B,V,J), float64; a point at depth <= Z_MIN gets pixel (0,0)"""
    X = np.asarray(points3d, dtype=np.float64)
    cams = np.asarray(cams, dtype=np.float64)
    V = cams.shape[0]
    fx, fy, cx, cy = _intrinsics(cams)
    R, t = cams[:, 4:13].reshape(V, 3, 3), cams[:, 13:16]
    xc = np.einsum("vxy,bvjy->bvjx", R, X[:, None, :, :] - t[None, :, None, :])
    zc = xc[..., 2]
    front = zc > sc.Z_MIN
    with np.errstate(divide="ignore", invalid="ignore"):
        yd0, yd1 = distort(xc[..., 0] / zc, xc[..., 1] / zc, np.asarray(dist, dtype=np.float64)[None, :, None, :])
        px = np.stack([np.where(front, fx * yd0 + cx, 0.0), np.where(front, fy * yd1 + cy, 0.0)], axis=-1)
    return px, zc


def undistort_pixels(pixels, cams, dist):
    """undistort_points: -> dict(pixels (B,V,J,2) with NaN at the invalid items, valid, iterations, min_det, yd_norm (B,V,J))"""
    px = np.asarray(pixels, dtype=np.float64)
    fx, fy, cx, cy = _intrinsics(cams)
    x, y = px[..., 0], px[..., 1]
    yd0, yd1 = (x - cx) / fx, (y - cy) / fy
    y0, y1, valid, iters, min_det = undistort(yd0, yd1, np.asarray(dist, dtype=np.float64)[None, :, None, :])
    out = np.stack([np.where(valid, x + fx * (y0 - yd0), np.nan), np.where(valid, y + fy * (y1 - yd1), np.nan)], axis=-1)
    return dict(pixels=out, valid=valid, iterations=iters, min_det=min_det, yd_norm=np.hypot(yd0, yd1))


def distort_pixels(pixels, cams, dist):
    """distort_points: the forward polynomial on a pinhole pixel, in the form input + correction"""
    px = np.asarray(pixels, dtype=np.float64)
    fx, fy, cx, cy = _intrinsics(cams)
    x, y = px[..., 0], px[..., 1]
    y0, y1 = (x - cx) / fx, (y - cy) / fy
    yd0, yd1 = distort(y0, y1, np.asarray(dist, dtype=np.float64)[None, :, None, :])
    return np.stack([x + fx * (yd0 - y0), y + fy * (yd1 - y1)], axis=-1)


def _views(x, y, cf, xr, yr, cams, wh, normalize_inputs, normalize_cameras):
    """step 6 / prepare_inputs: poses from (x, y, cf), rays through (xr, yr); all (B,V,J) float64 -> poses, rays (V,B,J,3),
    centers (V,B,1,3)"""
    cams = np.asarray(cams, dtype=np.float64)
    V, B = cams.shape[0], x.shape[0]
    w, h = float(wh[0]), float(wh[1])
    fx, fy, cx, cy = _intrinsics(cams)
    R, t = cams[:, 4:13].reshape(V, 3, 3), cams[:, 13:16]
    if normalize_inputs:
        x, y = (x / w) * 2.0 - 1.0, (y / w) * 2.0 - h / w
        xr, yr = (xr / w) * 2.0 - 1.0, (yr / w) * 2.0 - h / w
        if normalize_cameras:
            cx, cy = (cx / w) * 2.0 - 1.0, (cy / w) * 2.0 - h / w
            fx, fy = fx / w * 2.0, fy / w * 2.0
    u = np.stack([(xr - cx) / fx, (yr - cy) / fy, np.ones_like(xr)], axis=-1)
    rays = np.einsum("vyx,bvjy->vbjx", R, u) + t[:, None, None, :]
    poses = np.transpose(np.stack([x, y, cf], axis=-1), (1, 0, 2, 3))
    centers = np.broadcast_to(t[:, None, None, :], (V, B, 1, 3)).copy()
    return poses, rays, centers


def prepare(pixels, conf, cams, dist, wh=(1.0, 1.0), normalize_inputs=True, normalize_cameras=True):
    """prepare_inputs(distortion=): poses hold the observed pixel, the ray goes through the undistorted one; an item that is not
    invertible keeps its pinhole ray and gets confidence 0 -> dict(poses, rays, centers, valid)"""
    px = np.asarray(pixels, dtype=np.float64)
    B, V, J, _ = px.shape
    cf = np.ones((B, V, J)) if conf is None else np.asarray(conf, dtype=np.float64).reshape(B, V, J)
    u = undistort_pixels(px, cams, dist)
    xr, yr = np.where(u["valid"], u["pixels"][..., 0], px[..., 0]), np.where(u["valid"], u["pixels"][..., 1], px[..., 1])
    poses, rays, centers = _views(px[..., 0], px[..., 1], np.where(u["valid"], cf, 0.0), xr, yr, cams, wh, normalize_inputs, normalize_cameras)
    return dict(poses=poses, rays=rays, centers=centers, valid=u["valid"], min_det=u["min_det"], iterations=u["iterations"])


def synthesize(poses3d, cams, dist, image_size, seed=0, first_index=0, rotate=False, room=None, noise_level=0.0, penalize="none",
               penalize_a=1.0, penalize_b=0.0, clip=True, missing_level=0.0, conf=None, normalize_inputs=True, normalize_cameras=True,
               target_scale=None, target_offset=None):
    """synthesize_views(distortion=) with the kernel's own streams: synth_cases.synthesize with the steps that change -- 2 (the
    projection goes through the lens) and 6 (the ray goes through the undistorted pixel).  Steps 1, 3, 4, 5 and 7 are the lines of
    synth_cases.synthesize.  -> its dict, plus valid, min_det, iterations (B,V,J) of step 6's inverse"""
    X = np.asarray(poses3d, dtype=np.float64).copy()
    cams = np.asarray(cams, dtype=np.float64)
    B, J, _ = X.shape
    V = cams.shape[0]
    w, h = float(image_size[0]), float(image_size[1])
    gpose = first_index + np.arange(B)
    if rotate:                                                                                   # 1
        a = sc.draw(seed, "synth.rot", 0, gpose) * 360.0 * (np.pi / 180.0)
        ca, sa = np.cos(a)[:, None], np.sin(a)[:, None]
        X[..., 0], X[..., 1] = X[..., 0] * ca - X[..., 1] * sa, X[..., 0] * sa + X[..., 1] * ca
    if room is not None:
        X[..., 0] += (sc.draw(seed, "synth.room", 0, gpose) * (room[1] - room[0]) + room[0])[:, None]
        X[..., 1] += (sc.draw(seed, "synth.room", 1, gpose) * (room[3] - room[2]) + room[2])[:, None]
    clean, zc = project(X, cams, dist)                                                           # 2
    front = zc > sc.Z_MIN
    x, y = clean[..., 0], clean[..., 1]
    cf = np.where(front, np.ones((B, V, J)) if conf is None else np.asarray(conf, dtype=np.float64).reshape(B, V, J), 0.0)
    margin = np.abs(zc - sc.Z_MIN)
    gitem = (gpose[:, None, None] * V + np.arange(V)[None, :, None]) * J + np.arange(J)[None, None, :]
    if noise_level != 0.0:                                                                       # 3
        n = sc.normal_pair(seed, gitem) * noise_level
        xn, yn = x + n[..., 0], y + n[..., 1]
        cfn = cf * sc.penalty(penalize, np.sqrt(n[..., 0] ** 2 + n[..., 1] ** 2), penalize_a, penalize_b)
    else:
        xn, yn, cfn = x, y, cf
    for c, edges in ((xn, (0.0, w - 1.0, w)), (yn, (0.0, h - 1.0, h))):
        for e in edges:
            margin = np.minimum(margin, np.where(front, np.abs(c - e), np.inf))
    if clip:                                                                                     # 4
        inside = (0 < xn) & (xn < w - 1) & (0 < yn) & (yn < h - 1)
        cfv = np.where(inside, cfn, 0.0)
        xv, yv = np.clip(xn, 0, w - 1), np.clip(yn, 0, h - 1)
    else:
        margin = np.minimum(margin, np.where(front & (cfn != 0), np.abs(cfn), np.inf))
        out = (np.minimum(xn, yn) < 0) | (xn >= w) | (yn >= h)
        cfv = np.where((cfn > 0) & out, 0.0, cfn)
        xv, yv = np.where(cfv > 0, xn, 0.0), np.where(cfv > 0, yn, 0.0)
    if missing_level > 0.0:                                                                      # 5
        u = sc.draw(seed, "synth.missing", 0, gitem)
        margin = np.minimum(margin, np.where(front, np.abs(u - missing_level) * 1e3, np.inf))
        keep = np.where(u < missing_level, 0.0, 1.0)
        cfv, xv, yv = cfv * keep, xv * keep, yv * keep
    x, y, cf = np.where(front, xv, 0.0), np.where(front, yv, 0.0), np.where(front, cfv, 0.0)
    pixels = np.stack([x, y], axis=-1)
    r = prepare(pixels, cf, cams, dist, (w, h), normalize_inputs, normalize_cameras)            # 6
    s = np.ones(3) if target_scale is None else np.asarray(target_scale, dtype=np.float64)      # 7
    of = np.zeros(3) if target_offset is None else np.asarray(target_offset, dtype=np.float64)
    return dict(poses=r["poses"], rays=r["rays"], centers=r["centers"], target=(X - of) / s, placed=X, pixels=pixels, pixels_clean=clean,
                depth=zc, conf=np.transpose(r["poses"][..., 2], (1, 0, 2)), margin=margin, valid=r["valid"], min_det=r["min_det"],
                iterations=r["iterations"])


# ------------------------------------------------------------------------------------------------------------------------- scenes
def case(B, V, J, name, seed=3, invalid_every=0):
    """A scene of synth_cases.scene at the focal length of H36M under the coefficient set `name`, seen through the lens:
    dict(points (B,J,3) float32, cams (V,16), dist (V,5), pixels (B,V,J,2) float32 -- the distorted projections --, valid (B,V,J)).
    invalid_every = n > 0 replaces every n-th item of a view whose lens folds by a pixel no pinhole point maps to.  A case is
    rejected (AssertionError) unless every item meant to be valid keeps det J >= DET_MIN throughout its inverse and every item
    meant to be invalid lies at |y_d| >= REACH_FACTOR x the largest reachable value; nothing is ever skipped."""
    points, cams = sc.scene(B, V, J, seed=seed, focal=FOCAL)
    dist = table(name, V)
    px, depth = project(points, cams, dist)
    assert depth.min() > 0.5
    px = px.astype(np.float32)
    want = np.ones((B, V, J), bool)
    reaches = np.array([reach(dist[v]) for v in range(V)])
    if invalid_every:
        idx = np.arange(B * V * J).reshape(B, V, J)
        pick = (idx % invalid_every == invalid_every - 1) & np.isfinite(reaches)[None, :, None]
        assert pick.any(), "no view of this set has a fold: nothing can be made invalid"
        ang = 2.39996 * idx                                           # the golden angle: directions all round the axis
        rad = np.where(np.isfinite(reaches), reaches, 0.0)[None, :, None] * (REACH_FACTOR + 0.05 + 0.4 * ((idx % 7) / 7.0))
        fx, fy, cx, cy = _intrinsics(cams)
        bad = np.stack([fx * rad * np.cos(ang) + cx, fy * rad * np.sin(ang) + cy], axis=-1).astype(np.float32)
        px = np.where(pick[..., None], bad, px)
        want = ~pick
    u = undistort_pixels(px, cams, dist)
    # nothing is skipped: every item is either valid with a comfortable Jacobian or invalid by a comfortable margin
    assert (u["min_det"][want] >= DET_MIN).all(), "a valid item comes within %.3g of a fold" % u["min_det"][want].min()
    assert (u["yd_norm"][~want] >= REACH_FACTOR * np.broadcast_to(reaches[None, :, None], want.shape)[~want]).all()
    assert np.array_equal(u["valid"], want), "the restatement disagrees with the construction"
    return dict(points=points, cams=cams, dist=dist, pixels=px, valid=want, skipped=0, restated=u)


def golden():
    g = np.load(os.path.join(GOLD, "distortion.npz"))
    return {k: g[k] for k in g.files}
