"""Float64 restatement of openmpl_amd.geometry.refine_points / reprojection_errors (csrc/refine.hip) and the cases of their tests
(TEST INFRASTRUCTURE ONLY).

numpy float64 on the float32 inputs the kernel reads, nothing rounded: the tests round once to float32 where they compare.  The
reference has no refinement, so there is no golden of its own: the projection is tests/distortion_cases.project, which
tests/golden/distortion.npz pins to the reference's project_pose, and the lens Jacobian is distortion_cases.jacobian, which its
Newton inverse is tested with.  The Levenberg-Marquardt loop is that of include/mpl_hip.h, all items in lockstep: an item that has
stopped keeps its state while the others go on.
"""
import numpy as np

from tests import distortion_cases as dc
from tests import geometry_cases as gc
from tests import synth_cases as sc

LAMBDA0, LAMBDA_MIN, LAMBDA_MAX = 1e-3, 1e-15, 1e12
WH = (1000.0, 1000.0)


# --------------------------------------------------------------------------------------------- projection, Jacobian, cost
def residuals(X, pixels, cams, dist):
    """r = proj_v(X) - px_v -> (r (B,V,J,2), depth (B,V,J)); X (B,J,3).  The projection is dc.project, called, not re-derived"""
    with np.errstate(all="ignore"):
        px, zc = dc.project(X, cams, dist)
        return px - np.asarray(pixels, dtype=np.float64), zc


def jacobian(X, cams, dist):
    """d proj_v / d X -> (B,V,J,2,3): diag(f) (the lens Jacobian) (d y / d x_cam) R"""
    X = np.asarray(X, dtype=np.float64)
    cams = np.asarray(cams, dtype=np.float64)
    V = cams.shape[0]
    R, t = cams[:, 4:13].reshape(V, 3, 3), cams[:, 13:16]
    with np.errstate(all="ignore"):
        xc = np.einsum("vxy,bvjy->bvjx", R, X[:, None, :, :] - t[None, :, None, :])
        z = xc[..., 2]
        y0, y1 = xc[..., 0] / z, xc[..., 1] / z
        j00, j01, j10, j11, _ = dc.jacobian(y0, y1, np.asarray(dist, dtype=np.float64)[None, :, None, :])
        fx, fy = cams[:, 0][None, :, None], cams[:, 1][None, :, None]
        m0 = np.stack([fx * j00 / z, fx * j01 / z, -(fx * j00 * y0 + fx * j01 * y1) / z], axis=-1)       # (B,V,J,3): d px / d x_cam
        m1 = np.stack([fy * j10 / z, fy * j11 / z, -(fy * j10 * y0 + fy * j11 * y1) / z], axis=-1)
        return np.stack([np.einsum("bvjk,vkc->bvjc", m0, R), np.einsum("bvjk,vkc->bvjc", m1, R)], axis=-2)


def participation(pixels, conf):
    """-> (part (B,V,J) bool, w (B,V,J) float64, 0 where the view takes no part)"""
    px = np.asarray(pixels, dtype=np.float64)
    w = np.ones(px.shape[:3]) if conf is None else np.asarray(conf, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        part = np.isfinite(w) & (w > 0) & np.isfinite(px).all(axis=-1)
    return part, np.where(part, w, 0.0)


def evaluate(X, pixels, conf, cams, dist, huber=None):
    """One evaluation at X (B,J,3) -> dict(E, S (B,J): the cost in the mode of the call, +inf behind a camera that takes part, and
    the plain sum w |r|^2; H (B,J,3,3), g (B,J,3): the normal equations with the IRLS weights; zmin (B,J); behind (B,J);
    r (B,V,J,2), s (B,V,J) = |r|^2, part, w)"""
    part, w = participation(pixels, conf)
    r, zc = residuals(X, pixels, cams, dist)
    Jm = jacobian(X, cams, dist)
    with np.errstate(all="ignore"):
        behind = (part & ~(zc > sc.Z_MIN)).any(axis=1)
        r = np.where(part[..., None], r, 0.0)
        Jm = np.where(part[..., None, None], Jm, 0.0)
        s = np.sum(r * r, axis=-1)
        rho, wi = s, w
        if huber is not None:
            h = float(huber)
            rn = np.sqrt(s)
            tail = s > h * h
            rho = np.where(tail, 2.0 * h * rn - h * h, s)
            wi = np.where(tail, w * (h / np.where(tail, rn, 1.0)), w)
        E = np.sum(w * rho, axis=1)
        H = np.einsum("bvj,bvjac,bvjad->bjcd", wi, Jm, Jm)
        g = np.einsum("bvj,bvjac,bvja->bjc", wi, Jm, r)
        zmin = np.where(part, zc, np.inf).min(axis=1)
    return dict(E=np.where(behind, np.inf, E), S=np.sum(w * s, axis=1), H=H, g=g, zmin=zmin, behind=behind, r=r, s=s, part=part, w=w)


def cost(X, pixels, conf, cams, dist, huber=None):
    return evaluate(X, pixels, conf, cams, dist, huber)["E"]


def solve3(A, b):
    """A x = b for symmetric 3x3 A (..., 3, 3) by the adjugate, the closed form of the kernel; a singular A gives inf / NaN"""
    a, bb, c, d, f, h = A[..., 0, 0], A[..., 0, 1], A[..., 0, 2], A[..., 1, 1], A[..., 1, 2], A[..., 2, 2]
    with np.errstate(all="ignore"):
        c00, c01, c02 = d * h - f * f, c * f - bb * h, bb * f - c * d
        c11, c12, c22 = a * h - c * c, bb * c - a * f, a * d - bb * bb
        inv = 1.0 / (a * c00 + bb * c01 + c * c02)
        return np.stack([(c00 * b[..., 0] + c01 * b[..., 1] + c02 * b[..., 2]) * inv,
                         (c01 * b[..., 0] + c11 * b[..., 1] + c12 * b[..., 2]) * inv,
                         (c02 * b[..., 0] + c12 * b[..., 1] + c22 * b[..., 2]) * inv], axis=-1)


def lm_step(H, g, lam):
    """(H + lambda diag H) delta = -g"""
    A = H.copy()
    for k in range(3):
        A[..., k, k] = H[..., k, k] + lam * H[..., k, k]
    return solve3(A, -g)


def _take(mask, new, old):
    return np.where(mask.reshape(mask.shape + (1,) * (new.ndim - mask.ndim)), new, old)


# ------------------------------------------------------------------------------------------------------------------ the call
def refine(points, pixels, conf, cams, dist=None, huber=None, max_iterations=20, step_tolerance=1e-8):
    """refine_points -> dict(points (B,J,3), error (B,J), errors (B,V,J), iterations, status (B,J) ints, E0, E (B,J): the cost at the
    given and at the final point (NaN for an invalid item), accepted (B,J): accepted trials)"""
    X0 = np.asarray(points, dtype=np.float64)
    cams = np.asarray(cams, dtype=np.float64)
    dist = np.zeros((cams.shape[0], 5)) if dist is None else np.asarray(dist, dtype=np.float64)
    args = (pixels, conf, cams, dist, huber)
    cur = evaluate(X0, *args)
    n = cur["part"].sum(axis=1)
    invalid = ~np.isfinite(X0).all(axis=-1) | (n == 0) | cur["behind"]
    passed = ~invalid & ((n < 2) | (max_iterations == 0))
    live = ~invalid & ~passed
    status = np.where(invalid, 3, np.where(passed, 2, 1))
    X, E0 = X0.copy(), cur["E"].copy()
    lam = np.full(n.shape, LAMBDA0)
    iters, accepted = np.zeros(n.shape, int), np.zeros(n.shape, int)
    with np.errstate(all="ignore"):
        for _ in range(max_iterations):
            if not live.any():
                break
            delta = lm_step(cur["H"], cur["g"], lam)
            Xt = np.where(live[..., None], X + delta, X)
            tr = evaluate(Xt, *args)
            acc = live & (tr["E"] < cur["E"])                    # strictly lower: +inf and NaN are never accepted
            X = _take(acc, Xt, X)
            for k in ("E", "H", "g", "zmin"):
                cur[k] = _take(acc, tr[k], cur[k])
            lam = np.where(acc, np.maximum(lam / 10.0, LAMBDA_MIN), np.where(live, lam * 10.0, lam))
            iters += live
            accepted += acc
            conv = live & (np.abs(delta).max(axis=-1) <= step_tolerance * cur["zmin"])
            status = np.where(conv, 0, status)
            live = live & ~conv & ~(lam > LAMBDA_MAX)
        fin = evaluate(X, *args)
        errors = np.where(fin["part"] & ~invalid[:, None, :], np.sqrt(fin["s"]), np.nan)
        error = np.where(invalid, np.nan, np.sqrt(fin["S"] / fin["w"].sum(axis=1)))
    return dict(points=np.where(invalid[..., None], np.nan, X), error=error, errors=errors, iterations=iters, status=status,
                E0=np.where(invalid, np.nan, E0), E=np.where(invalid, np.nan, fin["E"]), accepted=accepted, zmin=fin["zmin"])


def newton_step(X, pixels, conf, cams, dist, huber=None):
    """the undamped step H delta = -g at X, and the smallest depth there -> (delta (B,J,3), zmin (B,J))"""
    e = evaluate(X, pixels, conf, cams, dist, huber)
    return solve3(e["H"], -e["g"]), e["zmin"]


def rounding_slack(X, pixels, conf, cams, dist, huber=None):
    """How much one fp32 rounding of the point X can add to E, (B,J): with |e_c| <= ulp32(X_c) / 2 and E = sum w' |r|^2 around X,
    E(X + e) - E(X) ~ 2 g.e + e^T H e <= 2 sum |g_c| |e_c| + (sum sqrt(H_cc) |e_c|)^2; doubled for what Gauss-Newton leaves out."""
    e = evaluate(X, pixels, conf, cams, dist, huber)
    half = 0.5 * np.spacing(np.abs(np.asarray(X, dtype=np.float64)).astype(np.float32)).astype(np.float64)
    Hd = np.stack([e["H"][..., k, k] for k in range(3)], axis=-1)
    return 2.0 * (2.0 * np.sum(np.abs(e["g"]) * half, axis=-1) + np.sum(np.sqrt(Hd) * half, axis=-1) ** 2)


# -------------------------------------------------------------------------------------------------------------------- cases
def linear_points(pixels, conf, cams, dist):
    """the float64 chain of triangulate_pixels with both stages off, on the fp32 pixels: prepare (rays through the undistorted
    pixels, rounded to fp32 as the device hands them on) -> the least-squares point of the lines; NaN where it is degenerate"""
    r = dc.prepare(pixels, conf, cams, dist, WH, False, False)
    V = len(r["rays"])
    cf = [r["poses"][v][..., 2].astype(np.float32) for v in range(V)]
    x, _ = gc.triangulate([r["rays"][v].astype(np.float32) for v in range(V)], [r["centers"][v].astype(np.float32) for v in range(V)], cf)
    return x


def case(B, V, J, name="h36m", seed=13, noise=2.0, conf="none", outliers=0, start="linear"):
    """A scene of synth_cases.scene at the focal length of H36M under the lens set `name`: the distorted projections of its points
    plus `noise` px of Gaussian noise (numpy RandomState), rounded to float32.
    conf: "none"; "uniform" (0.3 .. 1); "mixed": uniform with zeros, NaN and negatives inside, at most V - 2 of them per joint
    where V >= 3 so that two views still take part.  outliers = n: n views of every joint (chosen per joint) moved 40 .. 120 px off
    in a random direction.  start: "linear" -- the float64 least-squares point of linear_points, rounded to float32; where it is
    not finite (a single view), and with start="truth", the true point plus 0.02 units of noise; "exact" -- the true point itself.
    -> dict(points0 (B,J,3) float32, pixels (B,V,J,2) float32, conf (B,V,J) float32 or None, cams, dist, truth (B,J,3) float32)"""
    truth, cams = sc.scene(B, V, J, seed=seed, focal=dc.FOCAL)
    dist = dc.table(name, V)
    rs = np.random.RandomState(seed * 1009 + B * 131 + V * 17 + J)
    px, depth = dc.project(truth, cams, dist)
    assert depth.min() > 0.5
    px = px + noise * rs.randn(B, V, J, 2)
    if outliers:
        order = np.argsort(rs.rand(B, V, J), axis=1)
        out = order < outliers                                   # `outliers` views of every (b, j)
        ang, far = rs.uniform(0, 2 * np.pi, (B, V, J)), rs.uniform(40.0, 120.0, (B, V, J))
        px = px + np.where(out[..., None], np.stack([far * np.cos(ang), far * np.sin(ang)], axis=-1), 0.0)
    px = px.astype(np.float32)
    cf = None
    if conf != "none":
        cf = rs.uniform(0.3, 1.0, (B, V, J)).astype(np.float32)
        if conf == "mixed":
            kind = rs.randint(0, 6, (B, V, J))                   # 0: zero, 1: NaN, 2: negative, else kept
            rank = np.argsort(np.argsort(rs.rand(B, V, J), axis=1), axis=1)
            hit = (kind < 3) & (rank < max(V - 2, 0))
            cf = np.where(hit & (kind == 0), 0.0, np.where(hit & (kind == 1), np.nan, np.where(hit & (kind == 2), -cf, cf))).astype(np.float32)
        else:
            assert conf == "uniform", conf
    fallback = (truth.astype(np.float64) + 0.02 * rs.randn(B, J, 3)).astype(np.float32)
    x0 = truth if start == "exact" else fallback
    if start == "linear" and V >= 2:
        with np.errstate(all="ignore"):
            lin = linear_points(px, cf, cams, dist)
        x0 = np.where(np.isfinite(lin).all(axis=-1, keepdims=True), lin, fallback).astype(np.float32)
    return dict(points0=x0, pixels=px, conf=cf, cams=cams, dist=dist, truth=truth)


def plain_case_converging(B, V, J, name, conf="none", seed=13):
    """A plain-mode case whose status is compared exactly: run with max_iterations=50, the restatement converges within 20 trials in
    every item that iterates (asserted here, so that a marginal accept on the device has 30 trials of room)."""
    c = case(B, V, J, name, seed=seed, conf=conf)
    ref = refine(c["points0"], c["pixels"], c["conf"], c["cams"], c["dist"], None, 50, 1e-8)
    it = ref["status"] < 2
    assert (ref["status"][it] == 0).all() and (ref["iterations"][it] <= 20).all(), \
        "the restatement takes %d trials" % ref["iterations"].max()
    return c, ref


def mean_error(x, truth):
    d = np.linalg.norm(np.asarray(x, dtype=np.float64) - np.asarray(truth, dtype=np.float64), axis=-1)
    return float(np.nanmean(d)), float(np.nanmedian(d))
