"""Float64 restatement of openmpl_amd.geometry.refine_cameras / bundle_adjust (csrc/refine_cameras.hip) and the cases of their tests
(TEST INFRASTRUCTURE ONLY).

numpy float64 on the float32 inputs the kernel reads.  The reference has nothing comparable (PoseUtils.estimate_camera is a
weak-perspective fit), so there is no golden: the projection is tests/distortion_cases.project and the point Jacobian
tests/refine_cases.jacobian, both called, not re-derived -- d px / d x_cam is that Jacobian times R^T, which is R^-1 for the
orthonormal R the cases use.  The Levenberg-Marquardt loop is that of include/mpl_hip.h, all views in lockstep: a view that has
stopped keeps its state while the others go on.  The alternation rounds the points to float32 after every point step, as the device
hands them on.
"""
import numpy as np

from tests import refine_cases as rc
from tests import synth_cases as sc

LAMBDA0, LAMBDA_MIN, LAMBDA_MAX = rc.LAMBDA0, rc.LAMBDA_MIN, rc.LAMBDA_MAX
SMALL_ANGLE2 = 1e-8
MIN_OBSERVATIONS = 3


# ----------------------------------------------------------------------------------------------------- pose, Jacobian, cost
def rodrigues(w):
    """exp([w]x) for w (..., 3) -> (..., 3, 3): I + a K + b K^2, K^2 = w w^T - |w|^2 I; the series below |w|^2 = SMALL_ANGLE2"""
    w = np.asarray(w, dtype=np.float64)
    th2 = np.sum(w * w, axis=-1)
    with np.errstate(all="ignore"):
        th = np.sqrt(th2)
        small = th2 < SMALL_ANGLE2
        safe = np.where(small, 1.0, th)
        a = np.where(small, 1.0 - th2 / 6.0, np.sin(safe) / safe)
        b = np.where(small, 0.5 - th2 / 24.0, (1.0 - np.cos(safe)) / np.where(small, 1.0, th2))
        a, b = np.where(np.isnan(th2), np.nan, a), np.where(np.isnan(th2), np.nan, b)
        K = np.zeros(w.shape[:-1] + (3, 3))
        K[..., 0, 1], K[..., 0, 2] = -w[..., 2], w[..., 1]
        K[..., 1, 0], K[..., 1, 2] = w[..., 2], -w[..., 0]
        K[..., 2, 0], K[..., 2, 1] = -w[..., 1], w[..., 0]
        K2 = w[..., :, None] * w[..., None, :] - th2[..., None, None] * np.eye(3)
        return np.eye(3) + a[..., None, None] * K + b[..., None, None] * K2


def apply(cam, delta):
    """the camera record(s) cam (..., 16) at the trial pose R' = exp([w]x) R, t' = t + dt, delta = (w, dt) (..., 6)"""
    cam = np.asarray(cam, dtype=np.float64)
    delta = np.asarray(delta, dtype=np.float64)
    out = cam.copy()
    R = cam[..., 4:13].reshape(cam.shape[:-1] + (3, 3))
    with np.errstate(all="ignore"):
        out[..., 4:13] = np.einsum("...xy,...yz->...xz", rodrigues(delta[..., :3]), R).reshape(cam.shape[:-1] + (9,))
        out[..., 13:16] = cam[..., 13:16] + delta[..., 3:]
    return out


def participation(points, pixels, conf):
    """-> (part (B,V,J) bool, w (B,V,J) float64, 0 where the observation takes no part): refine_cases.participation and a finite point"""
    part, w = rc.participation(pixels, conf)
    part = part & np.isfinite(np.asarray(points, dtype=np.float64)).all(axis=-1)[:, None, :]
    return part, np.where(part, w, 0.0)


def jacobian(points, cams, dist):
    """d px / d (w, dt) -> (B,V,J,2,6): M [ -[x_cam]x | -R ] with M = d px / d x_cam = (d px / d X) R^T"""
    X = np.asarray(points, dtype=np.float64)
    cams = np.asarray(cams, dtype=np.float64)
    V = cams.shape[0]
    R, t = cams[:, 4:13].reshape(V, 3, 3), cams[:, 13:16]
    with np.errstate(all="ignore"):
        Jx = rc.jacobian(X, cams, dist)                                                      # M R
        xc = np.einsum("vxy,bvjy->bvjx", R, X[:, None, :, :] - t[None, :, None, :])
        M = np.einsum("bvjac,vkc->bvjak", Jx, R)
        K = np.zeros(xc.shape[:-1] + (3, 3))                                                 # -[x_cam]x
        K[..., 0, 1], K[..., 0, 2] = xc[..., 2], -xc[..., 1]
        K[..., 1, 0], K[..., 1, 2] = -xc[..., 2], xc[..., 0]
        K[..., 2, 0], K[..., 2, 1] = xc[..., 1], -xc[..., 0]
        return np.concatenate([np.einsum("bvjak,bvjkc->bvjac", M, K), -Jx], axis=-1)


def evaluate(points, pixels, conf, cams, dist, huber=None):
    """One evaluation at the poses of cams -> dict(E, S (V,): the cost in the mode of the call, +inf where a participating point is
    not in front, and the plain sum w |r|^2; W (V,) = sum w; H (V,6,6), g (V,6): the normal equations with the IRLS weights;
    zmin (V,); behind (V,); used (V,) ints)"""
    cams = np.asarray(cams, dtype=np.float64)
    dist = np.zeros((cams.shape[0], 5)) if dist is None else np.asarray(dist, dtype=np.float64)
    X = np.asarray(points, dtype=np.float64)
    part, w = participation(X, pixels, conf)
    Xs = np.where(np.isfinite(X).all(axis=-1, keepdims=True), X, 0.0)                        # a point that takes no part anywhere
    r, zc = rc.residuals(Xs, pixels, cams, dist)
    Jm = jacobian(Xs, cams, dist)
    with np.errstate(all="ignore"):
        behind = (part & ~(zc > sc.Z_MIN)).any(axis=(0, 2))
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
        E = np.sum(w * rho, axis=(0, 2))
        H = np.einsum("bvj,bvjac,bvjad->vcd", wi, Jm, Jm)
        g = np.einsum("bvj,bvjac,bvja->vc", wi, Jm, r)
        zmin = np.where(part, zc, np.inf).min(axis=(0, 2))
    return dict(E=np.where(behind, np.inf, E), S=np.sum(w * s, axis=(0, 2)), W=w.sum(axis=(0, 2)), H=H, g=g, zmin=zmin, behind=behind,
                used=part.sum(axis=(0, 2)))


def cost(points, pixels, conf, cams, dist, huber=None):
    return evaluate(points, pixels, conf, cams, dist, huber)["E"]


def lm_step(H, g, lam):
    """(H + lambda diag H) delta = -g for H (V,6,6) by the unpivoted Cholesky factorisation of the kernel; a pivot that is <= 0 or
    not finite gives a NaN delta"""
    V = H.shape[0]
    A = H.copy()
    for k in range(6):
        A[:, k, k] = H[:, k, k] + lam * H[:, k, k]
    L = np.zeros((V, 6, 6))
    ok = np.ones(V, bool)
    with np.errstate(all="ignore"):
        for j in range(6):
            d = A[:, j, j].copy()
            for k in range(j):
                d = d - L[:, j, k] * L[:, j, k]
            ok &= (d > 0.0) & np.isfinite(d)
            L[:, j, j] = np.sqrt(d)
            for i in range(j + 1, 6):
                s = A[:, j, i].copy()
                for k in range(j):
                    s = s - L[:, i, k] * L[:, j, k]
                L[:, i, j] = s / L[:, j, j]
        y = np.zeros((V, 6))
        for i in range(6):
            s = -g[:, i]
            for k in range(i):
                s = s - L[:, i, k] * y[:, k]
            y[:, i] = s / L[:, i, i]
        x = np.zeros((V, 6))
        for i in range(5, -1, -1):
            s = y[:, i].copy()
            for k in range(i + 1, 6):
                s = s - L[:, k, i] * x[:, k]
            x[:, i] = s / L[:, i, i]
    return np.where(ok[:, None], x, np.nan)


def _table(cams, dist):
    return np.zeros((np.asarray(cams).shape[0], 5)) if dist is None else np.asarray(dist, dtype=np.float64)


def _take(mask, new, old):
    return np.where(mask.reshape(mask.shape + (1,) * (new.ndim - mask.ndim)), new, old)


# ------------------------------------------------------------------------------------------------------------------ the call
def refine(points, pixels, conf, cams, dist=None, huber=None, max_iterations=20, step_tolerance=1e-8, fixed=()):
    """refine_cameras -> dict(cams (V,16), error, cost0, cost (V,) (NaN for an invalid view), used, iterations, status (V,) ints,
    accepted (V,): accepted trials, zmin (V,): the smallest participating depth at the final pose)"""
    cams0 = np.asarray(cams, dtype=np.float64)
    V = cams0.shape[0]
    args = (points, pixels, conf)
    cur = evaluate(*args, cams0, dist, huber)
    used = cur["used"]
    is_fixed = np.zeros(V, bool)
    is_fixed[list(fixed)] = True
    invalid = (used == 0) | ~np.isfinite(cams0).all(axis=1) | cur["behind"]
    passed = ~invalid & (is_fixed | (max_iterations == 0) | (used < MIN_OBSERVATIONS))
    live = ~invalid & ~passed
    status = np.where(invalid, 3, np.where(passed, 2, 1))
    C, E0 = cams0.copy(), cur["E"].copy()
    lam = np.full(V, LAMBDA0)
    iters, accepted = np.zeros(V, int), np.zeros(V, int)
    with np.errstate(all="ignore"):
        for _ in range(max_iterations):
            if not live.any():
                break
            delta = lm_step(cur["H"], cur["g"], lam)
            Ct = _take(live, apply(C, delta), C)
            tr = evaluate(*args, Ct, dist, huber)
            acc = live & (tr["E"] < cur["E"])                    # strictly lower: +inf and NaN are never accepted
            C = _take(acc, Ct, C)
            for k in ("E", "S", "H", "g", "zmin"):
                cur[k] = _take(acc, tr[k], cur[k])
            lam = np.where(acc, np.maximum(lam / 10.0, LAMBDA_MIN), np.where(live, lam * 10.0, lam))
            iters += live
            accepted += acc
            conv = live & (np.abs(delta[:, :3]).max(axis=1) <= step_tolerance) & \
                (np.abs(delta[:, 3:]).max(axis=1) <= step_tolerance * cur["zmin"])
            status = np.where(conv, 0, status)
            live = live & ~conv & ~(lam > LAMBDA_MAX)
        error = np.where(invalid, np.nan, np.sqrt(cur["S"] / cur["W"]))
    return dict(cams=C, error=error, cost0=np.where(invalid, np.nan, E0), cost=np.where(invalid, np.nan, cur["E"]), used=used,
                iterations=iters, status=status, accepted=accepted, zmin=cur["zmin"])


def score(points, pixels, conf, cams, dist, huber=None):
    """what the device reports at a pose it is handed: (error, E) per view, NaN where the view is invalid there"""
    e = evaluate(points, pixels, conf, cams, dist, huber)
    bad = (e["used"] == 0) | ~np.isfinite(np.asarray(cams, dtype=np.float64)).all(axis=1) | e["behind"]
    with np.errstate(all="ignore"):
        return np.where(bad, np.nan, np.sqrt(e["S"] / e["W"])), np.where(bad, np.nan, e["E"])


def bundle_adjust(points, pixels, conf, cams, dist=None, huber=None, rounds=5, fixed=(), max_iterations=20, step_tolerance=1e-8):
    """bundle_adjust -> dict(points (B,J,3) float32, cams (V,16), cost (rounds+1,), cameras, refined: the last round's dicts,
    slack (rounds,): what the float32 rounding of round r's points can add to cost[r + 1], the sum of refine_cases.rounding_slack)"""
    X = np.asarray(points, dtype=np.float32)
    C = np.asarray(cams, dtype=np.float64)
    costs, slack, cameras, refined = [], [], None, None
    for _ in range(rounds):
        cameras = refine(X, pixels, conf, C, dist, huber, max_iterations, step_tolerance, fixed)
        C = cameras["cams"]
        costs.append(cameras["cost0"].sum())
        refined = rc.refine(X, pixels, conf, C, dist, huber, max_iterations, step_tolerance)
        X = refined["points"].astype(np.float32)
        ok = np.isfinite(X).all(axis=-1)
        slack.append(float(np.sum(rc.rounding_slack(np.where(ok[..., None], X, 0.0), pixels, conf, C, _table(C, dist), huber)[ok])))
    costs.append(refine(X, pixels, conf, C, dist, huber, 0, step_tolerance, fixed)["cost0"].sum())
    return dict(points=X, cams=C, cost=np.array(costs), cameras=cameras, refined=refined, slack=np.array(slack))


# -------------------------------------------------------------------------------------------------------------------- cases
def perturb(cams, degrees, shift, seed, keep=()):
    """every camera not in `keep` turned by `degrees` about a random axis and its centre moved by `shift` in a random direction"""
    cams = np.asarray(cams, dtype=np.float64)
    rs = np.random.RandomState(seed)
    V = cams.shape[0]
    axis, way = rs.randn(V, 3), rs.randn(V, 3)
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    way /= np.linalg.norm(way, axis=1, keepdims=True)
    delta = np.concatenate([axis * np.deg2rad(degrees), way * shift], axis=1)
    delta[list(keep)] = 0.0
    out = apply(cams, delta)
    out[list(keep)] = cams[list(keep)]
    return out


def case(B, V, J, name="h36m", seed=13, noise=2.0, conf="none", degrees=2.0, shift=0.05, keep=(), nan_points=0, pseed=5):
    """refine_cases.case with the true points as the 3D input (`points`, float32) and a perturbed rig (`cams0`); nan_points = n > 0
    makes every n-th point NaN.  -> the dict of refine_cases.case plus points, cams0"""
    c = rc.case(B, V, J, name, seed=seed, noise=noise, conf=conf, start="exact")
    pts = c["truth"].astype(np.float32).copy()
    if nan_points:
        flat = pts.reshape(-1, 3)
        idx = np.arange(nan_points - 1, len(flat), nan_points)
        flat[idx, idx % 3] = np.nan                                # one coordinate is enough
    c["points"] = pts
    c["cams0"] = perturb(c["cams"], degrees, shift, pseed + 31 * V + B, keep)
    return c


def sure(ref, max_iterations):
    """the views of a restated run whose status is compared exactly and whose pose is compared at all: converged with more than half
    of the cap to spare, so that a marginal accept on the device has that many trials of room; and the views that never iterate"""
    return (ref["status"] >= 2) | ((ref["status"] == 0) & (ref["iterations"] <= max_iterations * 2 // 5))


def converging_case(B, V, J, name, huber=None, max_iterations=50, **kw):
    """A case in which every view that iterates converges within 2/5 of the cap (asserted here) -> (case, restated run)"""
    c = case(B, V, J, name, **kw)
    ref = refine(c["points"], c["pixels"], c["conf"], c["cams0"], c["dist"], huber, max_iterations, 1e-8)
    assert sure(ref, max_iterations).all(), "the restatement takes %d trials, status %s" % (ref["iterations"].max(), ref["status"])
    return c, ref


def closed_loop_case(seed=5):
    """the closed loop of the issue: (64,4,17), H36M-like lens, 2 px of noise, cameras 2 and 3 turned by 2 degrees and moved by 0.05
    units, cameras 0 and 1 exact and fixed -> (case, perturbed cams)"""
    c = rc.case(64, 4, 17, "h36m", noise=2.0)
    return c, perturb(c["cams"], 2.0, 0.05, seed, keep=(0, 1))


def rotation_error(cams):
    R = np.asarray(cams)[:, 4:13].reshape(-1, 3, 3)
    return float(np.abs(np.einsum("vxy,vzy->vxz", R, R) - np.eye(3)).max())
