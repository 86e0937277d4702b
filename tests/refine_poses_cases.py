"""Float64 restatement of openmpl_amd.geometry.refine_poses (csrc/refine_poses.hip) and the cases of its tests (TEST INFRASTRUCTURE
ONLY).

numpy float64 on the float32 inputs the kernel reads, nothing rounded.  The reprojection part is refine_cases.evaluate, called with
the weights of the joints that take no part set to zero; the projection behind it is distortion_cases.project.  What is stated here:
the participation rules of a pose, the bone term, the normal equations on the tree, their solve without fill-in, and the
Levenberg-Marquardt loop of include/mpl_hip.h with all poses in lockstep.

    E(X) = sum_{v,j} w_vj rho(|proj_v(X_j) - px_vj|^2) + bone_weight sum_{live bones j} ((|X_j - X_p(j)| - L_j) / L_j)^2
"""
import functools

import numpy as np

from tests import refine_cases as rc

LAMBDA0, LAMBDA_MIN, LAMBDA_MAX = rc.LAMBDA0, rc.LAMBDA_MIN, rc.LAMBDA_MAX
HUMAN = (-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 9, 8, 11, 12, 8, 14, 15)        # lib/multiviews/body.py as parents, as openmpl_amd.rpsm has it
BONE_WEIGHT = 1e4


# --------------------------------------------------------------------------------------------------------------------- trees
def tree(kind, J, seed=0):
    """parents of J joints: "human" (the first J joints of the body, which is a tree for every J), "chain" [-1, 0, 1, ...], "star"
    [-1, 0, 0, ...], "random" (parents[j] < j, numpy RandomState)"""
    if kind == "human":
        assert J <= len(HUMAN)
        return list(HUMAN[:J])
    if kind == "chain":
        return [j - 1 for j in range(J)]
    if kind == "star":
        return [-1] + [0] * (J - 1)
    assert kind == "random", kind
    rs = np.random.RandomState(seed * 7919 + J)
    return [-1] + [int(rs.randint(0, j)) for j in range(1, J)]


def depths(parents):
    out = []
    for j in range(len(parents)):
        d, k = 0, j
        while parents[k] != -1:
            k, d = parents[k], d + 1
        out.append(d)
    return out


def _par(parents):
    """parents as an index array, the root pointing at itself, and the mask of the joints that have a bone"""
    p = np.asarray(parents, dtype=np.int64)
    return np.where(p < 0, np.arange(len(p)), p), p >= 0


def bone_lengths(points, parents):
    X = np.asarray(points, dtype=np.float64)
    par, has = _par(parents)
    return np.where(has, np.linalg.norm(X - X[:, par], axis=-1), 0.0)


def limb_of(limb, B):
    L = np.asarray(limb, dtype=np.float64)
    return np.broadcast_to(L, (B, L.shape[-1])) if L.ndim == 1 else L


# ------------------------------------------------------------------------------------------------------------- participation
def participation(points, pixels, conf, limb, parents):
    """-> dict(view (B,V,J): the views that take part in a joint that takes part, w (B,V,J): their weights, 0 elsewhere,
    joint (B,J), live (B,J): the bone of child j is live)"""
    X = np.asarray(points, dtype=np.float64)
    part, w = rc.participation(pixels, conf)
    nv = part.sum(axis=1)
    par, has = _par(parents)
    L = limb_of(limb, X.shape[0])
    anchored = np.isfinite(X).all(axis=-1) & (nv >= 1)                    # a finite point and a participating view
    with np.errstate(invalid="ignore"):
        live = has & anchored & anchored[:, par] & np.isfinite(L) & (L > 0)
    tied = live.copy()
    for j in range(len(par)):
        tied[:, par[j]] |= live[:, j]
    joint = anchored & ((nv >= 2) | tied)
    view = part & joint[:, None, :]
    return dict(view=view, w=np.where(view, w, 0.0), joint=joint, live=live)


# ---------------------------------------------------------------------------------------------- cost and normal equations
def evaluate(X, pixels, cams, dist, huber, P, limb, parents, bone_weight):
    """One evaluation at X (B,J,3) with the participation P -> dict(E (B,): the cost in the mode of the call, +inf where a joint
    that takes part is behind a view that takes part; H (B,J,3,3): the diagonal blocks, the bones in them; g (B,J,3); u (B,J,3),
    c (B,J): the bone of child j is the off-diagonal block -c u u^T between j and its parent; zmin (B,); S (B,J): the plain sum
    w |r|^2; r_bone (B,J): |d| - L, NaN where the bone is not live)"""
    X = np.asarray(X, dtype=np.float64)
    B, J = X.shape[:2]
    par, _ = _par(parents)
    L = limb_of(limb, B)
    e = rc.evaluate(np.where(P["joint"][..., None], X, 0.0), pixels, P["w"].astype(np.float64), cams, dist, huber)
    H, g = e["H"].copy(), e["g"].copy()
    with np.errstate(all="ignore"):
        d = X - X[:, par]
        n = np.sqrt(np.sum(d * d, axis=-1))
        live = P["live"]
        Ls = np.where(live, L, 1.0)
        r = np.where(live, (n - Ls) / Ls, 0.0)
        u = np.where((live & (n > 0))[..., None], d / np.where(n > 0, n, 1.0)[..., None], 0.0)
        c = np.where(live, bone_weight / (Ls * Ls), 0.0)
        gr = bone_weight * r / Ls
        E = np.sum(e["E"], axis=1) + np.sum(bone_weight * r * r, axis=1)
    uu = c[..., None, None] * u[..., :, None] * u[..., None, :]
    H += uu
    g += gr[..., None] * u
    for j in range(J):                                       # the parent's share, its children in index order
        if parents[j] >= 0:
            H[:, par[j]] += uu[:, j]
            g[:, par[j]] -= gr[:, j, None] * u[:, j]
    zmin = np.where(P["joint"], e["zmin"], np.inf).min(axis=1)
    behind = (e["behind"] & P["joint"]).any(axis=1)
    return dict(E=E, H=H, g=g, u=u, c=c, zmin=zmin, S=e["S"], r_bone=np.where(live, n - L, np.nan), behind=behind)


def cost(X, pixels, conf, cams, dist, huber, limb, parents, bone_weight=BONE_WEIGHT, given=None):
    """E (B,) at X under the participation of the points `given` (default: X itself)"""
    dist = np.zeros((np.asarray(cams).shape[0], 5)) if dist is None else dist
    P = participation(X if given is None else given, pixels, conf, limb, parents)
    return evaluate(X, pixels, cams, dist, huber, P, limb, parents, bone_weight)["E"]


def dense_system(ev, lam, P, parents):
    """(A (B,3J,3J), rhs (B,3J)) of (H + lambda diag H) delta = -g, the joints that take no part as identity rows"""
    B, J = ev["c"].shape
    A, rhs = np.zeros((B, 3 * J, 3 * J)), np.zeros((B, 3 * J))
    for j in range(J):
        s = slice(3 * j, 3 * j + 3)
        Hj = ev["H"][:, j] * (1.0 + lam[:, None, None] * np.eye(3))
        A[:, s, s] = np.where(P["joint"][:, j, None, None], Hj, np.eye(3))
        rhs[:, s] = np.where(P["joint"][:, j, None], -ev["g"][:, j], 0.0)
        if parents[j] >= 0:
            q = slice(3 * parents[j], 3 * parents[j] + 3)
            O = -ev["c"][:, j, None, None] * ev["u"][:, j, :, None] * ev["u"][:, j, None, :]
            A[:, s, q] = O
            A[:, q, s] = O
    return A, rhs


def solve3(A, b):
    """A x = b for symmetric 3x3 A (..., 3, 3) by A = L D L^T without pivoting, the closed form of the kernel; a pivot that is not
    positive and finite gives NaN"""
    with np.errstate(all="ignore"):
        d0 = A[..., 0, 0]
        i0 = 1.0 / d0
        l10, l20 = A[..., 0, 1] * i0, A[..., 0, 2] * i0
        d1 = A[..., 1, 1] - l10 * A[..., 0, 1]
        t = A[..., 1, 2] - l20 * A[..., 0, 1]
        i1 = 1.0 / d1
        l21 = t * i1
        d2 = A[..., 2, 2] - l20 * A[..., 0, 2] - l21 * t
        i2 = 1.0 / d2
        y0 = b[..., 0]
        y1 = b[..., 1] - l10 * y0
        y2 = b[..., 2] - l20 * y0 - l21 * y1
        x2 = y2 * i2
        x1 = y1 * i1 - l21 * x2
        x0 = y0 * i0 - l10 * x1 - l20 * x2
        ok = (d0 > 0) & (d1 > 0) & (d2 > 0) & np.isfinite(d0) & np.isfinite(d1) & np.isfinite(d2)
        return np.where(ok[..., None], np.stack([x0, x1, x2], axis=-1), np.nan)


def tree_solve(ev, lam, P, parents):
    """(H + lambda diag H) delta = -g on the tree -> delta (B,J,3), 0 for a joint that takes no part.  Children before parents:
    with the block -c u u^T between child j and its parent, y = D_j^-1 rhs_j and z = D_j^-1 u leave the parent
    D_p -= c^2 (u.z) u u^T and rhs_p += c (u.y) u; then root first, delta_j = y + c (u.delta_p) z.  No fill-in."""
    B, J = ev["c"].shape
    D = ev["H"] * (1.0 + lam[:, None, None, None] * np.eye(3))
    rhs = -ev["g"].copy()
    u, c = ev["u"], ev["c"]
    dep = depths(parents)
    y, z = np.zeros((B, J, 3)), np.zeros((B, J, 3))
    with np.errstate(all="ignore"):
        for lev in range(max(dep), -1, -1):
            for j in range(J):
                if dep[j] != lev:
                    continue
                y[:, j] = np.where(P["joint"][:, j, None], solve3(D[:, j], rhs[:, j]), 0.0)
                if parents[j] < 0:
                    continue
                tied = P["live"][:, j] & (c[:, j] > 0)
                z[:, j] = np.where(tied[:, None], solve3(D[:, j], u[:, j]), 0.0)
                a = np.where(tied, c[:, j] * c[:, j] * np.sum(u[:, j] * z[:, j], axis=-1), 0.0)
                b = np.where(tied, c[:, j] * np.sum(u[:, j] * y[:, j], axis=-1), 0.0)
                D[:, parents[j]] -= a[:, None, None] * u[:, j, :, None] * u[:, j, None, :]
                rhs[:, parents[j]] += b[:, None] * u[:, j]
        delta = np.zeros((B, J, 3))
        for lev in range(0, max(dep) + 1):
            for j in range(J):
                if dep[j] != lev:
                    continue
                delta[:, j] = y[:, j]
                if parents[j] >= 0:
                    tied = P["live"][:, j] & (c[:, j] > 0)
                    s = np.where(tied, c[:, j] * np.sum(u[:, j] * delta[:, parents[j]], axis=-1), 0.0)
                    delta[:, j] = np.where(tied[:, None], y[:, j] + s[:, None] * z[:, j], y[:, j])
    return delta


# ------------------------------------------------------------------------------------------------------------------ the call
def refine(points, pixels, conf, cams, limb, parents, dist=None, huber=None, bone_weight=BONE_WEIGHT, max_iterations=50,
           step_tolerance=1e-8):
    """refine_poses -> dict(points (B,J,3), error (B,J), bone_error (B,J), cost0, cost (B,), iterations, status (B,) ints,
    accepted (B,), joint (B,J), live (B,J), zmin (B,))"""
    X0 = np.asarray(points, dtype=np.float64)
    cams = np.asarray(cams, dtype=np.float64)
    dist = np.zeros((cams.shape[0], 5)) if dist is None else np.asarray(dist, dtype=np.float64)
    P = participation(X0, pixels, conf, limb, parents)
    args = (pixels, cams, dist, huber, P, limb, parents, float(bone_weight))
    B = X0.shape[0]
    Xz = np.where(P["joint"][..., None], X0, 0.0)              # what takes no part never enters the arithmetic
    cur = evaluate(Xz, *args)
    invalid = cur["behind"]
    passed = ~invalid & (~P["joint"].any(axis=1) | (max_iterations == 0))
    live = ~invalid & ~passed
    status = np.where(invalid, 3, np.where(passed, 2, 1))
    X, E0 = Xz.copy(), cur["E"].copy()
    lam = np.full(B, LAMBDA0)
    iters, accepted = np.zeros(B, int), np.zeros(B, int)
    with np.errstate(all="ignore"):
        for _ in range(max_iterations):
            if not live.any():
                break
            delta = tree_solve(cur, lam, P, parents)
            Xt = np.where(live[:, None, None], X + delta, X)
            tr = evaluate(Xt, *args)
            acc = live & (tr["E"] < cur["E"])                    # strictly lower: +inf and NaN are never accepted
            X = rc._take(acc, Xt, X)
            for k in ("E", "H", "g", "u", "c", "zmin", "S", "r_bone"):
                cur[k] = rc._take(acc, tr[k], cur[k])
            lam = np.where(acc, np.maximum(lam / 10.0, LAMBDA_MIN), np.where(live, lam * 10.0, lam))
            iters += live
            accepted += acc
            conv = live & (np.abs(delta).max(axis=(1, 2)) <= step_tolerance * cur["zmin"])
            status = np.where(conv, 0, status)
            live = live & ~conv & ~(lam > LAMBDA_MAX)
        error = np.where(P["joint"] & ~invalid[:, None], np.sqrt(cur["S"] / P["w"].sum(axis=1)), np.nan)
    out = np.where(P["joint"][..., None], X, X0)
    return dict(points=np.where(invalid[:, None, None], np.nan, out), error=error,
                bone_error=np.where(invalid[:, None], np.nan, cur["r_bone"]), cost0=np.where(invalid, np.nan, E0),
                cost=np.where(invalid, np.nan, cur["E"]), iterations=iters, status=status, accepted=accepted, joint=P["joint"],
                live=P["live"], zmin=cur["zmin"])


def rounding_slack(X, pixels, conf, cams, dist, huber, limb, parents, bone_weight=BONE_WEIGHT, given=None):
    """How much one fp32 rounding of every coordinate of the pose X can add to E, (B,), as refine_cases.rounding_slack derives it
    for one point: with |e_c| <= ulp32(X_c) / 2 and E a sum of squares around X, E(X + e) - E(X) ~ 2 g.e + e^T H e, and because H
    is positive semi-definite e^T H e <= (sum_jc sqrt(H_jc,jc) |e_jc|)^2, the bones included through the diagonal of H; doubled for
    what Gauss-Newton leaves out."""
    dist = np.zeros((np.asarray(cams).shape[0], 5)) if dist is None else dist
    P = participation(X if given is None else given, pixels, conf, limb, parents)
    e = evaluate(X, pixels, cams, dist, huber, P, limb, parents, bone_weight)
    half = 0.5 * np.spacing(np.abs(np.asarray(X, dtype=np.float64)).astype(np.float32)).astype(np.float64)
    half = np.where(P["joint"][..., None], half, 0.0)
    Hd = np.stack([e["H"][..., k, k] for k in range(3)], axis=-1)
    return 2.0 * (2.0 * np.sum(np.abs(e["g"]) * half, axis=(1, 2)) + np.sum(np.sqrt(Hd) * half, axis=(1, 2)) ** 2)


# -------------------------------------------------------------------------------------------------------------------- cases
def case(B, V, J, kind="human", name="h36m", conf="none", limb="pose", seed=13, noise=2.0, start="linear", limb_error=0.0):
    """refine_cases.case with a tree and bone lengths: parents, and limb -- "pose": (B,J) float32, the bone lengths of the true
    pose; "shared": (J,) float32, their median over the batch; limb_error scales them by (1 + limb_error)."""
    c = rc.case(B, V, J, name, seed=seed, noise=noise, conf=conf, start=start)
    c["parents"] = tree(kind, J, seed)
    L = bone_lengths(c["truth"], c["parents"]) * (1.0 + limb_error)
    c["limb"] = (np.median(L, axis=0) if limb == "shared" else L).astype(np.float32)
    return c


def occlusion_case(B=32, V=4, J=17, seed=13, keep=0.3, start_noise=0.05):
    """The model's prediction against occluded detections: a joint keeps one view only with probability `keep` (conf 0 in the
    others); the start is the truth plus `start_noise` units of Gaussian noise.  -> (case, one (B,J) bool: the one-view joints)"""
    c = case(B, V, J, "human", "h36m", seed=seed)
    rs = np.random.RandomState(seed + 977)
    one = rs.rand(B, J) < keep
    kept = rs.randint(0, V, (B, J))
    cf = np.ones((B, V, J), np.float32)
    cf[one[:, None, :] & (np.arange(V)[None, :, None] != kept[:, None, :])] = 0.0
    c["conf"] = cf
    c["points0"] = (c["truth"].astype(np.float64) + start_noise * rs.randn(B, J, 3)).astype(np.float32)
    return c, one


def run(c, huber=None, bone_weight=BONE_WEIGHT, max_iterations=50, lens=True, **kw):
    return refine(kw.get("points", c["points0"]), c["pixels"], kw.get("conf", c["conf"]), c["cams"], kw.get("limb", c["limb"]),
                  kw.get("parents", c["parents"]), c["dist"] if lens else None, huber, bone_weight, max_iterations, 1e-8)


def converging(c, ref, max_iterations):
    """what a parity case asserts: every pose that iterates converges in at most half of the trials it is run with, so that a
    marginal accept on the device has room"""
    it = ref["status"] < 2
    assert (ref["status"][it] == 0).all() and (ref["iterations"][it] <= max_iterations // 2).all(), \
        "the restatement takes %d trials of %d, statuses %s" % (ref["iterations"].max(initial=0), max_iterations, ref["status"])
    return ref


# ------------------------------------------------------------------------------------------- what the tests share, computed once
SHARED_WEIGHT = 1e2        # the poses of synth_cases.scene share no skeleton: the median length is tens of per cent off a pose's own,
#                            and at the default weight that is a large-residual problem on which Gauss-Newton crawls


@functools.lru_cache(maxsize=None)
def parity_case(B, V, J, kind, name, conf, limb, huber):
    """A case of the parity grid and the restatement's run of it -> (case, ref, the keyword arguments of the run).  limb="pose" at
    the default weight, "shared" at SHARED_WEIGHT.  Plain mode: asserted to converge in at most half of the trials it is run with;
    Huber mode: run at the default cap, and may end capped."""
    c = case(B, V, J, kind, name, conf, limb)
    kw = dict(huber=huber, bone_weight=BONE_WEIGHT if limb == "pose" else SHARED_WEIGHT,
              max_iterations=50 if huber is not None or limb == "pose" else 100)
    ref = run(c, **kw)
    return c, (converging(c, ref, kw["max_iterations"]) if huber is None else ref), kw


@functools.lru_cache(maxsize=None)
def two_view_loop():
    """(32,2,17) under the "h36m" lens with the true bone lengths of every pose -> (case, ref, refine_cases.refine of the same)"""
    c = case(32, 2, 17)
    return c, converging(c, run(c, max_iterations=100), 100), rc.refine(c["points0"], c["pixels"], None, c["cams"], c["dist"])


@functools.lru_cache(maxsize=None)
def four_view_loop():
    c = case(32, 4, 17)
    return c, converging(c, run(c), 50), rc.refine(c["points0"], c["pixels"], None, c["cams"], c["dist"])


@functools.lru_cache(maxsize=None)
def occlusion_loop():
    c, one = occlusion_case()
    return c, one, run(c, max_iterations=100)


def joint_errors(x, truth):
    return np.linalg.norm(np.asarray(x, dtype=np.float64) - np.asarray(truth, dtype=np.float64), axis=-1)
