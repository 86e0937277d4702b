"""Float64 restatement of openmpl_amd/procrustes.py and the inputs of its tests (TEST INFRASTRUCTURE ONLY).

numpy float64 (numpy.linalg.svd) on the float32 inputs the kernel reads, pinned by tests/golden/procrustes.npz, which the
reference's own PoseUtils.procrustes produced (tests/golden/make_golden_procrustes.py).  On top of the reference's lines it
states what the kernel adds: participation (joint selection, confidences), de-normalisation on load, the degenerate poses and the
coplanar rule.  d is summed on the points (the reference's 1 - S^2 is the same number and cancels where the fit is good).
"""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RANK_TOL = 1e-12                 # s[1] / s[0] at or below: collinear (NaN); s[2] / s[0] at or below: coplanar (proper rotation)
MODES = [(scaling, reflection) for scaling in (True, False) for reflection in ("best", False, True)]
FIELDS = ("aligned", "d", "rotation", "scale", "translation")


def golden():
    g = np.load(os.path.join(GOLD, "procrustes.npz"))
    return {k: g[k] for k in g.files}


def mode_tag(scaling, reflection):
    return "%s_%s" % ("s" if scaling else "r", {"best": "best", False: "off", True: "on"}[reflection])


def rel_errors(got, ref):
    """the parity rule of DESIGN.md section 2: (max|d| / max|ref|, ||d||_2 / ||ref||_2) over the finite entries of ref;
    NaN must sit in the same places"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN in other places than the reference"
    ok = ~np.isnan(ref)
    d = got[ok] - ref[ok]
    if d.size == 0 or np.abs(ref[ok]).max() == 0:
        return float(np.abs(d).max(initial=0.0)), 0.0
    return float(np.abs(d).max() / np.abs(ref[ok]).max()), float(np.linalg.norm(d) / np.linalg.norm(ref[ok]))


def align_one(A, B, take, scaling=True, reflection="best"):
    """pose_utils.py:84-143 on one pose.  A, B: (J,3) float64, target and prediction; take: indices of the joints that take part
    (an index listed twice counts twice) -> (Z (J,3), d, R (3,3), scale, translation (3)), all NaN for a degenerate pose."""
    J = A.shape[0]
    nan = (np.full((J, 3), np.nan), np.nan, np.full((3, 3), np.nan), np.nan, np.full(3, np.nan))
    if len(take) < 3:
        return nan
    At, Bt = A[take], B[take]
    A_bar, B_bar = At.mean(0), Bt.mean(0)                            # :89-92
    A0, B0 = At - A_bar, Bt - B_bar
    ssX, ssY = (A0 ** 2).sum(), (B0 ** 2).sum()                       # :95-96
    if not (np.isfinite(ssX) and np.isfinite(ssY) and ssX > 0 and ssY > 0):
        return nan
    A_norm, B_norm = np.sqrt(ssX), np.sqrt(ssY)
    M = np.dot((A0 / A_norm).T, B0 / B_norm)                          # :99-106
    U, s, Vt = np.linalg.svd(M)
    V = Vt.T.copy()
    if not s[1] > RANK_TOL * s[0]:
        return nan
    if not s[2] > RANK_TOL * s[0]:                                    # coplanar: U and V completed by cross products
        U = U.copy()
        U[:, 2] = np.cross(U[:, 0], U[:, 1])
        V[:, 2] = np.cross(V[:, 0], V[:, 1])
    R = np.dot(V, U.T)                                                # :109
    s = s.copy()
    if reflection != "best":                                          # :111-119
        if bool(reflection) != bool(np.linalg.det(R) < 0):
            V[:, -1] *= -1
            s[-1] *= -1
            R = np.dot(V, U.T)
    S = s.sum()
    scale = S * A_norm / B_norm if scaling else 1.0                   # :124, :132
    Z = scale * np.dot(B - B_bar, R) + A_bar                          # :130, :134 (B_norm B0n = B0), for every joint
    d = ((Z[take] - At) ** 2).sum() / ssX
    return Z, d, R, scale, A_bar - scale * np.dot(B_bar, R)           # :139


def align(pred, target, conf=None, joints=None, scaling=True, reflection="best", scale=None, offset=None):
    """What openmpl_amd.procrustes_align returns, float64: dict(aligned (B,J,3), d (B), rotation (B,3,3), scale (B), translation (B,3))"""
    sc = np.ones(3) if scale is None else np.asarray(np.broadcast_to(np.asarray(scale, dtype=np.float32), (3,)), dtype=np.float64)
    of = np.zeros(3) if offset is None else np.asarray(np.broadcast_to(np.asarray(offset, dtype=np.float32), (3,)), dtype=np.float64)
    P = np.asarray(pred, dtype=np.float64) * sc + of
    T = np.asarray(target, dtype=np.float64) * sc + of
    Bn, J, _ = P.shape
    sel = np.arange(J) if joints is None else np.asarray([int(k) % J for k in joints])
    out = dict(aligned=np.zeros((Bn, J, 3)), d=np.zeros(Bn), rotation=np.zeros((Bn, 3, 3)), scale=np.zeros(Bn), translation=np.zeros((Bn, 3)))
    for b in range(Bn):
        take = sel
        if conf is not None:
            c = np.asarray(conf, dtype=np.float64).reshape(Bn, J)[b, sel]
            with np.errstate(invalid="ignore"):
                take = sel[np.isfinite(c) & (c > 0)]
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            res = align_one(T[b], P[b], take, scaling, reflection)
        for k, v in zip(FIELDS, res):
            out[k][b] = v
    return out


# ----------------------------------------------------------------------------- inputs
def rotation(rs):
    """a proper rotation, uniformly enough"""
    q, r = np.linalg.qr(rs.randn(3, 3))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 2] *= -1
    return q


def similarity_case(B, J, seed=0, noise=0.05, mirror=(), exact=False, room=2.0):
    """targets: J points of a pose about 1 m across, somewhere in a room (within `room` m of the origin); predictions: a random similarity of them (scale 0.5 .. 2,
    any rotation, a shift of up to 1 m) plus noise (relative to the spread), float32.  Poses listed in `mirror` are reflected.
    -> dict(pred, target (B,J,3) float32; s (B), R (B,3,3), t (B,3): pred = s * target @ R + t before noise and rounding)"""
    rs = np.random.RandomState(seed * 7919 + B * 131 + J)
    tgt = (rs.uniform(-0.5, 0.5, size=(B, J, 3)) + rs.uniform(-room, room, size=(B, 1, 3))).astype(np.float32)
    s = rs.uniform(0.5, 2.0, size=B)
    R = np.stack([rotation(rs) for _ in range(B)])
    for b in mirror:
        R[b] = R[b] @ np.diag([1.0, 1.0, -1.0])
    t = rs.uniform(-1.0, 1.0, size=(B, 3))
    pred = s[:, None, None] * np.einsum("bjx,bxy->bjy", tgt.astype(np.float64), R) + t[:, None, :]
    if not exact:
        pred = pred + noise * s[:, None, None] * 0.3 * rs.randn(B, J, 3)
    return dict(pred=pred.astype(np.float32), target=tgt, s=s, R=R, t=t)
