"""Float64 restatement of openmpl_amd.geometry.relative_pose (csrc/relative_pose.hip, csrc/five_point.hpp) and the cases of its tests
(TEST INFRASTRUCTURE ONLY).

numpy float64 on the float32 inputs the kernel reads, the five steps of include/mpl_hip.h in their order.  The reference has nothing
comparable, so there is no golden: the lens inverse is tests/distortion_cases.undistort_pixels, participation is
refine_cameras_cases.participation and the random numbers are openmpl_amd.detrng -- all called, not re-derived.  The five-point
solver is stated twice: `method="action"` eliminates the ten cubics in the graded order x^3 x^2y x^2z xy^2 xyz xz^2 y^3 y^2z yz^2
z^3 | x^2 xy xz y^2 yz z^2 x y z 1 and reads (x, y, z) off the right eigenvectors of the action matrix of x (what the tests compare
the device with), on the null space that numpy's SVD of the 5 x 9 system gives; `method="poly"` takes the null space from eigh of
A^T A, eliminates in Nister's order, forms the 3 x 3 polynomial matrix in z and takes numpy.roots of its determinant, the route of
the device.  Both polish (x, y, z) on the ten cubics, as the device does.  The distance between the two is the yardstick of the
comparison.

Measured with this file (test_relative_pose_cases_cpu.py prints them), numpy 2.x float64:
  * exact data (float64 pixels): the candidate nearest the true pose is 7e-15 (action) and 7e-12 (poly) off in the median, 5.6 real
    candidates a sample;
  * the winners of outlier_case() -- (8,4,17), 2 px of noise, a quarter of every view's detections planted 40 .. 120 px off, which
    leaves 73 and 76 of 136 correspondences clean, 256 hypotheses, threshold 6 px --: pair (0,1) winner 134 with 69 inliers, 1 of
    them planted, rotation off by 3.41 degrees and direction by 2.35; pair (2,3) winner 211 with 82 inliers, 6 planted, 1.92 and
    1.39 degrees (WINNER_DEGREES, WINNER_PLANTED are the bounds asserted: nothing tighter than that).  A planted detection moved
    along its epipolar line is an inlier of any two-view test;
  * over gpu_cases(): 93.8 to 100 % of the drawn hypotheses are well-conditioned (all of WELL_SV, WELL_PIVOT, WELL_PICK, WELL_ROOTS
    and a best candidate with more inliers than any other); over those the two formulations differ by at most 2.52e-9 (case
    outliers; 3e-11 .. 8e-10 in the others) in an entry of the best pose: FORMULATION_SPREAD; the device is allowed
    POSE_TOL = 100 times that, 2.6e-7.  In the case "five" every candidate fits the five correspondences and none is clear of
    another: its hypotheses are compared candidate by candidate (`tied`);
  * the restated polish (refine(), plain and Huber at 6 px, weights = the inliers) from the winners of outlier_case() against the same
    call from the true poses: 6 trials each, the poses agree to 2.68e-9 (POLISH_SPREAD), 1.31 / 0.58 and 0.50 / 0.35 degrees from the
    truth (rotation / direction) where the winners were 3.41 / 2.35 and 1.92 / 1.39; the analytic Jacobian is within 5e-8 of central
    differences at entries of up to 1.3e3.
"""
import numpy as np

from openmpl_amd import detrng
from tests import distortion_cases as dc
from tests import locate_cameras_cases as lc
from tests import refine_cameras_cases as cc

SAMPLE, ATTEMPTS, MIN_INLIERS, MAX_ROOTS = 5, 16, 6, 10
DEPTH_MIN = 1e-9
NEAR_THRESHOLD = 1e-9              # no d^2 of a case lies within this, relative, of threshold^2
FORMULATION_SPREAD = 2.6e-9        # measured 2.52e-9: max |pose(action) - pose(poly)| over the well-conditioned hypotheses of gpu_cases()
POSE_TOL = 100.0 * FORMULATION_SPREAD
POLISH_SPREAD = 2.7e-9             # measured 2.68e-9: the restated polish from the winners of outlier_case() against that from the true poses
WINNER_DEGREES, WINNER_PLANTED = (3.6, 2.5), 6      # rotation, direction: measured 3.41 and 2.35 at most; planted inliers 6 at most (see above)
# a hypothesis is well-conditioned when all of these hold
WELL_SV = 1e-4                     # the fifth singular value of the 5 x 9 sample system over the first
WELL_PIVOT = 1e-6                  # the smallest pivot of an elimination over the largest, in the graded and in Nister's order
WELL_PICK = 1e-9                   # the five largest diagonal entries of the null space's projector apart by this: the basis is picked alike
WELL_ROOTS = 1e-4                  # the separation of the roots: real from real, and complex from the real axis, over max(1, |z|)


# ------------------------------------------------------------------------------------------------------------ steps 1 and 2
def _table(cams, dist):
    return np.zeros((np.asarray(cams).shape[0], 5)) if dist is None else np.asarray(dist, dtype=np.float64)


def observations(pixels, conf, cams, dist, pairs):
    """step 1 -> dict(part (B,P,J) bool, w (B,P,J), ua, ub (B,P,J,2): the undistorted pixels, ya, yb (B,P,J,2): their normalised
    coordinates, usable (P,))"""
    cams = np.asarray(cams, dtype=np.float64)
    pixels = np.asarray(pixels)
    B, V, J = pixels.shape[:3]
    part, w = cc.participation(np.zeros((B, J, 3)), pixels, conf)
    with np.errstate(all="ignore"):
        und = dc.undistort_pixels(np.where(np.isfinite(pixels), pixels, 0.0), cams, _table(cams, dist))
        part = part & und["valid"] & np.isfinite(cams[:, :4]).all(axis=1)[None, :, None]
        fx, fy, cx, cy = dc._intrinsics(cams)
        u = np.where(part[..., None], und["pixels"], 0.0)
        y = np.where(part[..., None], np.stack([(u[..., 0] - cx) / fx, (u[..., 1] - cy) / fy], axis=-1), 0.0)
    a, b = [p[0] for p in pairs], [p[1] for p in pairs]
    both = part[:, a] & part[:, b]
    sel = lambda x, i: np.where(both[..., None], x[:, i], 0.0)      # noqa: E731
    return dict(part=both, w=np.where(both, w[:, a] * w[:, b], 0.0), ua=sel(u, a), ub=sel(u, b), ya=sel(y, a), yb=sel(y, b),
                usable=both.sum(axis=(0, 2)) >= SAMPLE)


def samples(part, seed, hypotheses):
    """step 2 -> (slots (P,H,5) ints, drawn (P,H) bool): slot n = b * J + j"""
    B, P, J = part.shape
    N = B * J
    slots, drawn = np.zeros((P, hypotheses, SAMPLE), int), np.zeros((P, hypotheses), bool)
    for p in range(P):
        flat = part[:, p].reshape(N)
        u = detrng.uniform01(seed, "relative_pose", hypotheses * SAMPLE * ATTEMPTS, lane=p)
        n = np.floor(u * N).astype(int).reshape(hypotheses, SAMPLE, ATTEMPTS)
        for h in range(hypotheses):
            chosen = []
            for k in range(SAMPLE):
                for a in range(ATTEMPTS):
                    if flat[n[h, k, a]] and n[h, k, a] not in chosen:
                        chosen.append(n[h, k, a])
                        break
                else:
                    break
            if len(chosen) == SAMPLE:
                slots[p, h], drawn[p, h] = chosen, True
    return slots, drawn


# -------------------------------------------------------------------------------------------------------- step 3, the solver
# a polynomial in (x, y, z) of degree <= 3 is an array (..., 4, 4, 4) indexed by the three exponents
def _grid(lin):
    """(..., 4) coefficients of x y z 1 -> the polynomial"""
    g = np.zeros(lin.shape[:-1] + (4, 4, 4))
    g[..., 1, 0, 0], g[..., 0, 1, 0], g[..., 0, 0, 1], g[..., 0, 0, 0] = lin[..., 0], lin[..., 1], lin[..., 2], lin[..., 3]
    return g


def _times(p, lin):
    """the polynomial p times x lin0 + y lin1 + z lin2 + lin3"""
    out = p * lin[..., 3, None, None, None]
    out[..., 1:, :, :] += p[..., :-1, :, :] * lin[..., 0, None, None, None]
    out[..., :, 1:, :] += p[..., :, :-1, :] * lin[..., 1, None, None, None]
    out[..., :, :, 1:] += p[..., :, :, :-1] * lin[..., 2, None, None, None]
    return out


GRADED = [(3, 0, 0), (2, 1, 0), (2, 0, 1), (1, 2, 0), (1, 1, 1), (1, 0, 2), (0, 3, 0), (0, 2, 1), (0, 1, 2), (0, 0, 3),
          (2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
NISTER = [(3, 0, 0), (0, 3, 0), (2, 1, 0), (1, 2, 0), (2, 0, 1), (2, 0, 0), (0, 2, 1), (0, 2, 0), (1, 1, 1), (1, 1, 0),
          (1, 0, 0), (1, 0, 1), (1, 0, 2), (0, 1, 0), (0, 1, 1), (0, 1, 2), (0, 0, 0), (0, 0, 1), (0, 0, 2), (0, 0, 3)]


def null_space(ya, yb, method="action"):
    """(N,5,2) twice -> (basis (N,4,3,3): X Y Z W, sv (N,5) descending, pick (N,): the smallest gap between two of the five largest
    diagonal entries of the projector).  A row of the 5 x 9 system is kron(d_b, d_a), so that row . vec(E) = d_b^T E d_a; the right
    singular vectors beyond the fifth span its null space (method "poly": the eigenvectors of A^T A at its four smallest eigenvalues),
    and X Y Z W are the columns of the projector on it at the four largest
    entries of its diagonal, in descending order, made orthonormal in that order: a basis that does not depend on the one the SVD
    returned"""
    da = np.concatenate([ya, np.ones(ya.shape[:-1] + (1,))], axis=-1)
    db = np.concatenate([yb, np.ones(yb.shape[:-1] + (1,))], axis=-1)
    A = np.einsum("nir,nic->nirc", db, da).reshape(len(ya), SAMPLE, 9)
    _, sv, Vt = np.linalg.svd(A)
    Nn = Vt[:, 5:]                                                   # (N,4,9), orthonormal rows
    if method == "poly":                                             # the second formulation: eigh of A^T A
        Nn = np.swapaxes(np.linalg.eigh(np.einsum("nki,nkj->nij", A, A))[1][:, :, :4], 1, 2)
    proj = np.einsum("nje,njf->nef", Nn, Nn)                         # the projector on the null space: the same for every basis of it
    diag = np.einsum("nee->ne", proj)
    order = np.argsort(-diag, axis=1, kind="stable")
    basis = np.take_along_axis(proj, order[:, :4, None], axis=1)     # its columns at the four largest diagonal entries, descending
    top = np.take_along_axis(diag, order, axis=1)
    q = np.zeros_like(basis)
    for k in range(4):                                               # Gram-Schmidt in that order, every projection taken twice
        v = basis[:, k].copy()
        for _ in range(2):
            for j in range(k):
                v -= np.einsum("ne,ne->n", q[:, j], v)[:, None] * q[:, j]
        q[:, k] = v / np.linalg.norm(v, axis=1)[:, None]
    return q.reshape(len(ya), 4, 3, 3), sv, (top[:, :-1] - top[:, 1:])[:, :4].min(axis=1)


def cubics(basis, order):
    """the ten cubics det E = 0, (E E^T - tr(E E^T) / 2) E = 0 of E = x X + y Y + z Z + W -> (N,10,20) in the monomials of `order`"""
    E = np.moveaxis(basis, 1, -1)                                    # (N,3,3,4): every entry a polynomial of degree 1
    g = _grid(E)
    rows = []
    det = 0.0
    for c in range(3):
        c1, c2 = (c + 1) % 3, (c + 2) % 3
        det = det + _times(_times(g[:, 1, c1], E[:, 2, c2]) - _times(g[:, 1, c2], E[:, 2, c1]), E[:, 0, c])
    rows.append(det)
    G = [[sum(_times(g[:, i, c], E[:, j, c]) for c in range(3)) for j in range(3)] for i in range(3)]
    tr = G[0][0] + G[1][1] + G[2][2]
    for i in range(3):
        G[i][i] = G[i][i] - 0.5 * tr
    for i in range(3):
        for j in range(3):
            rows.append(sum(_times(G[i][c], E[:, c, j]) for c in range(3)))
    M = np.stack(rows, axis=1)                                       # (N,10,4,4,4)
    return np.stack([M[:, :, a, b, c] for a, b, c in order], axis=-1)


def eliminate(M):
    """Gauss-Jordan on the first ten columns with partial pivoting -> (B (N,10,10): the right half of [I | B], ratio (N,): the
    smallest pivot over the largest, 0 where a pivot vanishes)"""
    M = M.copy()
    N = len(M)
    idx = np.arange(N)
    pmin, pmax = np.full(N, np.inf), np.zeros(N)
    with np.errstate(all="ignore"):
        for k in range(10):
            piv = np.argmax(np.abs(M[:, k:, k]), axis=1) + k
            rowp, rowk = M[idx, piv].copy(), M[idx, k].copy()
            best = np.abs(rowp[:, k])
            pmin, pmax = np.minimum(pmin, best), np.maximum(pmax, best)
            M[idx, piv] = rowk
            M[idx, k] = rowp / rowp[:, k:k + 1]
            f = M[:, :, k].copy()
            f[:, k] = 0.0
            M -= f[:, :, None] * M[idx, k][:, None, :]
        ratio = np.where(np.isfinite(pmin / pmax), pmin / pmax, 0.0)
    return M[:, :, 10:], ratio


def _candidates_action(basis):
    """-> (xyz (N,10,3) NaN-padded and sorted by z, roots (N,), ratio (N,), sep (N,))"""
    B, ratio = eliminate(cubics(basis, GRADED))
    N = len(B)
    A = np.zeros((N, 10, 10))
    A[:, :6] = -B[:, :6]
    A[:, 6, 0] = A[:, 7, 1] = A[:, 8, 2] = A[:, 9, 6] = 1.0
    ok = np.isfinite(A).all(axis=(1, 2))
    lam, vec = np.linalg.eig(np.where(ok[:, None, None], A, 0.0))
    xyz, roots, sep = np.full((N, MAX_ROOTS, 3), np.nan), np.zeros(N, int), np.zeros(N)
    with np.errstate(all="ignore"):
        for n in range(N):
            if not ok[n]:
                continue
            real = np.imag(lam[n]) == 0.0
            v = np.real(vec[n][:, real])
            sol = (v[6:9] / v[9]).T                                  # (roots, 3)
            sol = sol[np.argsort(sol[:, 2])]
            roots[n] = len(sol)
            xyz[n, :len(sol)] = sol
            z_all = vec[n][8] / vec[n][9]
            sep[n] = _separation(z_all, real)
    return xyz, roots, ratio, sep


def _separation(z, real):
    """the smallest distance of a real root to another, or of a complex root to the real axis, over max(1, |z|)"""
    gaps = [np.inf]
    zr = np.sort(np.real(z[real]))
    if len(zr) > 1:
        gaps.append(np.min(np.diff(zr) / np.maximum(1.0, np.maximum(np.abs(zr[1:]), np.abs(zr[:-1])))))
    if (~real).any():
        gaps.append(np.min(np.abs(np.imag(z[~real])) / np.maximum(1.0, np.abs(z[~real]))))
    g = min(gaps)
    return g if np.isfinite(g) else 1.0


def _candidates_poly(basis):
    B, ratio = eliminate(cubics(basis, NISTER))
    N = len(B)
    xyz, roots, sep = np.full((N, MAX_ROOTS, 3), np.nan), np.zeros(N, int), np.zeros(N)
    with np.errstate(all="ignore"):
        for n in range(N):
            if not np.isfinite(B[n]).all():
                continue
            rows = []
            for r in range(3):
                e, f = B[n, 4 + 2 * r], B[n, 5 + 2 * r]
                # ascending in z: <lead z> - z <lead>
                px = np.array([e[0], e[1] - f[0], e[2] - f[1], -f[2]])
                py = np.array([e[3], e[4] - f[3], e[5] - f[4], -f[5]])
                p1 = np.array([e[6], e[7] - f[6], e[8] - f[7], e[9] - f[8], -f[9]])
                rows.append((px, py, p1))
            P = np.polynomial.polynomial
            (a0, b0, c0), (a1, b1, c1), (a2, b2, c2) = rows
            det = P.polyadd(P.polysub(P.polymul(a0, P.polysub(P.polymul(b1, c2), P.polymul(b2, c1))),
                                      P.polymul(b0, P.polysub(P.polymul(a1, c2), P.polymul(a2, c1)))),
                            P.polymul(c0, P.polysub(P.polymul(a1, b2), P.polymul(a2, b1))))
            det = np.concatenate([det, np.zeros(11 - len(det))])
            z = np.roots(det[::-1])
            real = np.imag(z) == 0.0
            zr = np.sort(np.real(z[real]))
            roots[n], sep[n] = len(zr), _separation(z, real)
            for k, zk in enumerate(zr[:MAX_ROOTS]):
                v = np.array([[P.polyval(zk, q) for q in row] for row in rows])
                cr = [np.cross(v[0], v[1]), np.cross(v[0], v[2]), np.cross(v[1], v[2])]
                c = cr[int(np.argmax([np.dot(q, q) for q in cr]))]
                xyz[n, k] = c[0] / c[2], c[1] / c[2], zk
    return xyz, roots, ratio, sep


POLISH = 3


def polish(xyz, M, order):
    """(x, y, z) (N,K,3) polished on the ten cubics M (N,10,20) in the monomials of `order`: POLISH Gauss-Newton steps,
    (J^T J) delta = -J^T f; a step that is not finite is not taken"""
    ex = np.array(order)                                             # (20,3)
    xyz = xyz.copy()
    with np.errstate(all="ignore"):
        for _ in range(POLISH):
            v = xyz[:, :, None, :]                                   # (N,K,1,3)
            mono = np.prod(v ** ex, axis=-1)                         # (N,K,20)
            f = np.einsum("nrc,nkc->nkr", M, mono)
            J = np.zeros(f.shape + (3,))
            for a in range(3):
                low = ex.copy()
                low[:, a] = np.maximum(low[:, a] - 1, 0)
                J[..., a] = np.einsum("nrc,nkc->nkr", M, ex[:, a] * np.prod(v ** low, axis=-1))
            H, g = np.einsum("nkra,nkrb->nkab", J, J), np.einsum("nkra,nkr->nka", J, f)
            step = np.full(xyz.shape, np.nan)
            ok = np.isfinite(H).all(axis=(-1, -2)) & np.isfinite(g).all(axis=-1) & (np.abs(np.linalg.det(np.nan_to_num(H))) > 0.0)
            step[ok] = np.linalg.solve(H[ok], g[ok][..., None])[..., 0]
            xyz = np.where(np.isfinite(step).all(axis=-1, keepdims=True), xyz - step, xyz)
    return xyz


def poses_of(E, ya, yb):
    """E (M,3,3), the samples ya, yb (M,5,2) -> (pose (M,12): R row-major then t, NaN where void; valid (M,)).  E = U diag(s) V^T
    with U, V proper; R in {U W V^T, U W^T V^T}, t = +-u3, the first combination with all five samples at positive depth in both
    cameras; the depths (l_a, l_b) of l_a R d_a - l_b d_b = -t by its normal equations"""
    M = len(E)
    ok = np.isfinite(E).all(axis=(1, 2))
    with np.errstate(all="ignore"):
        U, S, Vt = np.linalg.svd(np.where(ok[:, None, None], E, 0.0))
        U[:, :, 2] *= np.sign(np.linalg.det(U))[:, None]
        Vt[:, 2, :] *= np.sign(np.linalg.det(Vt))[:, None]
        W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
        da = np.concatenate([ya, np.ones((M, SAMPLE, 1))], axis=-1)
        db = np.concatenate([yb, np.ones((M, SAMPLE, 1))], axis=-1)
        pose, valid = np.full((M, 12), np.nan), np.zeros(M, bool)
        for Wk in (W, W.T):
            R = U @ Wk @ Vt
            for sign in (1.0, -1.0):
                t = sign * U[:, :, 2]
                p = np.einsum("mrc,mic->mir", R, da)
                q = -db
                pp, pq, qq = np.sum(p * p, -1), np.sum(p * q, -1), np.sum(q * q, -1)
                bp, bq = -np.einsum("mir,mr->mi", p, t), -np.einsum("mir,mr->mi", q, t)
                det = pp * qq - pq * pq
                la, lb = (bp * qq - bq * pq) / det, (pp * bq - pq * bp) / det
                front = ((la > DEPTH_MIN) & (lb > DEPTH_MIN)).all(axis=1) & ok & (S[:, 1] > 0.0) & ~valid
                pose[front] = np.concatenate([R.reshape(M, 9), t], axis=1)[front]
                valid |= front
    valid &= np.isfinite(pose).all(axis=1)
    return np.where(valid[:, None], pose, np.nan), valid


def solve(ya, yb, method="action"):
    """the five-point solver on N samples (N,5,2) twice -> dict(poses (N,10,12) NaN where void, valid (N,10), roots (N,): the real
    candidates, sv (N,5), ratio, sep, pick (N,))"""
    basis, sv, pick = null_space(ya, yb, method)
    xyz, roots, ratio, sep = (_candidates_action if method == "action" else _candidates_poly)(basis)
    ratio = np.minimum(ratio, eliminate(cubics(basis, NISTER if method == "action" else GRADED))[1])      # of both eliminations
    N = len(ya)
    xyz = polish(xyz, cubics(basis, GRADED), GRADED)
    with np.errstate(all="ignore"):
        E = np.einsum("nkc,ncij->nkij", np.concatenate([xyz, np.ones((N, MAX_ROOTS, 1))], axis=-1), basis)
    rep = lambda y: np.repeat(y[:, None], MAX_ROOTS, axis=1).reshape(N * MAX_ROOTS, SAMPLE, 2)      # noqa: E731
    pose, valid = poses_of(E.reshape(N * MAX_ROOTS, 3, 3), rep(ya), rep(yb))
    with np.errstate(all="ignore"):
        far = np.nan_to_num(np.nanmax(np.abs(xyz).reshape(N, -1), axis=1), nan=0.0)
    return dict(poses=pose.reshape(N, MAX_ROOTS, 12), valid=valid.reshape(N, MAX_ROOTS), roots=roots, far=far, sv=sv, ratio=ratio, sep=sep, pick=pick, E=E)


# ------------------------------------------------------------------------------------------------------------ steps 4 and 5
def fundamental(poses, cam_a, cam_b):
    """poses (...,12), the records of the two views -> F (...,3,3) = K_b^-T [t]x R K_a^-1"""
    R, t = poses[..., :9].reshape(poses.shape[:-1] + (3, 3)), poses[..., 9:]
    tx = np.zeros(poses.shape[:-1] + (3, 3))
    tx[..., 0, 1], tx[..., 0, 2], tx[..., 1, 0], tx[..., 1, 2], tx[..., 2, 0], tx[..., 2, 1] = \
        -t[..., 2], t[..., 1], t[..., 2], -t[..., 0], -t[..., 1], t[..., 0]
    Kinv = lambda c: np.array([[1.0 / c[0], 0.0, -c[2] / c[0]], [0.0, 1.0 / c[1], -c[3] / c[1]], [0.0, 0.0, 1.0]])      # noqa: E731
    with np.errstate(all="ignore"):
        return Kinv(cam_b).T @ (tx @ R) @ Kinv(cam_a)


def sampson(F, ua, ub):
    """F (M,3,3), the undistorted pixels ua, ub (N,2) -> d (M,N), the signed Sampson distance in pixels"""
    ha = np.concatenate([ua, np.ones((len(ua), 1))], axis=1)
    hb = np.concatenate([ub, np.ones((len(ub), 1))], axis=1)
    with np.errstate(all="ignore"):
        Fa = np.einsum("mij,nj->mni", F, ha)
        Fb = np.einsum("mji,nj->mni", F, hb)
        num = np.einsum("mni,ni->mn", Fa, hb)
        return num / np.sqrt(Fa[..., 0] ** 2 + Fa[..., 1] ** 2 + Fb[..., 0] ** 2 + Fb[..., 1] ** 2)


def score(obs, cams, pairs, poses, threshold):
    """step 4 on poses (P,M,12) -> dict(count (P,M) ints, cost (P,M), inliers (B,P,M,J) bool, d2 (B,P,M,J)): a pose that is not
    finite scores (0, inf)"""
    cams = np.asarray(cams, dtype=np.float64)
    B, P, J = obs["part"].shape
    M = poses.shape[1]
    t2 = float(threshold) ** 2
    count, cost = np.zeros((P, M), int), np.full((P, M), np.inf)
    inl, d2 = np.zeros((B, P, M, J), bool), np.full((B, P, M, J), np.nan)
    for p, (a, b) in enumerate(pairs):
        void = ~np.isfinite(poses[p]).all(axis=-1)
        F = fundamental(np.where(void[:, None], 0.0, poses[p]), cams[a], cams[b])
        d = sampson(F, obs["ua"][:, p].reshape(B * J, 2), obs["ub"][:, p].reshape(B * J, 2))
        part, w = obs["part"][:, p].reshape(B * J), obs["w"][:, p].reshape(B * J)
        with np.errstate(all="ignore"):
            dd = d * d
            within = part[None] & (dd <= t2) & ~void[:, None]
            c = np.sum(np.where(part[None], w[None] * np.where(within, dd, t2), 0.0), axis=1)
        count[p], cost[p] = within.sum(axis=1), np.where(void, np.inf, c)
        inl[:, p], d2[:, p] = within.reshape(M, B, J).transpose(1, 0, 2), dd.reshape(M, B, J).transpose(1, 0, 2)
    return dict(count=count, cost=cost, inliers=inl, d2=d2)


def best_candidates(count, cost):
    """(P,H,10) twice -> k (P,H): the best candidate of every hypothesis -- most inliers, then the lowest cost, then the lowest
    number -- or -1 where all are void; and clear (P,H): it has more inliers than any other"""
    P, H, K = count.shape
    best, clear = np.full((P, H), -1), np.ones((P, H), bool)
    for p in range(P):
        for h in range(H):
            k = lc.winner(count[p, h], cost[p, h])
            best[p, h] = k
            if k >= 0:
                others = [count[p, h, i] for i in range(K) if i != k and np.isfinite(cost[p, h, i])]
                clear[p, h] = not others or max(others) < count[p, h, k]
    return best, clear


def hypothesise(pixels, conf, cams, dist, pairs, threshold=6.0, hypotheses=1024, seed=0, method="action"):
    """steps 1 to 4 -> dict(poses (P,H,12), scores (P,H,2), roots (P,H), valid, drawn, well (P,H), obs, candidates: the dict of
    solve() reshaped to (P,H,...), cand_score: the dict of score() on the candidates)"""
    cams = np.asarray(cams, dtype=np.float64)
    obs = observations(pixels, conf, cams, dist, pairs)
    B, P, J = obs["part"].shape
    H = hypotheses
    slots, drawn = samples(obs["part"], seed, H)
    drawn &= obs["usable"][:, None]
    ya = np.stack([obs["ya"][:, p].reshape(B * J, 2)[slots[p]] for p in range(P)])       # (P,H,5,2)
    yb = np.stack([obs["yb"][:, p].reshape(B * J, 2)[slots[p]] for p in range(P)])
    s = solve(ya.reshape(P * H, SAMPLE, 2), yb.reshape(P * H, SAMPLE, 2), method)
    s = {k: v.reshape((P, H) + v.shape[1:]) for k, v in s.items()}
    s["poses"] = np.where(drawn[:, :, None, None], s["poses"], np.nan)
    s["valid"] &= drawn[:, :, None]
    s["roots"] = np.where(drawn, s["roots"], 0)
    cs = score(obs, cams, pairs, s["poses"].reshape(P, H * MAX_ROOTS, 12), threshold)
    count, cost = cs["count"].reshape(P, H, MAX_ROOTS), cs["cost"].reshape(P, H, MAX_ROOTS)
    k, clear = best_candidates(count, cost)
    valid = k >= 0
    kk = np.maximum(k, 0)[..., None]
    poses = np.where(valid[..., None], np.take_along_axis(s["poses"], kk[..., None], axis=2)[:, :, 0], np.nan)
    scores = np.stack([np.where(valid, np.take_along_axis(count, kk, axis=2)[..., 0], 0).astype(np.float64),
                       np.where(valid, np.take_along_axis(cost, kk, axis=2)[..., 0], np.inf)], axis=-1)
    # where every valid candidate has all participants as inliers (a pair with exactly five: each fits them by construction), none
    # can be clear of another and which one is best is a matter of rounding: such a hypothesis is compared candidate by candidate
    n_part = obs["part"].sum(axis=(0, 2))[:, None, None]
    tied = drawn & valid & np.where(np.isfinite(cost), count == n_part, True).all(axis=2)
    clear = clear | tied
    with np.errstate(all="ignore"):
        well = drawn & (s["sv"][..., 4] >= WELL_SV * s["sv"][..., 0]) & (s["ratio"] >= WELL_PIVOT) & (s["sep"] >= WELL_ROOTS) & \
            (s["pick"] >= WELL_PICK) & clear
    return dict(poses=poses, scores=scores, roots=s["roots"], valid=valid, drawn=drawn, well=well, obs=obs, candidates=s,
                cand_score=cs, best_candidate=k, slots=slots, tied=tied)


def finish(obs, cams, pairs, poses, scores, threshold, baseline=1.0):
    """step 5: from the scores of all hypotheses to the outputs of the call -> dict(rotation (P,3,3), direction (P,3), cams (P,2,16),
    inliers (B,P,J) float32, count, best, error, status)"""
    cams = np.asarray(cams, dtype=np.float64)
    B, P, J = obs["part"].shape
    out = dict(rotation=np.full((P, 3, 3), np.nan), direction=np.full((P, 3), np.nan), cams=np.full((P, 2, 16), np.nan),
               inliers=np.zeros((B, P, J), np.float32), count=np.zeros(P, np.int32), best=np.full(P, -1, np.int32),
               error=np.full(P, np.nan), status=np.full(P, 3, np.uint8))
    for p, (a, b) in enumerate(pairs):
        out["cams"][p, 0, :4], out["cams"][p, 1, :4] = cams[a, :4], cams[b, :4]
        if not obs["usable"][p]:
            continue
        h = lc.winner(scores[p, :, 0], scores[p, :, 1])
        out["best"][p] = h
        if h < 0 or scores[p, h, 0] < MIN_INLIERS:
            continue
        s = score({k: v[:, p:p + 1] for k, v in obs.items() if k != "usable"}, cams, [pairs[p]], poses[p:p + 1, h:h + 1], threshold)
        inl, d2 = s["inliers"][:, 0, 0], s["d2"][:, 0, 0]
        R, t = poses[p, h, :9].reshape(3, 3), poses[p, h, 9:]
        out["rotation"][p], out["direction"][p], out["status"][p] = R, t, 0
        out["inliers"][:, p], out["count"][p] = inl, inl.sum()
        out["error"][p] = np.sqrt(d2[inl].sum() / inl.sum())
        out["cams"][p, 0, 4:] = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])
        out["cams"][p, 1, 4:13] = poses[p, h, :9]
        for k in range(3):                                           # every product and sum rounded on its own, in the device's order
            out["cams"][p, 1, 13 + k] = -(baseline * ((R[0, k] * t[0] + R[1, k] * t[1]) + R[2, k] * t[2]))
    return out


def relative_pose(pixels, conf, cams, dist=None, pairs=((0, 1),), threshold=6.0, hypotheses=1024, seed=0, baseline=1.0, method="action"):
    """relative_pose(return_hypotheses=True) without the polish -> the dict of finish() plus poses (P,H,12), scores (P,H,2), roots
    (P,H), hyp"""
    hyp = hypothesise(pixels, conf, cams, dist, pairs, threshold, hypotheses, seed, method)
    out = finish(hyp["obs"], cams, pairs, hyp["poses"], hyp["scores"], threshold, baseline)
    out.update(poses=hyp["poses"], scores=hyp["scores"], roots=hyp["roots"], hyp=hyp)
    return out


# --------------------------------------------------------------------------------------------------------------- the polish
LAMBDA0, LAMBDA_MIN, LAMBDA_MAX, MIN_REFINE = cc.LAMBDA0, cc.LAMBDA_MIN, cc.LAMBDA_MAX, 6


def tangent(t):
    """e1 = normalise(t x axis_k), k the coordinate of t of the smallest magnitude (the lowest among equals), e2 = t x e1"""
    k = int(np.argmin(np.abs(t)))
    e1 = np.cross(t, np.eye(3)[k])
    e1 = e1 / np.linalg.norm(e1)
    return e1, np.cross(t, e1)


def _cross(v, A):
    """[v]x A"""
    return np.cross(v, A, axisb=0, axisc=0)


def apply_step(pose, delta):
    """the trial pose R' = exp([w]x) R, t' = normalise(t + d1 e1 + d2 e2)"""
    R, t = pose[:9].reshape(3, 3), pose[9:]
    e1, e2 = tangent(t)
    with np.errstate(all="ignore"):
        t2 = t + delta[3] * e1 + delta[4] * e2
        return np.concatenate([(cc.rodrigues(delta[:3]) @ R).reshape(9), t2 / np.linalg.norm(t2)])


def refine_evaluate(ya, yb, w, cam_a, cam_b, pose, huber=None):
    """the sums of one evaluation over the participating correspondences (w > 0) of a pair -> dict(E, S, W, H (5,5), g (5,), d)"""
    R, t = pose[:9].reshape(3, 3), pose[9:]
    e1, e2 = tangent(t)
    M = [_cross(t, R)] + [_cross(t, _cross(np.eye(3)[k], R)) for k in range(3)] + [_cross(e1, R), _cross(e2, R)]
    on = w > 0.0
    a = np.concatenate([ya[on], np.ones((on.sum(), 1))], axis=1)
    b = np.concatenate([yb[on], np.ones((on.sum(), 1))], axis=1)
    k = np.array([1.0 / cam_b[0], 1.0 / cam_b[1], 1.0 / cam_a[0], 1.0 / cam_a[1]])

    def forms(Mk):
        Ma, Mb = a @ Mk.T, b @ Mk
        return np.sum(b * Ma, axis=1), np.stack([Ma[:, 0] * k[0], Ma[:, 1] * k[1], Mb[:, 0] * k[2], Mb[:, 1] * k[3]], axis=1)
    with np.errstate(all="ignore"):
        n, g = forms(M[0])
        s = np.sqrt(np.sum(g * g, axis=1))
        d = n / s
        J = np.stack([nk / s - n * np.sum(g * gk, axis=1) / s ** 3 for nk, gk in (forms(Mk) for Mk in M[1:])], axis=1)
        ww, dd = w[on], d * d
        tail = (dd > huber * huber) if huber else np.zeros(len(d), bool)
        h = huber if huber else 0.0
        E = np.sum(ww * np.where(tail, 2.0 * h * np.abs(d) - h * h, dd))
        wi = np.where(tail, ww * h / np.abs(d), ww)
        return dict(E=E, S=np.sum(ww * dd), W=np.sum(ww), H=np.einsum("n,ni,nj->ij", wi, J, J), g=np.einsum("n,ni,n->i", wi, J, d), d=d, J=J)


def _lm_step(H, g, lam):
    """(H + lambda diag H) delta = -g by the unpivoted Cholesky factorisation; NaN where a pivot is <= 0 or not finite"""
    A = H + lam * np.diag(np.diag(H))
    with np.errstate(all="ignore"):
        L = np.zeros((5, 5))
        for j in range(5):
            dj = A[j, j] - np.sum(L[j, :j] ** 2)
            if not (dj > 0.0 and np.isfinite(dj)):
                return np.full(5, np.nan)
            L[j, j] = np.sqrt(dj)
            for i in range(j + 1, 5):
                L[i, j] = (A[j, i] - np.sum(L[i, :j] * L[j, :j])) / L[j, j]
        y = np.linalg.solve(L, -g)
        return np.linalg.solve(L.T, y)


def refine(pixels, conf, cams, pairs, rotation, direction, dist=None, huber=None, max_iterations=20, step_tolerance=1e-8, weight=None):
    """refine_relative_pose -> dict(rotation (P,3,3), direction (P,3), error, cost0, cost (P,), used, iterations, status (P,) ints)"""
    cams = np.asarray(cams, dtype=np.float64)
    obs = observations(pixels, conf, cams, dist, pairs)
    B, P, J = obs["part"].shape
    out = dict(rotation=np.array(rotation, dtype=np.float64), direction=np.array(direction, dtype=np.float64), error=np.full(P, np.nan),
               cost0=np.full(P, np.nan), cost=np.full(P, np.nan), used=np.zeros(P, int), iterations=np.zeros(P, int), status=np.full(P, 3))
    for p, (va, vb) in enumerate(pairs):
        w = obs["w"][:, p].reshape(B * J)
        if weight is not None:
            wp = np.asarray(weight, dtype=np.float64)[:, p].reshape(B * J)
            with np.errstate(all="ignore"):
                w = np.where(np.isfinite(wp) & (wp > 0.0), w * wp, 0.0)
        ya, yb = obs["ya"][:, p].reshape(B * J, 2), obs["yb"][:, p].reshape(B * J, 2)
        pose = np.concatenate([out["rotation"][p].reshape(9), out["direction"][p]])
        out["used"][p] = int((w > 0.0).sum())
        ev = lambda q: refine_evaluate(ya, yb, w, cams[va], cams[vb], q, huber)      # noqa: E731
        if out["used"][p] == 0 or not np.isfinite(pose).all() or not np.isfinite(cams[[va, vb], :4]).all():
            continue
        cur = ev(pose)
        if not np.isfinite(cur["E"]):
            continue
        E0, lam, status, trials = cur["E"], LAMBDA0, 2, 0
        if max_iterations > 0 and out["used"][p] >= MIN_REFINE:
            status = 1
            while True:
                delta = _lm_step(cur["H"], cur["g"], lam)
                trial = apply_step(pose, delta)
                tr = ev(trial)
                trials += 1
                if tr["E"] < cur["E"]:
                    pose, cur, lam = trial, tr, max(lam / 10.0, LAMBDA_MIN)
                else:
                    lam *= 10.0
                if np.abs(delta).max() <= step_tolerance:
                    status = 0
                    break
                if lam > LAMBDA_MAX or trials >= max_iterations:
                    break
        out["rotation"][p], out["direction"][p] = pose[:9].reshape(3, 3), pose[9:]
        out["error"][p], out["cost0"][p], out["cost"][p] = np.sqrt(cur["S"] / cur["W"]), E0, cur["E"]
        out["iterations"][p], out["status"][p] = trials, status
    return out


# -------------------------------------------------------------------------------------------------------------------- cases
def true_pose(truth_cams, pair):
    """the records of the two views -> (R (3,3), t (3,) of unit length, baseline): x_b = R x_a + baseline t"""
    a, b = np.asarray(truth_cams)[pair[0]], np.asarray(truth_cams)[pair[1]]
    Ra, Rb = a[4:13].reshape(3, 3), b[4:13].reshape(3, 3)
    R = Rb @ Ra.T
    t = Rb @ (a[13:] - b[13:])
    return R, t / np.linalg.norm(t), float(np.linalg.norm(t))


def pose_errors(rotation, direction, truth_cams, pair):
    """-> (degrees between the two rotations, degrees between the two directions)"""
    R, t, _ = true_pose(truth_cams, pair)
    cos = (np.trace(np.asarray(rotation) @ R.T) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(cos, -1.0, 1.0)))), float(np.degrees(np.arccos(np.clip(np.dot(direction, t), -1.0, 1.0))))


def pose_gap(a, b):
    """the largest entry of the difference of two poses (...,12)"""
    return np.abs(np.asarray(a) - np.asarray(b)).max(axis=-1)


def case(B, V, J, pairs=((0, 1),), name="h36m", noise=2.0, conf="none", outliers=0.0, lens=True, exact=False, **kw):
    """locate_cameras_cases.case as a two-view problem: dict(pixels, conf, cams (intrinsics, blank poses), truth_cams, dist, planted,
    pairs, and kw -- hypotheses, seed, threshold -- as the arguments of the call).  exact: the pixels are the float64 projections
    of the points, nothing rounded"""
    c = lc.case(B, V, J, name=name, noise=noise, conf=conf, outliers=outliers, lens=lens)
    px = c["pixels"]
    if exact:
        px = dc.project(c["points"].astype(np.float64), c["truth_cams"], _table(c["cams"], c["dist"]))[0]
    out = dict(pixels=px, conf=c["conf"], cams=c["cams"], truth_cams=c["truth_cams"], dist=c["dist"], planted=c["planted"],
               pairs=tuple(tuple(p) for p in pairs), threshold=6.0, hypotheses=64, seed=0)
    out.update(kw)
    return out


def call_args(c):
    return dict(pairs=c["pairs"], threshold=c["threshold"], hypotheses=c["hypotheses"], seed=c["seed"])


def run(c, **kw):
    args = call_args(c)
    args.update(kw)
    return relative_pose(c["pixels"], c["conf"], c["cams"], c["dist"], **args)


def outlier_case(**kw):
    """the case of the issue: (8,4,17), the H36M-like lens, 2 px of noise, a quarter of every view's detections planted 40 .. 120 px
    off, 256 hypotheses, pairs (0,1) and (2,3)"""
    return case(8, 4, 17, pairs=((0, 1), (2, 3)), outliers=0.25, hypotheses=256, **kw)


TILE = 64              # RPOSE_TILE of the kernel: slots staged at a time


def few_case(n, noise=0.0, **kw):
    """exactly n participants of a (1,2,17) pinhole scene (float32 pixels): the others have confidence 0"""
    c = case(1, 2, 17, noise=noise, lens=False, hypotheses=16, **kw)
    conf = np.zeros((1, 2, 17), np.float32)
    conf[:, :, :n] = 1.0
    c["conf"] = conf
    return c


def gpu_cases():
    """name -> case: the shapes of the GPU tests, the smallest at which the kernel can go wrong"""
    v32 = tuple((0, v) for v in range(1, 17)) + tuple((v, 0) for v in range(17, 32)) + ((1, 0),)
    cases = {
        # exactly five participants: the one sample fits itself, there is no sixth inlier.  Six: located.  With the 2 px of noise of
        # the other cases: without noise the cost of the true pose is 5e-13 px^2 of float32 pixel rounding, a cancellation which no
        # two fp64 evaluations share to 1e-10
        "five": few_case(5, noise=2.0),
        "six": few_case(6, noise=2.0),
        "outliers": outlier_case(),
        "n63_pinhole_mixed": case(9, 2, 7, conf="mixed", lens=False),               # one below the tile; conf with zeros, NaN, negatives
        "n64_j64": case(1, 2, 64),                                                  # the tile, and the widest pose
        "n65": case(5, 2, 13),                                                      # one above
        "v32": case(2, 32, 17, pairs=v32, name="per_view", hypotheses=16),          # every pair slot, fx != fy, per-view intrinsics
        "nan_pixels_one_view": case(4, 3, 17, pairs=((0, 1), (1, 2), (2, 0)), hypotheses=65),
    }
    px = cases["nan_pixels_one_view"]["pixels"].copy()
    px[::2, 1, ::3] = np.nan
    cases["nan_pixels_one_view"]["pixels"] = px
    assert len(v32) == 32
    assert [int(np.prod(np.asarray(cases[k]["pixels"]).shape[:3:2])) for k in ("n63_pinhole_mixed", "n64_j64", "n65")] == [TILE - 1, TILE, TILE + 1]
    for H in (1, 63, 64, 65, 256):
        cases["small_h%d" % H] = case(2, 2, 17, hypotheses=H)
    return cases


def umeyama(X, Y):
    """the similarity (s, R, t) that takes the points X (N,3) closest to Y: Y ~ s R X + t"""
    mx, my = X.mean(axis=0), Y.mean(axis=0)
    Xc, Yc = X - mx, Y - my
    U, S, Vt = np.linalg.svd(Yc.T @ Xc / len(X))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
    R = U @ D @ Vt
    s = np.trace(np.diag(S) @ D) / np.mean(np.sum(Xc * Xc, axis=1))
    return s, R, my - s * R @ mx


def aligned_mean_error(points, truth):
    """the mean distance of the points to the truth after one global similarity, over the finite points"""
    X, Y = np.asarray(points, dtype=np.float64).reshape(-1, 3), np.asarray(truth, dtype=np.float64).reshape(-1, 3)
    ok = np.isfinite(X).all(axis=1)
    s, R, t = umeyama(X[ok], Y[ok])
    return float(np.mean(np.linalg.norm(s * X[ok] @ R.T + t - Y[ok], axis=1)))
