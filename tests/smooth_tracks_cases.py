"""Temporal smoothing of pose tracks (mpl_smooth_tracks, include/mpl_hip.h) restated in float64 numpy, and the cases of its tests.

The restatement (`smooth`) follows the header to the letter: per (segment, joint) track a dense D from its definition, one
np.linalg.solve of (W' + smoothness D^T D) X = W' Y per reweighting, the IRLS loop, the stopping rule and the statuses.  A second
formulation (`solver="banded"`: the pentadiagonal L D L^T written out in numpy, sequential over the frames) exists to measure how
far two float64 formulations of the same problem lie apart (`formulation_distance`), and carries the two lengths at which a dense
matrix is out of reach (4096 and 65536 frames).

Cases are cached and read-only."""
import functools

import numpy as np

from openmpl_amd import cabi

FINITE_MAX = np.finfo(np.float64).max
CONVERGED, CAPPED, PASSED_THROUGH = 0, 1, 2
DENSE_MAX = 1100                       # longer tracks go to the banded formulation

# the lengths of the issue, and one below, at and one above every threshold of the implementation (read from the binding)
BASE_LENGTHS = tuple(range(1, 13)) + (31, 32, 33, 63, 64, 65, 127, 128, 129, 130, 191, 192, 193, 255, 256, 257, 511, 512, 513, 1000)
THRESHOLDS = cabi.smooth_thresholds()
LENGTHS = tuple(sorted(set(BASE_LENGTHS + tuple(t + d for t in THRESHOLDS for d in (-1, 0, 1)))))
SMOOTHNESS = (1e-2, 1.0, 1e4)
HUBER = 0.05
SEGMENT_LISTS = {"mixed": (1, 5, 64, 2, 129), "forty": (3,) * 40}


def chunking(T):
    """(block length, blocks) of the device for a segment of T frames (mpl_hip.h): what the gap-on-a-chunk case aims at"""
    if T <= cabi.SMOOTH_SINGLE_MAX:
        return T, 1
    L = max(cabi.SMOOTH_CHUNK_MIN, -(-T // cabi.SMOOTH_LANES))
    return L, -(-T // L)


# ------------------------------------------------------------------------------------------------------------------ the restatement
def takes_part(Y, w):
    """(T,) bool for one track: Y (T,3), w (T,) or None"""
    ok = np.isfinite(Y).all(axis=1)
    if w is not None:
        with np.errstate(invalid="ignore"):
            ok &= (w > 0) & (w <= FINITE_MAX)
    return ok


def difference(T, order):
    """D^order of a segment of T frames, dense ((T - order, T); no row when T <= order)"""
    D = np.zeros((max(T - order, 0), T))
    for r in range(D.shape[0]):
        D[r, r:r + order + 1] = (-1.0, 1.0) if order == 1 else (1.0, -2.0, 1.0)
    return D


def rho(s, h):
    if not h:
        return s
    return np.where(s <= h * h, s, 2.0 * h * np.sqrt(s) - h * h)


def cost_track(X, Y, w, part, lam, order, h):
    """E(X) of one track, float64; Y and w anything at gaps"""
    r2 = ((X - np.where(part[:, None], Y, 0.0)) ** 2).sum(axis=1)
    data = float((np.where(part, w, 0.0) * rho(r2, h))[part].sum())
    DX = difference(len(X), order) @ X if len(X) <= DENSE_MAX else (np.diff(X, n=order, axis=0))
    return data + lam * float((DX ** 2).sum())


def _banded_solve(wq, B, lam, order):
    """(diag(wq) + lam D^T D) X = B by the pentadiagonal L D L^T, frame after frame"""
    T = len(wq)
    t = np.arange(T)
    if order == 2:
        r0 = ((t >= 1) & (t <= T - 2)).astype(float); rm = ((t >= 2) & (t <= T - 1)).astype(float); rp = (t <= T - 3).astype(float)
        a, e, f = wq + lam * (4 * r0 + rm + rp), lam * -2.0 * (r0 + rp), lam * rp
    else:
        r0 = (t <= T - 2).astype(float); rm = (t >= 1).astype(float)
        a, e, f = wq + lam * (r0 + rm), lam * -r0, np.zeros(T)
    d, l1, l2 = np.zeros(T), np.zeros(T), np.zeros(T)
    y = np.array(B, dtype=np.float64)
    for i in range(T):
        di = a[i]
        if i >= 1:
            di -= l1[i - 1] ** 2 * d[i - 1]
            y[i] -= l1[i - 1] * y[i - 1]
        if i >= 2:
            di -= l2[i - 2] ** 2 * d[i - 2]
            y[i] -= l2[i - 2] * y[i - 2]
        d[i] = di
        if i + 1 < T:
            l1[i] = (e[i] - (l2[i - 1] * d[i - 1] * l1[i - 1] if i >= 1 else 0.0)) / di
        if i + 2 < T:
            l2[i] = f[i] / di
    x = y / d[:, None]
    for i in range(T - 1, -1, -1):
        if i + 1 < T:
            x[i] -= l1[i] * x[i + 1]
        if i + 2 < T:
            x[i] -= l2[i] * x[i + 2]
    return x


def _solve(wq, Yz, lam, order, solver):
    if solver == "banded":
        return _banded_solve(wq, wq[:, None] * Yz, lam, order)
    D = difference(len(wq), order)
    return np.linalg.solve(np.diag(wq) + lam * (D.T @ D), wq[:, None] * Yz)


def _prepared(Y, w, order, huber):
    Y = np.asarray(Y, dtype=np.float64)
    w = np.ones(len(Y)) if w is None else np.asarray(w, dtype=np.float64)
    part = takes_part(Y, w)
    h = float(huber) if (huber is not None and huber > 0 and np.isfinite(huber)) else 0.0
    Yz, wz = np.where(part[:, None], Y, 0.0), np.where(part, w, 0.0)
    extent = float((Yz[part].max(axis=0) - Yz[part].min(axis=0)).max()) if part.any() else 0.0
    return Y, part, h, Yz, wz, extent


def _reweighted(X, Yz, wz, h):
    r = np.sqrt(((X - Yz) ** 2).sum(axis=1))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(r > h, wz * (h / r), wz)


def smooth_track(Y, w, lam, order=2, huber=None, max_iterations=20, step_tolerance=1e-6, solver=None, trace=None):
    """one track: Y (T,3) float32 / float64, w (T,) or None -> dict(points float64 (T,3), residual, irls_weight (T,), cost0, cost,
    iterations, status).  trace: a list that receives E of every iterate that was taken"""
    Y, part, h, Yz, wz, extent = _prepared(Y, w, order, huber)
    solver = solver or ("dense" if len(Y) <= DENSE_MAX else "banded")
    if part.sum() < order or max_iterations == 0:
        return dict(points=Y.copy(), residual=np.where(part, 0.0, np.nan), irls_weight=part.astype(np.float64), cost0=0.0, cost=0.0,
                    iterations=0, status=PASSED_THROUGH, passed=True)
    X = _solve(wz, Yz, lam, order, solver)
    it, status = 1, CONVERGED
    cost = cost0 = cost_track(X, Yz, wz, part, lam, order, h)
    if trace is not None:
        trace.append(cost)
    if h > 0 and extent > 0:
        while True:
            if it >= max_iterations:
                status = CAPPED
                break
            Xn = _solve(_reweighted(X, Yz, wz, h), Yz, lam, order, solver)
            it += 1
            En = cost_track(Xn, Yz, wz, part, lam, order, h)
            if not En < cost:
                break
            step = float(np.abs(Xn - X).max())
            X, cost = Xn, En
            if trace is not None:
                trace.append(cost)
            if step <= step_tolerance * extent:
                break
    r = np.sqrt(((X - Yz) ** 2).sum(axis=1))
    with np.errstate(divide="ignore", invalid="ignore"):
        irls = np.where(part, np.where((h > 0) & (r > h), h / r, 1.0), 0.0)
    return dict(points=X, residual=np.where(part, r, np.nan), irls_weight=irls, cost0=cost0, cost=cost, iterations=it, status=status,
                passed=False)


def next_step(X, Y, w, lam, order, huber, solver=None):
    """one reweighted solve from the iterate X (float64 (T,3)) of one track -> (E(X), E(next), largest coordinate step, extent):
    what the stopping rule of the header looks at"""
    Y, part, h, Yz, wz, extent = _prepared(Y, w, order, huber)
    solver = solver or ("dense" if len(Y) <= DENSE_MAX else "banded")
    X = np.asarray(X, dtype=np.float64)
    Xn = _solve(_reweighted(X, Yz, wz, h), Yz, lam, order, solver)
    return cost_track(X, Yz, wz, part, lam, order, h), cost_track(Xn, Yz, wz, part, lam, order, h), float(np.abs(Xn - X).max()), extent


def smooth(points, weight=None, segments=None, *, smoothness, order=2, huber=None, max_iterations=20, step_tolerance=1e-6, solver=None):
    """the call restated: points (T,J,3), weight (T,J) or None -> dict of arrays shaped like the outputs of smooth_tracks; points are
    float64 (`points64` of the device), with the given float32 values where a track passed through"""
    T, J = points.shape[:2]
    segments = (T,) if segments is None else tuple(segments)
    assert sum(segments) == T and min(segments) >= 1
    S = len(segments)
    out = dict(points=np.zeros((T, J, 3)), residual=np.zeros((T, J)), irls_weight=np.zeros((T, J)), cost0=np.zeros((S, J)), cost=np.zeros((S, J)),
               iterations=np.zeros((S, J), np.int32), status=np.zeros((S, J), np.uint8), passed=np.zeros((T, J), bool))
    t0 = 0
    for s, n in enumerate(segments):
        for j in range(J):
            r = smooth_track(points[t0:t0 + n, j], None if weight is None else weight[t0:t0 + n, j], smoothness, order, huber, max_iterations,
                             step_tolerance, solver)
            for k in ("points", "residual", "irls_weight", "passed"):
                out[k][t0:t0 + n, j] = r[k]
            for k in ("cost0", "cost", "iterations", "status"):
                out[k][s, j] = r[k]
        t0 += n
    return out


def cost(X, points, weight, segments, *, smoothness, order=2, huber=None):
    """(S,J): E of the header at the points X (T,J,3) float64, 0 for a track that passes through whatever max_iterations"""
    T, J = points.shape[:2]
    segments = (T,) if segments is None else tuple(segments)
    h = float(huber) if (huber is not None and huber > 0 and np.isfinite(huber)) else 0.0
    out = np.zeros((len(segments), J))
    t0 = 0
    for s, n in enumerate(segments):
        for j in range(J):
            Y = np.asarray(points[t0:t0 + n, j], np.float64)
            w = np.ones(n) if weight is None else np.asarray(weight[t0:t0 + n, j], np.float64)
            part = takes_part(Y, w)
            if part.sum() >= order:
                out[s, j] = cost_track(np.asarray(X[t0:t0 + n, j], np.float64), Y, np.where(part, w, 0.0), part, smoothness, order, h)
        t0 += n
    return out


def gradient(X, Y, w, lam, order, h):
    """dE/dX of one track at X, float64 (T,3)"""
    part = takes_part(Y, w)
    Yz, wz = np.where(part[:, None], np.asarray(Y, np.float64), 0.0), np.where(part, w, 0.0)
    r = X - Yz
    n = np.sqrt((r ** 2).sum(axis=1))
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where((h > 0) & (n > h), h / n, 1.0) if h else np.ones(len(X))
    D = difference(len(X), order)
    return 2.0 * (wz * k)[:, None] * r + 2.0 * lam * (D.T @ (D @ X))


def max_scaled(a, b):
    """max |a - b| / max |b| over the finite entries of b"""
    ok = np.isfinite(b)
    m = np.abs(b[ok]).max(initial=0.0)
    return float(np.abs(a[ok] - b[ok]).max(initial=0.0) / m) if m > 0 else float(np.abs(a[ok] - b[ok]).max(initial=0.0))


def formulation_distance(c, **kw):
    """the max-scaled distance of the banded from the dense formulation on a case, both float64; nan beyond the dense reach"""
    if max(c["segments"]) > DENSE_MAX:
        return float("nan")
    a = smooth(c["points"], c["weight"], c["segments"], solver="dense", **kw)
    b = smooth(c["points"], c["weight"], c["segments"], solver="banded", **kw)
    return max_scaled(b["points"], a["points"])


# ------------------------------------------------------------------------------------------------------------------------ the cases
def sinusoids(T, J, seed=0, noise=0.01):
    """(T,J,3) float64 tracks one unit across: sums of three sinusoids with periods of 40 to 400 frames; and the same with noise"""
    rs = np.random.RandomState(100 + seed)
    t = np.arange(T)[:, None, None]
    X = np.zeros((T, J, 3))
    for _ in range(3):
        X += rs.uniform(0.5, 1.0, (1, J, 3)) * np.sin(2 * np.pi * t / rs.uniform(40.0, 400.0, (1, J, 3)) + rs.uniform(0, 2 * np.pi, (1, J, 3)))
    span = np.maximum(X.max(axis=0) - X.min(axis=0), 1e-12) if T > 1 else np.ones((J, 3))
    X = X / span + rs.uniform(-1.0, 1.0, (1, J, 3))
    return X, X + noise * rs.standard_normal(X.shape)


def gap_mask(T, kind, seed=0):
    """(T,) bool, True where a frame is taken out"""
    g = np.zeros(T, bool)
    L, P = chunking(T)
    if kind == "none":
        pass
    elif kind.startswith("ends"):
        n = int(kind[4:])
        g[:n] = True
        g[max(T - n, 0):] = True
    elif kind == "chunk":                      # exactly one block of the split and the separators on both its sides
        b = min(1, P - 1)
        g[max(b * L - 2, 0):min((b + 1) * L, T)] = True
    elif kind == "middle40":
        g[max(T // 2 - 20, 0):T // 2 + 20] = True
    elif kind == "every_second":
        g[1::2] = True
    elif kind == "all_but_one":
        g[:] = True
        g[T // 3] = False
    elif kind == "all_but_two":
        g[:] = True
        g[T // 3] = False
        g[min(T // 3 + max(T // 2, 1), T - 1)] = False
    elif kind == "all":
        g[:] = True
    elif kind == "random10":
        g[np.random.RandomState(7 + seed).rand(T) < 0.1] = True
    else:
        raise KeyError(kind)
    return g


GAPS = ("ends1", "ends2", "ends9", "chunk", "middle40", "every_second", "all_but_one", "all_but_two", "all")


def _freeze(c):
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def case(T, J=3, segments=None, weights="none", gaps="none", nan_points=False, outliers=False, seed=0, gap_by="weight"):
    """float32 points (T,J,3) and weight (T,J) or None of a call.  weights: none / random / mixed (zeros, negatives, NaN, inf
    among positive ones); gaps: a kind of gap_mask, laid over every track of every segment, as a zero weight (gap_by="weight") or a
    NaN point ("point"); nan_points: NaN coordinates mixed in; outliers: 5 % of the frames displaced by 0.3 .. 1.0 units"""
    segments = (T,) if segments is None else tuple(segments)
    assert sum(segments) == T
    rs = np.random.RandomState(1000 + seed + 7 * T + J)
    truth, Y = sinusoids(T, J, seed)
    Y = Y.copy()
    if outliers:
        hit = rs.rand(T, J) < 0.05
        d = rs.standard_normal((T, J, 3))
        d *= (rs.uniform(0.3, 1.0, (T, J)) / np.linalg.norm(d, axis=-1))[..., None]
        Y[hit] += d[hit]
    w = None
    if weights == "random":
        w = rs.uniform(0.2, 3.0, (T, J))
    elif weights == "mixed":
        w = rs.uniform(0.2, 3.0, (T, J))
        k = rs.randint(0, 12, (T, J))
        w[k == 0] = 0.0
        w[k == 1] = -1.5
        w[k == 2] = np.nan
        w[k == 3] = np.inf
    if gaps != "none":
        g = np.concatenate([gap_mask(n, gaps, seed) for n in segments])
        if gap_by == "weight":
            w = np.ones((T, J)) if w is None else w
            w[g] = 0.0
        else:
            Y[g, :, rs.randint(0, 3)] = np.nan
    if nan_points:
        k = rs.rand(T, J) < 0.1
        Y[k, rs.randint(0, 3, int(k.sum()))] = np.nan
    return _freeze(dict(points=Y.astype(np.float32), weight=None if w is None else w.astype(np.float32), segments=segments, truth=truth, T=T, J=J))


def grid():
    """-> [(name, case kwargs, call kwargs)]: every length of LENGTHS under both orders and both costs with the smoothness, the
    joints and the weights taking turns; the segment lists; the gap kinds at a split length, under both ways of making a gap; the
    outliers"""
    out = []
    for i, T in enumerate(LENGTHS):
        for order in (1, 2):
            for huber in (None, HUBER):
                k = i + order + (huber is not None)
                J = (1, 3, 17)[k % 3] if T <= 130 else (1, 3)[k % 2]
                weights = ("none", "random", "mixed")[(k // 3) % 3]
                out.append(("T%d_o%d_%s" % (T, order, "huber" if huber else "plain"),
                            dict(T=T, J=J, weights=weights, nan_points=(k % 4 == 0), outliers=huber is not None, seed=k % 5),
                            dict(smoothness=SMOOTHNESS[k % 3], order=order, huber=huber)))
    for name, seg in SEGMENT_LISTS.items():
        for order in (1, 2):
            for huber in (None, HUBER):
                out.append(("seg_%s_o%d_%s" % (name, order, "huber" if huber else "plain"),
                            dict(T=sum(seg), J=3, segments=seg, weights="mixed", nan_points=True, outliers=huber is not None),
                            dict(smoothness=1.0, order=order, huber=huber)))
    for T in (130, 257):
        for g, gaps in enumerate(GAPS):
            for order in (1, 2):
                out.append(("gap_%s_T%d_o%d" % (gaps, T, order), dict(T=T, J=1 if T > 130 else 3, gaps=gaps, gap_by=("weight", "point")[(g + order) % 2],
                                                                      outliers=bool(g % 2)),
                            dict(smoothness=SMOOTHNESS[(g + order) % 3], order=order, huber=HUBER if g % 2 else None)))
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """(case, call kwargs, restatement) of a grid entry"""
    ckw, kw = {n: (c, k) for n, c, k in grid()}[name]
    c = case(**ckw)
    ref = smooth(c["points"], c["weight"], c["segments"], **kw)
    return c, kw, _freeze(ref)


@functools.lru_cache(maxsize=None)
def accuracy_case(T=512, J=17, seed=3):
    """the accuracy condition of the issue: sinusoid tracks one unit across with noise 0.01, 5 % outlier frames, 10 % gaps"""
    c = case(T, J, outliers=True, gaps="random10", seed=seed)
    return c


ACCURACY_SMOOTHNESS = 30.0             # chosen once from the restatement: order 2, Huber at HUBER
