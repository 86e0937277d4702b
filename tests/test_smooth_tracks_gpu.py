"""Temporal smoothing on the device (csrc/smooth_tracks.hip, openmpl_amd.geometry.smooth_tracks) against the float64 restatement of
tests/smooth_tracks_cases.py.

Parity is the rule of DESIGN.md section 2 (geometry_cases.rel_errors): max|d| <= 1e-4 max|ref| and norm-wise 1e-4 on points, residual
and irls_weight, NaN in the same places; the status equal; the solve count equal, or -- a Huber track whose stopping test sits within
rounding -- the restatement's next step from the device's own float64 iterate confirms the stop.  cost0 and cost lie within 1e-10
relative of the restatement's E at the device's own float64 points (the bound of refine_cameras: the same sum from the same numbers in
another order).  Beside it the measured parity: the max-scaled distance of the device's float64 points from the restatement's is at
most 100 times the distance of the two float64 formulations of the restatement on the same case (the margin and the reasoning of
locate_cameras: the device is a third formulation of the same float64 problem), the distance floored at one float64 epsilon.
Measured on an MI355X over the grid: see DESIGN.md section 7 and profiles/smooth_tracks.txt."""
import numpy as np
import pytest
import torch

from tests import geometry_cases as gc
from tests import smooth_tracks_cases as sc

pytestmark = pytest.mark.gpu

TOL = 1e-4
COST_TOL = 1e-10
FORMULATION_MARGIN = 100.0
EPS = float(np.finfo(np.float64).eps)


@pytest.fixture(autouse=True)
def _device_error_is_clear():
    yield
    from openmpl_amd import cabi
    torch.cuda.synchronize()
    assert not cabi.device_error()


def _dev(x):
    return None if x is None else torch.from_numpy(np.array(x)).cuda()


def _run(c, points=None, weight="case", segments="case", **kw):
    from openmpl_amd import smooth_tracks
    P = _dev(c["points"] if points is None else points)
    W = _dev(c["weight"] if isinstance(weight, str) else weight)
    seg = c["segments"] if isinstance(segments, str) else segments
    r = smooth_tracks(P, W, segments=seg, return_float64=True, **kw)
    S = len(seg) if seg is not None else 1
    T, J = P.shape[:2]
    assert r.points.shape == (T, J, 3) and r.points.dtype == torch.float32 and r.points64.dtype == torch.float64
    assert r.residual.shape == (T, J) and r.irls_weight.shape == (T, J) and r.residual.dtype == r.irls_weight.dtype == torch.float32
    assert r.cost0.shape == (S, J) and r.cost.shape == (S, J) and r.cost0.dtype == r.cost.dtype == torch.float64
    assert r.iterations.dtype == torch.int32 and r.status.dtype == torch.uint8 and r.status.shape == (S, J)
    return {k: getattr(r, k).cpu().numpy() for k in r._fields}


def _tracks(segments, J):
    t0 = 0
    for s, n in enumerate(segments):
        for j in range(J):
            yield s, j, slice(t0, t0 + n)
        t0 += n


def _residual_errors(got, ref, given):
    """rel_errors with a floor under both scales.  The residual is the difference X - Y of numbers of the size of Y, and Y is given
    in float32: a residual below one float32 epsilon of max|Y| is beneath the resolution of the data -- on a track that
    interpolates its frames exactly (one or two frames taking part) it is the rounding error of X - Y on both sides, 1e-15 against
    1e-14, and a relative comparison of the two says nothing.  There the scale is eps32 max|Y| (and that times sqrt(n) norm-wise)"""
    m, nrm = gc.rel_errors(got, ref)
    ok = np.isfinite(ref)
    if not ok.any():
        return m, nrm
    floor = float(np.finfo(np.float32).eps) * float(np.abs(given[np.isfinite(given)]).max(initial=0.0))
    d = got[ok].astype(np.float64) - ref[ok]
    top, norm = float(np.abs(ref[ok]).max()), float(np.linalg.norm(ref[ok]))
    return float(np.abs(d).max() / max(top, floor)) if max(top, floor) > 0 else m, \
        float(np.linalg.norm(d) / max(norm, floor * np.sqrt(d.size))) if max(norm, floor) > 0 else nrm


def _assert_costs(E_dev, X, c, kw, what):
    """a cost of the device within COST_TOL relative of the restatement's E at the same float64 points.  E is the squared norm of the
    vector of sqrt(w) r and sqrt(smoothness) D X; each entry is formed from coordinates of size max|X| with an error of a few
    float64 epsilons of that size (the device contracts multiply-adds), so the two norms differ by at most the norm of those errors
    whatever E is -- which is what is left to compare on a track that interpolates exactly and whose E is rounding error alone"""
    E = sc.cost(X, c["points"], c["weight"], c["segments"], **{k: kw[k] for k in ("smoothness", "order", "huber")})
    worst = 0.0
    for s, j, sl in _tracks(c["segments"], c["points"].shape[1]):
        w = np.ones(sl.stop - sl.start) if c["weight"] is None else c["weight"][sl, j].astype(np.float64)
        part = sc.takes_part(c["points"][sl, j].astype(np.float64), w)
        floor = np.sqrt(3.0 * (w[part].sum() + 16.0 * kw["smoothness"] * len(w))) * 4.0 * EPS * float(np.abs(X[sl, j]).max())
        rel = abs(E_dev[s, j] - E[s, j]) / max(abs(E[s, j]), 1e-300)
        worst = max(worst, rel if abs(np.sqrt(E_dev[s, j]) - np.sqrt(E[s, j])) > floor else min(rel, COST_TOL))
        assert rel <= COST_TOL or abs(np.sqrt(E_dev[s, j]) - np.sqrt(E[s, j])) <= floor, (what, s, j, E_dev[s, j], E[s, j], floor)
    print("%s: within %.2e relative of the restatement's E at the device's points" % (what, worst))


def _assert_parity(got, ref, c, kw, what, measured=None, first=None):
    for k in ("points", "residual", "irls_weight"):
        m, nrm = gc.rel_errors(got[k], ref[k]) if k != "residual" else _residual_errors(got[k], ref[k], c["points"])
        print("%s %s: max-scaled %.2e, norm-wise %.2e" % (what, k, m, nrm))
        assert m <= TOL and nrm <= TOL, (what, k, m, nrm)
    assert np.array_equal(got["status"], ref["status"]), (what, got["status"], ref["status"])
    assert (got["cost"] <= got["cost0"]).all(), what
    # the fp32 points are the fp64 ones rounded once
    assert np.array_equal(got["points"].view(np.uint32), got["points64"].astype(np.float32).view(np.uint32)), what
    # the costs, at the device's own points
    _assert_costs(got["cost"], got["points64"], c, kw, what + " cost")
    if kw.get("huber") and first is not None:                # cost0: the first iterate is the result of the same call capped at one solve
        assert np.array_equal(first["cost0"], got["cost0"]) and np.array_equal(first["cost"], first["cost0"]), what
        assert ((first["iterations"] == 1) | (first["status"] == 2)).all(), what
        _assert_costs(first["cost0"], first["points64"], c, kw, what + " cost0")
    if not kw.get("huber"):
        assert np.array_equal(got["iterations"], ref["iterations"]) and np.array_equal(got["cost0"], got["cost"]), what
    else:
        J = c["points"].shape[1]
        for s, j, sl in _tracks(c["segments"], J):
            if got["iterations"][s, j] == ref["iterations"][s, j]:
                continue
            w = None if c["weight"] is None else c["weight"][sl, j]
            E0, E1, step, extent = sc.next_step(got["points64"][sl, j], c["points"][sl, j], w, kw["smoothness"], kw["order"], kw["huber"])
            tol = kw.get("step_tolerance", 1e-6)
            print("%s track (%d,%d): %d solves against %d; from the device's iterate E %.17g -> %.17g, step %.3e against %.3e"
                  % (what, s, j, got["iterations"][s, j], ref["iterations"][s, j], E0, E1, step, tol * extent))
            assert got["status"][s, j] == sc.CAPPED or step <= tol * extent or E0 - E1 <= 1e-12 * abs(E0), (what, s, j)
    if measured is not None:
        ok = ~ref["passed"]
        dist = sc.max_scaled(got["points64"][ok], ref["points"][ok]) if ok.any() else 0.0
        measured.append(dist)
        return dist
    return None


# --------------------------------------------------------------------------------------------------------------------- 1. parity
GRID = sc.grid()


@pytest.mark.parametrize("part", range(4))
def test_smooth_tracks_matches_the_restatement(part):
    """the grid in four parts; measured worst distance of the device's float64 points from the restatement: see the module's
    docstring (every case is asserted against 100 times the distance of the two float64 formulations on that case)"""
    worst, worst_ratio = 0.0, 0.0
    for name, ckw, kw in GRID[part::4]:
        c, kw, ref = sc.reference(name)
        got = _run(c, **kw)
        first = _run(c, max_iterations=1, **kw) if kw["huber"] else None
        dist = _assert_parity(got, ref, c, kw, name, measured=[], first=first)
        between = max(sc.formulation_distance(c, **kw), EPS)
        print("%s: device float64 off the restatement by %.2e, the two formulations %.2e apart" % (name, dist, between))
        assert dist <= FORMULATION_MARGIN * between, (name, dist, between)
        worst, worst_ratio = max(worst, dist), max(worst_ratio, dist / between)
    print("part %d: worst device distance %.2e, worst ratio to the formulation distance %.1f" % (part, worst, worst_ratio))


@pytest.mark.parametrize("T,J,huber", [(4096, 3, None), (4096, 3, sc.HUBER), (65536, 1, None)])
def test_long_tracks(T, J, huber):
    """beyond the reach of a dense matrix the restatement is the banded formulation"""
    c = sc.case(T, J, weights="random", gaps="middle40", outliers=huber is not None)
    kw = dict(smoothness=1.0, order=2, huber=huber, max_iterations=6)
    ref = sc.smooth(c["points"], c["weight"], c["segments"], **kw)
    got = _run(c, **kw)
    _assert_parity(got, ref, c, kw, "T%d J%d %s" % (T, J, "huber" if huber else "plain"))


# ---------------------------------------------------------------------------------------------------------------- 2. independence
def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def test_a_track_does_not_depend_on_its_company():
    seg = sc.SEGMENT_LISTS["mixed"]
    c = sc.case(sum(seg), 17, segments=seg, weights="mixed", nan_points=True, outliers=True)
    kw = dict(smoothness=1.0, order=2, huber=sc.HUBER)
    whole = _run(c, **kw)
    again = _run(c, **kw)
    for k in whole:
        assert _same_bits(whole[k], again[k]), k
    t0 = 0
    for s, n in enumerate(seg):                              # every segment alone
        alone = _run(c, points=c["points"][t0:t0 + n], weight=c["weight"][t0:t0 + n], segments=(n,), **kw)
        for k in ("points", "residual", "irls_weight", "points64"):
            assert _same_bits(alone[k], whole[k][t0:t0 + n]), (s, k)
        for k in ("cost0", "cost", "iterations", "status"):
            assert _same_bits(alone[k][0], whole[k][s]), (s, k)
        t0 += n
    for j in (0, 5, 16):                                     # a joint alone
        alone = _run(c, points=c["points"][:, j:j + 1], weight=c["weight"][:, j:j + 1], **kw)
        for k in ("points", "residual", "irls_weight", "points64"):
            assert _same_bits(alone[k][:, 0], whole[k][:, j]), (j, k)
        for k in ("cost0", "cost", "iterations", "status"):
            assert _same_bits(alone[k][:, 0], whole[k][:, j]), (j, k)


# ---------------------------------------------------------------------------------------------------------------- 3. pass-through
def test_passed_through_tracks_return_the_given_bits():
    T, J = 130, 3
    c = sc.case(T, J, weights="mixed", nan_points=True)
    bits = c["points"].copy().view(np.uint32)
    nan = np.isnan(c["points"])
    bits[nan] = 0x7FC01234                                   # NaN with a payload
    pts = bits.view(np.float32)
    part = np.isfinite(pts).all(-1) & (c["weight"] > 0) & np.isfinite(c["weight"])
    got = _run(c, points=pts, smoothness=1.0, max_iterations=0)
    assert (got["status"] == 2).all() and (got["iterations"] == 0).all() and (got["cost"] == 0).all() and (got["cost0"] == 0).all()
    assert np.array_equal(got["points"].view(np.uint32), bits)
    assert np.array_equal(got["residual"][part], np.zeros(part.sum(), np.float32)) and np.isnan(got["residual"][~part]).all()
    assert np.array_equal(got["irls_weight"], part.astype(np.float32))
    # starved tracks: joint 0 nothing, joint 1 one frame, joint 2 two frames
    w = np.zeros((T, J), np.float32)
    w[40, 1] = 1.0
    w[[7, 90], 2] = 2.0
    finite = np.nan_to_num(pts, nan=0.25)
    for order, want in ((1, [2, 0, 0]), (2, [2, 2, 0])):
        for huber in (None, sc.HUBER):
            got = _run(c, points=finite, weight=w, smoothness=1.0, order=order, huber=huber)
            ref = sc.smooth(finite, w, None, smoothness=1.0, order=order, huber=huber)
            assert list(got["status"][0]) == want and np.array_equal(ref["status"], got["status"]), (order, huber)
            for j in range(J):
                if want[j] == 2:
                    assert np.array_equal(got["points"][:, j].view(np.uint32), finite[:, j].view(np.uint32))
                    assert got["iterations"][0, j] == 0 and got["cost"][0, j] == 0
            _assert_parity(got, ref, dict(c, points=finite, weight=w), dict(smoothness=1.0, order=order, huber=huber), "starved o%d" % order)
    # a starved track with NaN points keeps their payloads
    got = _run(c, points=pts, weight=w, smoothness=1.0, order=2)
    assert np.array_equal(got["points"][:, :2].view(np.uint32), bits[:, :2])


# ------------------------------------------------------------------------------------------------------------- 4. input validation
def test_refusals_are_raised_before_any_launch():
    from openmpl_amd import cabi, smooth_tracks
    from tests.guarded import Guarded
    T, J = 12, 3
    P = torch.zeros((T, J, 3), device="cuda")
    Wt = torch.ones((T, J), device="cuda")
    bad = [
        (dict(points=P.cpu()), RuntimeError), (dict(points=P.double()), RuntimeError), (dict(points=P[..., :2]), RuntimeError),
        (dict(points=P[:, :, None]), RuntimeError), (dict(weight=Wt.cpu()), RuntimeError), (dict(weight=Wt.double()), RuntimeError),
        (dict(weight=Wt[:, :2]), RuntimeError), (dict(segments=(5, 6)), ValueError), (dict(segments=(12, 0)), ValueError),
        (dict(segments=()), ValueError), (dict(segments=(6.5, 5.5)), ValueError), (dict(segments=(-1, 13)), ValueError),
        (dict(smoothness=0.0), RuntimeError), (dict(smoothness=float("nan")), RuntimeError), (dict(smoothness=float("inf")), RuntimeError),
        (dict(smoothness=-1.0), RuntimeError), (dict(order=0), RuntimeError), (dict(order=3), RuntimeError),
        (dict(max_iterations=-1), RuntimeError), (dict(max_iterations=1001), RuntimeError), (dict(max_iterations=2.5), RuntimeError),
        (dict(step_tolerance=-1.0), RuntimeError), (dict(step_tolerance=float("nan")), RuntimeError),
        (dict(points=torch.zeros((T, cabi.SMOOTH_MAX_JOINTS + 1, 3), device="cuda"), weight=None), RuntimeError),
        (dict(points=torch.zeros((cabi.SMOOTH_MAX_SEGMENT + 1, 1, 3), device="cuda"), weight=None), ValueError),
    ]
    for kw, exc in bad:
        args = dict(points=P, weight=Wt, smoothness=1.0)
        args.update(kw)
        with Guarded("cuda") as g:
            with pytest.raises(exc):
                smooth_tracks(**args)
        assert g.launches == [], (kw, g.launches)
    # and the C ABI itself: a missing or short workspace, a flag of the laboratory, a table that does not sum
    lib = cabi.load()
    seg = (cabi.C.c_int * 1)(T)
    table = torch.tensor([0, T], dtype=torch.int32, device="cuda")
    need = lib.mpl_smooth_tracks_workspace_bytes(T, J, 1)
    assert need > 0 and lib.mpl_smooth_tracks_workspace_bytes(0, J, 1) == 0 and lib.mpl_smooth_tracks_workspace_bytes(T, J, T + 1) == 0
    ws = torch.empty((need,), dtype=torch.uint8, device="cuda")
    outs = [torch.empty((T, J, 3), device="cuda"), torch.empty((T, J), device="cuda"), torch.empty((T, J), device="cuda"),
            torch.empty((1, J), dtype=torch.float64, device="cuda"), torch.empty((1, J), dtype=torch.float64, device="cuda"),
            torch.empty((1, J), dtype=torch.int32, device="cuda"), torch.empty((1, J), dtype=torch.uint8, device="cuda")]

    def call(seg=seg, S=1, frames=T, flags=0, ws_ptr=ws.data_ptr(), ws_bytes=need, order=2, lam=1.0):
        return lib.mpl_smooth_tracks(P.data_ptr(), None, seg, table.data_ptr(), S, frames, J, lam, order, 0.0, 20, 1e-6, flags, ws_ptr, ws_bytes,
                                     *(t.data_ptr() for t in outs), None, None)
    cabi.profile_start()
    codes = [call(ws_ptr=None), call(ws_bytes=need - 1), call(flags=2), call(frames=T + 1), call(order=3), call(lam=0.0),
             call(seg=(cabi.C.c_int * 1)(cabi.SMOOTH_MAX_SEGMENT + 1), frames=cabi.SMOOTH_MAX_SEGMENT + 1)]
    torch.cuda.synchronize()
    assert sum(n for _, n in cabi.profile_stop().values()) == 0
    assert codes == [-3, -3, -1, -1, -1, -2, -1], codes


# --------------------------------------------------------------------------------------------------------------- 5. the closed loop
def test_closed_loop_on_the_device():
    """placed poses -> synthesize_views(noise_level=2) -> triangulate_pixels(refine=True) -> smooth_tracks on the device, beside the
    float64 chain (the restatements of refine_cases on the device's own pixels, then of this module): the mean distance to the placed
    poses after smoothing stays within 1.1 times the float64 chain's and below the unsmoothed figure"""
    from tests import smooth_loop
    r = smooth_loop.closed_loop()
    print("closed loop: unsmoothed %.5f, smoothed on the device %.5f, float64 chain %.5f" % (r["raw"], r["device"], r["float64"]))
    assert r["device"] <= 1.1 * r["float64"] and r["device"] < r["raw"]
