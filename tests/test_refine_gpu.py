"""Reprojection-error refinement on the device (csrc/refine.hip, openmpl_amd.geometry.refine_points / reprojection_errors /
triangulate_pixels(refine=)) against the float64 restatement of tests/refine_cases.py.

Parity is the rule of DESIGN.md section 2 (geometry_cases.rel_errors): max|d| <= 1e-4 max|ref| and norm-wise 1e-4, NaN in the same
places.  The trial count is never compared: the device contracts multiply-adds, and a trial whose cost ties with the current one to
the last bits may be accepted on one side only.  What does not depend on the restatement's trajectory is checked beside it: the
restatement's cost at the point the device returns is no higher than at the point it was given."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import distortion_cases as dc
from tests import geometry_cases as gc
from tests import refine_cases as rc
from tests import synth_cases as sc

pytestmark = pytest.mark.gpu

SHAPES = [(3, 2, 17), (5, 3, 17), (2, 4, 64), (1, 32, 3), (1, 1, 1)]       # two views; 85 items across a 64-item workgroup; the
#                                                                            joint limit; the view limit; one item, passed through
TOL = 1e-4
HUBER = 2.5            # px: with 2 px of noise per axis about a third of the observations lie on the linear part of the cost


@pytest.fixture(autouse=True)
def _device_error_is_clear():
    yield
    from openmpl_amd import cabi
    torch.cuda.synchronize()
    assert not cabi.device_error()


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _launches(fn):
    from openmpl_amd import cabi
    torch.cuda.synchronize()
    cabi.profile_start()
    try:
        res = fn()
    finally:
        torch.cuda.synchronize()
        counts = cabi.profile_stop()
    return res, sum(n for _, n in counts.values())


def _run(c, points=None, pixels=None, conf="case", lens=True, **kw):
    """refine_points on a case of refine_cases -> (dict of numpy arrays, launches)"""
    from openmpl_amd import refine_points
    cf = c["conf"] if isinstance(conf, str) else conf
    args = (_dev(c["points0"] if points is None else points), _dev(c["pixels"] if pixels is None else pixels), _dev(cf), _dev(c["cams"]))
    D = _dev(c["dist"]) if lens else None
    r, n = _launches(lambda: refine_points(*args, distortion=D, **kw))
    assert r.points.dtype == torch.float32 and r.error.dtype == torch.float32 and r.errors.dtype == torch.float32
    assert r.iterations.dtype == torch.int32 and r.status.dtype == torch.uint8
    return {k: getattr(r, k).cpu().numpy() for k in r._fields}, n


def _assert_parity(got, ref, what):
    for k in ("points", "error", "errors"):
        m, nrm = gc.rel_errors(got[k], ref[k])
        print("%s %s: max-scaled %.2e, norm-wise %.2e" % (what, k, m, nrm))
        assert m <= TOL and nrm <= TOL, (what, k, m, nrm)


def _assert_cost_did_not_rise(got, c, conf, huber, what):
    """the restatement's E at the device's fp32 point against E at the given point plus one fp32 rounding of the point"""
    ok = got["status"] < 3
    X = np.where(ok[..., None], got["points"].astype(np.float64), c["points0"].astype(np.float64))
    E = rc.cost(X, c["pixels"], conf, c["cams"], c["dist"], huber)
    E0 = rc.cost(c["points0"], c["pixels"], conf, c["cams"], c["dist"], huber)
    slack = rc.rounding_slack(X, c["pixels"], conf, c["cams"], c["dist"], huber)
    with np.errstate(invalid="ignore"):
        worst = float(np.max((E - E0)[ok], initial=-np.inf))
    print("%s: E(device point) - E(given point) at most %.3e px^2 (slack up to %.1e)" % (what, worst, float(np.max(slack[ok], initial=0.0))))
    assert (E[ok] <= E0[ok] + slack[ok]).all(), what


# --------------------------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("B,V,J", SHAPES)
@pytest.mark.parametrize("name", dc.SETS)
def test_refine_points_matches_the_restatement(B, V, J, name):
    for conf in ("none", "uniform", "mixed"):
        # plain mode, run with room to spare: the restatement converges within 20 trials (asserted by the builder), so that 0
        # against 1 is compared exactly
        c, ref = rc.plain_case_converging(B, V, J, name, conf=conf)
        got, n = _run(c, max_iterations=50)
        what = "%s %s plain conf=%s" % ((B, V, J), name, conf)
        assert n == 1, what
        _assert_parity(got, ref, what)
        assert np.array_equal(got["status"], ref["status"]), what
        assert (got["iterations"][ref["status"] >= 2] == 0).all() and (got["iterations"] <= 50).all()
        _assert_cost_did_not_rise(got, c, c["conf"], None, what)
        # Huber mode at the default cap
        ref = rc.refine(c["points0"], c["pixels"], c["conf"], c["cams"], c["dist"], HUBER)
        got, n = _run(c, huber=HUBER)
        what = "%s %s huber conf=%s" % ((B, V, J), name, conf)
        assert n == 1, what
        _assert_parity(got, ref, what)
        assert np.array_equal(got["status"] == 2, ref["status"] == 2) and np.array_equal(got["status"] == 3, ref["status"] == 3), what
        assert np.isin(got["status"][ref["status"] < 2], (0, 1)).all() and (got["iterations"] <= 20).all()
        _assert_cost_did_not_rise(got, c, c["conf"], HUBER, what)
        if V >= 2 and B * J > 1:
            assert (ref["status"] == 0).any() and (ref["accepted"] > 0).any()        # the case does what it is there for


def test_no_distortion_is_the_pinhole_and_zero_coefficients_agree():
    c = rc.case(5, 3, 17, "zeros", conf="uniform")
    ref = rc.refine(c["points0"], c["pixels"], c["conf"], c["cams"], None)
    got, n = _run(c, lens=False)
    assert n == 1
    _assert_parity(got, ref, "pinhole")
    zer, _ = _run(c)
    _assert_parity(zer, ref, "zero coefficients")
    assert np.array_equal(got["status"], zer["status"])


# --------------------------------------------------------------------------------------------------------- 2. reprojection_errors
@pytest.mark.parametrize("B,V,J", SHAPES)
def test_reprojection_errors(B, V, J):
    from openmpl_amd import reprojection_errors
    c = rc.case(B, V, J, "per_view", conf="mixed")
    P, X, Cf, Cm, D = _dev(c["points0"]), _dev(c["pixels"]), _dev(c["conf"]), _dev(c["cams"]), _dev(c["dist"])
    (errors, error), n = _launches(lambda: reprojection_errors(P, X, Cf, Cm, D))
    assert n == 1 and errors.shape == (B, V, J) and error.shape == (B, J)
    zero, _ = _run(c, max_iterations=0)
    assert np.array_equal(errors.cpu().numpy(), zero["errors"], equal_nan=True) and np.array_equal(error.cpu().numpy(), zero["error"])
    assert np.array_equal(zero["points"].view(np.uint32), c["points0"].view(np.uint32))          # the input, bit for bit
    assert (zero["status"] == 2).all() and (zero["iterations"] == 0).all()
    # against the projection itself, on noisy pixels
    px, _ = dc.project(c["points0"], c["cams"], c["dist"])
    part, w = rc.participation(c["pixels"], c["conf"])
    d = np.linalg.norm(px - c["pixels"].astype(np.float64), axis=-1)
    ref_errors = np.where(part, d, np.nan)
    ref_error = np.sqrt(np.sum(w * np.where(part, d, 0.0) ** 2, axis=1) / w.sum(axis=1))
    for k, g, r in (("errors", errors, ref_errors), ("error", error, ref_error)):
        m, nrm = gc.rel_errors(g.cpu().numpy(), r)
        print("reprojection_errors %s %s: max-scaled %.2e, norm-wise %.2e (up to %.1f px)" % ((B, V, J), k, m, nrm, np.nanmax(r)))
        assert m <= TOL and nrm <= TOL
    assert np.nanmax(ref_errors) > 1.0


# --------------------------------------------------------------------------------------------------------------- 3. isolation
def test_invalid_and_passed_through_items_stay_in_their_item():
    B, V, J = 5, 3, 17
    c = rc.case(B, V, J, "h36m", conf="uniform")
    base, _ = _run(c)
    x0, cf = c["points0"].copy(), c["conf"].copy()
    x0[0, 3, 1] = np.nan                                                      # a NaN point
    x0[1, 5] = (c["cams"][1, 13:16] - 2.0 * c["cams"][1, 10:13]).astype(np.float32)      # behind camera 1, which takes part
    cf[2, :, 7] = 0.0                                                         # all weights zero
    cf[3, 1:, 9] = (np.nan, -0.5)                                             # one view left
    hit = np.zeros((B, J), bool)
    hit[0, 3] = hit[1, 5] = hit[2, 7] = hit[3, 9] = True
    got, n = _run(c, points=x0, conf=cf)
    assert n == 1
    ref = rc.refine(x0, c["pixels"], cf, c["cams"], c["dist"])
    assert [int(got["status"][i]) for i in ((0, 3), (1, 5), (2, 7), (3, 9))] == [3, 3, 3, 2]
    assert np.array_equal(got["status"][hit], ref["status"][hit])
    for k in ("points", "error", "iterations", "status"):
        assert np.array_equal(got[k][~hit], base[k][~hit]), k                  # every other item: the bits of the undisturbed run
    assert np.array_equal(np.transpose(got["errors"], (0, 2, 1))[~hit], np.transpose(base["errors"], (0, 2, 1))[~hit])
    inv = hit & (got["status"] == 3)
    assert np.isnan(got["points"][inv]).all() and np.isnan(got["error"][inv]).all() and np.isnan(np.transpose(got["errors"], (0, 2, 1))[inv]).all()
    assert (got["iterations"][hit] == 0).all()
    # one view left: the point bit for bit, the error that of the one view
    assert np.array_equal(got["points"][3, 9].view(np.uint32), x0[3, 9].view(np.uint32))
    assert np.isfinite(got["errors"][3, 0, 9]) and np.isnan(got["errors"][3, 1:, 9]).all() and got["error"][3, 9] == got["errors"][3, 0, 9]
    _assert_parity(got, ref, "disturbed")


def test_runs_and_batchings_give_identical_bits():
    B, V, J = 70, 3, 5
    c = rc.case(B, V, J, "per_view", conf="mixed")
    for kw in (dict(), dict(huber=HUBER)):
        a, _ = _run(c, **kw)
        b, _ = _run(c, **kw)
        parts = [_run(c, points=c["points0"][s], pixels=c["pixels"][s], conf=c["conf"][s], **kw)[0] for s in (slice(0, 1), slice(1, B))]
        for k in a:
            assert np.array_equal(a[k], b[k], equal_nan=True), k
            assert np.array_equal(a[k], np.concatenate([p[k] for p in parts], axis=0), equal_nan=True), k


# ------------------------------------------------------------------------------------------------------------- 4. the closed loop
def test_closed_loop_refinement_of_triangulated_detections():
    """synthesize_views(noise_level=2) under the H36M-like lens -> triangulate_pixels(refine=True) against refine=False.  With 102
    joints the gain of the float64 chain at this seed is a few per cent of the linear error (printed); the device has to show a
    refined mean no larger than the linear one and land on the float64 chain's mean."""
    from openmpl_amd import PoseEvaluator, synthesize_views, triangulate_pixels
    B, V, J = 6, 4, 17
    poses3d, cams = sc.scene(B, V, J, seed=13, focal=dc.FOCAL)
    dist = dc.table("h36m", V)
    P, Cm, D = _dev(poses3d), _dev(cams), _dev(dist)
    r = synthesize_views(P, Cm, rc.WH, seed=21, noise_level=2.0, normalize_inputs=False, normalize_cameras=False, return_pixels=True,
                         distortion=D)
    conf = torch.stack([p[..., 2] for p in r.poses], dim=1).contiguous()
    placed = poses3d.astype(np.float64)
    dist_to = lambda x: float(np.linalg.norm(np.asarray(x, dtype=np.float64) - placed, axis=-1).mean())      # noqa: E731
    (lin, res, inl), n_lin = _launches(lambda: triangulate_pixels(r.pixels, conf, Cm, rc.WH, distortion=D))
    (off, res0, inl0), n_off = _launches(lambda: triangulate_pixels(r.pixels, conf, Cm, rc.WH, distortion=D, refine=False))
    (ref_, res1, inl1), n_on = _launches(lambda: triangulate_pixels(r.pixels, conf, Cm, rc.WH, distortion=D, refine=True))
    assert n_lin == 2 and n_off == 2 and n_on == 3
    assert torch.equal(off, lin) and torch.equal(res0, res) and torch.equal(inl0, inl)
    assert torch.equal(res1, res) and torch.equal(inl1, inl) and not torch.equal(ref_, lin)
    # the float64 chain on the same fp32 pixels
    px, cf = r.pixels.cpu().numpy(), conf.cpu().numpy()
    x64 = rc.linear_points(px, cf, cams, dist).astype(np.float32)
    r64 = rc.refine(x64, px, cf, cams, dist)
    e_lin, e_ref, e_lin64, e_ref64 = dist_to(lin.cpu().numpy()), dist_to(ref_.cpu().numpy()), dist_to(x64), dist_to(r64["points"])
    print("closed loop, mean distance to the placed poses: linear %.5f, refined %.5f (x %.4f); float64 chain %.5f -> %.5f"
          % (e_lin, e_ref, e_ref / e_lin, e_lin64, e_ref64))
    assert bool((inl == 1).all()) and (r64["status"] == 0).all()
    assert e_ref <= e_lin
    assert abs(e_ref - e_ref64) <= TOL * e_ref64
    m, nrm = gc.rel_errors(ref_.cpu().numpy(), r64["points"])
    assert m <= TOL and nrm <= TOL
    ev = PoseEvaluator(J)
    ev.update(ref_, r.target)
    rep = ev.compute()
    assert rep["n_samples"] == B and np.isfinite(rep["absolute"]["mpjpe"])
    # the Huber option reaches the refinement
    hub, _, _ = triangulate_pixels(r.pixels, conf, Cm, rc.WH, distortion=D, refine=True, huber=HUBER)
    h64 = rc.refine(x64, px, cf, cams, dist, HUBER)
    m, nrm = gc.rel_errors(hub.cpu().numpy(), h64["points"])
    assert m <= TOL and nrm <= TOL and not torch.equal(hub, ref_)


# ------------------------------------------------------------------------------------------------------------------ the refusals
def test_refusals_of_the_c_abi_launch_nothing():
    from openmpl_amd import cabi
    lib = cabi.load()
    B, V, J = 3, 3, 17
    c = rc.case(B, V, J, "h36m")
    P, X, Cm, D = _dev(c["points0"]), _dev(c["pixels"]), _dev(c["cams"]), _dev(c["dist"])
    out = torch.full((3 + 1 + V + 1, B * J), -12345.0, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    o = lambda row: out[row].data_ptr()      # noqa: E731

    def call(points=P.data_ptr(), pixels=X.data_ptr(), cams=Cm.data_ptr(), views=V, joints=J, it=20, tol=1e-8, pts=o(0), err=o(3), batch=B):
        return lib.mpl_refine_points(points, pixels, None, cams, D.data_ptr(), batch, views, joints, 0.0, it, tol, pts, err, o(4), None, None, st)

    def refused():
        return [call(points=None), call(pixels=None), call(cams=None), call(pts=None), call(err=None), call(batch=0), call(views=0),
                call(views=33), call(joints=65), call(it=-1), call(it=1001), call(tol=-1.0), call(tol=float("nan")), call(tol=float("inf"))]

    codes, n = _launches(refused)
    assert codes == [-1] * 9 + [-2] * 5 and n == 0 and bool((out == -12345.0).all())
    # a huber that is <= 0 or NaN is the plain mode, not an error; the optional outputs may be absent
    rcs, n = _launches(lambda: [lib.mpl_refine_points(P.data_ptr(), X.data_ptr(), None, Cm.data_ptr(), None, B, V, J, h, 20, 1e-8, o(0), o(3),
                                                      None, None, None, st) for h in (float("nan"), -1.0)])
    assert rcs == [0, 0] and n == 2 and bool((out[4:] == -12345.0).all()) and bool((out[3] != -12345.0).all())


def test_python_checks_of_cams_distortion_and_limits_launch_nothing():
    from openmpl_amd import cabi, refine_points, reprojection_errors
    c = rc.case(2, 3, 5, "h36m")
    P, X, Cm, D = _dev(c["points0"]), _dev(c["pixels"]), _dev(c["cams"]), _dev(c["dist"])
    cabi.profile_start()
    for bad in (Cm[:2], Cm.float(), Cm.cpu(), Cm[:, :15]):
        with pytest.raises(RuntimeError, match="cams must be float64"):
            refine_points(P, X, None, bad)
    for bad in (D[:2], D[:, :4], D.float(), D.cpu(), D.reshape(-1)):
        with pytest.raises(RuntimeError, match="distortion must"):
            reprojection_errors(P, X, None, Cm, distortion=bad)
    with pytest.raises(RuntimeError, match="no CPU path: conf must live on a GPU"):
        refine_points(P, X, torch.ones(2, 3, 5), Cm)
    with pytest.raises(NotImplementedError, match="at most 32 views, 64 joints"):
        refine_points(torch.zeros(1, 65, 3, device="cuda"), torch.zeros(1, 2, 65, 2, device="cuda"), None, Cm[:2])
    assert sum(n for _, n in cabi.profile_stop().values()) == 0
    assert C.sizeof(C.c_int) == 4        # out_iterations is int32 on both sides
