"""Camera-pose refinement and alternating bundle adjustment on the device (csrc/refine_cameras.hip, openmpl_amd.geometry.refine_cameras
/ bundle_adjust) against the float64 restatement of tests/refine_cameras_cases.py.

The kernel runs one workgroup of T = 512 threads (8 waves) per view over the N = B J observations of the view; the shapes are the
ones at which that can go wrong.  The trial count is printed, never compared: the device contracts multiply-adds and sums in another
order, and a trial whose cost ties with the current one to the last bits may be accepted on one side only.  What does not depend on
the restatement's trajectory is checked beside it: cost0, cost and error are the restatement's at the camera the device returns, and
its cost there is no higher than at the camera it was given."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import distortion_cases as dc
from tests import refine_cameras_cases as cc
from tests import refine_cases as rc

pytestmark = pytest.mark.gpu

T = 512
SHAPES = [(1, 4, 3), (1, 4, 17), (4, 1, 17), (2, 32, 5), (64, 4, 17), (70, 3, 17)]
#          N = 3, the minimum that iterates; less than one wave; a single view (grid of 1); the view limit; N = 1088 > 2 T;
#          N = 1190: T < N, N % T = 166, N % 64 = 38
TOL = 1e-8             # step_tolerance of every run
HUBER = 2.5            # px: with 2 px of noise per axis about a third of the observations lie on the linear part of the cost
RTOL = 1e-10           # cost0, cost, error: fp64 sums of at most 2e3 non-negative terms that differ in order, about N 2^-53
# A residual is the difference of two pixel coordinates of up to 1e3, each a handful of fp64 roundings (contracted on the device): 64
# ulp of 1e3.  It only shows where the fit is exact (N = 3: six equations, six unknowns) and the cost is all cancellation
DELTA = 64 * 2.0 ** -52 * 1e3
EXACT_FIT = 1e-3       # px: a view whose restated RMS is below this is such a fit


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


def _run(c, points=None, pixels=None, conf="case", cams=None, lens=True, **kw):
    """refine_cameras on a case of refine_cameras_cases -> (dict of numpy arrays, launches)"""
    from openmpl_amd import refine_cameras
    cf = c["conf"] if isinstance(conf, str) else conf
    args = (_dev(c["points"] if points is None else points), _dev(c["pixels"] if pixels is None else pixels), _dev(cf),
            _dev(c["cams0"] if cams is None else cams))
    D = _dev(c["dist"]) if lens else None
    r, n = _launches(lambda: refine_cameras(*args, distortion=D, **kw))
    V = args[3].shape[0]
    assert r.cams.dtype == torch.float64 and r.cams.shape == (V, 16)
    assert all(getattr(r, k).dtype == torch.float64 and getattr(r, k).shape == (V,) for k in ("error", "cost0", "cost"))
    assert r.used.dtype == torch.int32 and r.iterations.dtype == torch.int32 and r.status.dtype == torch.uint8
    return {k: getattr(r, k).cpu().numpy() for k in r._fields}, n


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else a.dtype)


def _same_bits(a, b, rows=slice(None)):
    return all(np.array_equal(_bits(a[k][rows]), _bits(b[k][rows])) for k in a)


def _close(got, want, exact_fit, atol, what):
    """rtol RTOL, NaN in the same places; `atol` more in the views that are exact fits"""
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    bound = RTOL * np.abs(want) + np.where(exact_fit, atol, 0.0)
    with np.errstate(invalid="ignore"):
        worst = float(np.max((np.abs(got - want) / np.where(want != 0, np.abs(want), 1.0))[ok & ~exact_fit], initial=0.0))
    assert (np.abs(got - want)[ok] <= bound[ok]).all(), (what, got, want)
    return worst


def _check(got, ref, c, cams0, conf, dist, huber, max_it, what, points=None):
    X = c["points"] if points is None else points
    args = (X, c["pixels"], conf)
    assert np.array_equal(got["used"], ref["used"]), what
    sure, iterates = cc.sure(ref, max_it), ref["status"] < 2
    assert np.array_equal(got["status"][sure], ref["status"][sure]), (what, got["status"], ref["status"])
    assert np.isin(got["status"][iterates], (0, 1)).all(), what
    assert (got["iterations"][~iterates] == 0).all() and (got["iterations"] <= max_it).all() and (got["iterations"][iterates] >= 1).all()
    assert np.array_equal(_bits(got["cams"][:, :4]), _bits(cams0[:, :4])), what               # intrinsics: copied
    assert np.array_equal(_bits(got["cams"][~iterates]), _bits(cams0[~iterates])), what      # passed through or invalid: bit for bit
    # cost0, cost and error are the restatement's at the given camera and at the device's own
    err_at, E_at = cc.score(*args, got["cams"], dist, huber)
    _, E_given = cc.score(*args, cams0, dist, huber)
    W = cc.evaluate(*args, cams0, dist, huber)["W"]
    with np.errstate(invalid="ignore"):
        fit = np.nan_to_num(err_at, nan=np.inf) < EXACT_FIT
        atol_cost = 2.0 * np.sqrt(np.nan_to_num(E_at) * W) * DELTA + W * DELTA * DELTA
    worst = max(_close(got["cost0"], E_given, np.zeros_like(fit), 0.0, what + " cost0"),
                _close(got["cost"], E_at, fit, atol_cost, what + " cost"), _close(got["error"], err_at, fit, 2.0 * DELTA, what + " error"))
    valid = got["status"] < 3
    assert (E_at[valid] <= E_given[valid]).all() and (got["cost"][valid] <= got["cost0"][valid]).all(), what
    assert np.array_equal(_bits(got["cost"][got["status"] == 2]), _bits(got["cost0"][got["status"] == 2])), what
    # the pose, where both runs stop because their step is below the tolerance
    both = sure & iterates
    dR = np.abs(got["cams"][:, 4:13] - ref["cams"][:, 4:13]).max(axis=1)
    dt = np.abs(got["cams"][:, 13:] - ref["cams"][:, 13:]).max(axis=1) / np.where(np.isfinite(ref["zmin"]), ref["zmin"], 1.0)
    print("%s: trials %s (restated %s), status %s, cost / error off by %.1e, R off by %.1e, centre by %.1e of the depth (in units of the "
          "tolerance: %.2f, %.2f)" % (what, got["iterations"], ref["iterations"], got["status"], worst, dR[both].max(initial=0.0),
                                      dt[both].max(initial=0.0), dR[both].max(initial=0.0) / TOL, dt[both].max(initial=0.0) / TOL))
    assert (dR[both] <= 10 * TOL).all() and (dt[both] <= 10 * TOL).all(), what
    assert cc.rotation_error(got["cams"][np.isfinite(cams0).all(axis=1)]) <= 1e-12, what


def _parity(B, V, J, name, lens, confs, hubers):
    for conf in confs:
        c = cc.case(B, V, J, name, conf=conf, nan_points=7)
        dist = c["dist"] if lens else None
        for huber in hubers:
            max_it = 50 if huber is None else 100
            ref = cc.refine(c["points"], c["pixels"], c["conf"], c["cams0"], dist, huber, max_it, TOL)
            got, n = _run(c, lens=lens, huber=huber, max_iterations=max_it, step_tolerance=TOL)
            what = "%s %s %s conf=%s huber=%s" % ((B, V, J), name, "lens" if lens else "pinhole", conf, huber)
            assert n == 1, what
            _check(got, ref, c, c["cams0"], c["conf"], dist, huber, max_it, what)
            # the views whose pose is compared: all that iterate under the plain cost with clean confidences; elsewhere (Huber's
            # linear convergence, or a handful of observations left at N = 10) nine in ten, and never none
            iterates = ref["status"] < 2
            compared = int((cc.sure(ref, max_it) & iterates).sum())
            print("%s: pose compared in %d of %d views that iterate" % (what, compared, int(iterates.sum())))
            if huber is None and conf != "mixed":
                assert compared == iterates.sum() > 0, what
            else:
                assert compared >= max(1, int(np.ceil(0.9 * iterates.sum()))), what


# --------------------------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("B,V,J", SHAPES)
@pytest.mark.parametrize("lens", [True, False])
def test_refine_cameras_matches_the_restatement(B, V, J, lens):
    _parity(B, V, J, "h36m" if lens else "zeros", lens, ("none", "uniform", "mixed"), (None, HUBER))


@pytest.mark.parametrize("name", dc.SETS)
def test_every_lens_set(name):
    _parity(70, 3, 17, name, True, ("uniform",), (None, HUBER))


def test_zero_coefficients_agree_with_the_pinhole_kernel():
    c = cc.case(70, 3, 17, "zeros", conf="uniform")
    a, _ = _run(c, lens=True)
    b, _ = _run(c, lens=False)
    assert np.array_equal(a["status"], b["status"]) and np.array_equal(a["used"], b["used"])
    assert np.abs(a["cams"] - b["cams"]).max() <= 10 * TOL * max(1.0, np.abs(a["cams"][:, 13:]).max())
    np.testing.assert_allclose(a["cost"], b["cost"], rtol=RTOL)


# ------------------------------------------------------------------------------------------------------------------ 2. isolation
def test_spoiled_views_stay_in_their_view():
    B, V, J = 4, 5, 17
    c = cc.case(B, V, J, "h36m", conf="uniform")
    cf = c["conf"].copy()
    cf[1, (0, 1, 2, 4), 5] = 0.0                                               # a point only camera 3 sees
    base, _ = _run(c, conf=cf)
    X, cams = c["points"].copy(), c["cams0"].copy()
    cf2 = cf.copy()
    cf2[:, 1] = 0.0                                                            # view 1: no observation
    cf2[:, 2] = np.nan
    cf2[0, 2, :2] = 0.7                                                        # view 2: two observations
    X[1, 5] = (cams[3, 13:16] - 2.0 * cams[3, 10:13]).astype(np.float32)      # view 3: a participating point behind the camera
    cams[4, 9] = np.nan                                                        # view 4: a record that is not finite
    got, n = _run(c, points=X, conf=cf2, cams=cams)
    ref = cc.refine(X, c["pixels"], cf2, cams, c["dist"])
    assert n == 1 and list(got["status"][1:]) == [3, 2, 3, 3] and np.array_equal(got["status"], ref["status"])
    assert _same_bits(got, base, rows=slice(0, 1))                             # the neighbour: the bits of the undisturbed run
    assert base["status"][0] == 0 and (base["status"] < 2).all()
    assert np.array_equal(_bits(got["cams"][1:]), _bits(cams[1:]))             # as given, the NaN row too
    assert np.isnan(got["error"][[1, 3, 4]]).all() and np.isnan(got["cost0"][[1, 3, 4]]).all() and np.isnan(got["cost"][[1, 3, 4]]).all()
    assert np.isfinite(got["error"][2]) and got["cost"][2] == got["cost0"][2] and list(got["used"]) == list(ref["used"])
    assert got["used"][1] == 0 and got["used"][2] == 2 and (got["iterations"][1:] == 0).all()
    _check(got, ref, c, cams, cf2, c["dist"], None, 20, "spoiled", points=X)


def test_fixed_views_and_no_iterations_return_their_rows_bit_for_bit():
    c = cc.case(8, 4, 17, "per_view", conf="uniform")
    free, _ = _run(c)
    got, n = _run(c, fixed=(0, 2))
    assert n == 1 and list(got["status"]) == [2, free["status"][1], 2, free["status"][3]] and (free["status"] == 0).all()
    assert np.array_equal(_bits(got["cams"][[0, 2]]), _bits(c["cams0"][[0, 2]]))
    assert _same_bits(got, free, rows=[1, 3])                                  # the other views do not know
    for k in (0, 2):
        assert got["cost"][k] == got["cost0"][k] == free["cost0"][k] and got["iterations"][k] == 0 and got["used"][k] == free["used"][k]
    _check(got, cc.refine(c["points"], c["pixels"], c["conf"], c["cams0"], c["dist"], fixed=(0, 2)), c, c["cams0"], c["conf"], c["dist"],
           None, 20, "fixed")
    zero, n = _run(c, max_iterations=0, huber=HUBER)
    assert n == 1 and (zero["status"] == 2).all() and (zero["iterations"] == 0).all()
    assert np.array_equal(_bits(zero["cams"]), _bits(c["cams0"])) and np.array_equal(_bits(zero["cost"]), _bits(zero["cost0"]))
    np.testing.assert_allclose(zero["error"], free["cost0"] ** 0.5 / cc.evaluate(c["points"], c["pixels"], c["conf"], c["cams0"],
                                                                                c["dist"])["W"] ** 0.5, rtol=RTOL)


def test_runs_give_identical_bits():
    c = cc.case(70, 3, 17, "per_view", conf="mixed", nan_points=5)
    for kw in (dict(), dict(huber=HUBER)):
        a, _ = _run(c, **kw)
        b, _ = _run(c, **kw)
        assert _same_bits(a, b) and (a["status"] < 2).all()


# -------------------------------------------------------------------------------------------------------------------- the C ABI
def _abi_call(lib, P, X, Cm, D, outs, B, V, J, cams_out, it=20, tol=TOL, mask=0, **over):
    st = torch.cuda.current_stream().cuda_stream
    a = dict(points=P.data_ptr(), pixels=X.data_ptr(), cams=Cm.data_ptr(), out=cams_out, err=outs["error"].data_ptr(), batch=B, views=V,
             joints=J)
    a.update(over)
    return lib.mpl_refine_cameras(a["points"], a["pixels"], None, a["cams"], D.data_ptr(), a["batch"], a["views"], a["joints"], 0.0, it, tol,
                                  mask, a["out"], a["err"], outs["cost0"].data_ptr(), outs["cost"].data_ptr(), outs["used"].data_ptr(),
                                  outs["iterations"].data_ptr(), outs["status"].data_ptr(), st)


def _abi_outputs(V):
    return dict(cams=torch.full((V, 16), -12345.0, dtype=torch.float64, device="cuda"),
                error=torch.full((V,), -12345.0, dtype=torch.float64, device="cuda"),
                cost0=torch.full((V,), -12345.0, dtype=torch.float64, device="cuda"),
                cost=torch.full((V,), -12345.0, dtype=torch.float64, device="cuda"),
                used=torch.full((V,), -12345, dtype=torch.int32, device="cuda"),
                iterations=torch.full((V,), -12345, dtype=torch.int32, device="cuda"),
                status=torch.full((V,), 99, dtype=torch.uint8, device="cuda"))


def test_out_cams_may_alias_cams_dev():
    from openmpl_amd import cabi
    lib = cabi.load()
    B, V, J = 8, 4, 17
    c = cc.case(B, V, J, "h36m")
    P, X, Cm, D = _dev(c["points"]), _dev(c["pixels"]), _dev(c["cams0"]), _dev(c["dist"])
    apart, inplace = _abi_outputs(V), _abi_outputs(V)
    alias = Cm.clone()
    codes, n = _launches(lambda: [_abi_call(lib, P, X, Cm, D, apart, B, V, J, apart["cams"].data_ptr()),
                                  _abi_call(lib, P, X, alias, D, inplace, B, V, J, alias.data_ptr())])
    assert codes == [0, 0] and n == 2
    inplace["cams"] = alias
    for k in apart:
        assert torch.equal(apart[k].view(torch.uint8), inplace[k].view(torch.uint8)), k
    assert torch.equal(Cm, _dev(c["cams0"])) and not torch.equal(alias, Cm) and bool((apart["status"] == 0).all())
    # bits of the mask at or above `views` are ignored; the optional outputs may be absent
    other = _abi_outputs(V)
    st = torch.cuda.current_stream().cuda_stream
    codes, n = _launches(lambda: [_abi_call(lib, P, X, Cm, D, other, B, V, J, other["cams"].data_ptr(), mask=0xfffffff0),
                                  lib.mpl_refine_cameras(P.data_ptr(), X.data_ptr(), None, Cm.data_ptr(), None, B, V, J, float("nan"), 20, TOL,
                                                         0, inplace["cams"].data_ptr(), inplace["error"].data_ptr(), None, None, None, None,
                                                         None, st)])
    assert codes == [0, 0] and n == 2
    for k in apart:
        assert torch.equal(apart[k].view(torch.uint8), other[k].view(torch.uint8)), k


def test_refusals_of_the_c_abi_launch_nothing():
    from openmpl_amd import cabi
    lib = cabi.load()
    B, V, J = 3, 3, 17
    c = cc.case(B, V, J, "h36m")
    P, X, Cm, D = _dev(c["points"]), _dev(c["pixels"]), _dev(c["cams0"]), _dev(c["dist"])
    out = _abi_outputs(V)
    call = lambda **kw: _abi_call(lib, P, X, Cm, D, out, B, V, J, out["cams"].data_ptr(), **kw)      # noqa: E731

    def refused():
        return [call(points=None), call(pixels=None), call(cams=None), call(out=None), call(err=None), call(batch=0), call(views=0),
                call(views=33), call(joints=65), call(it=-1), call(it=1001), call(tol=-1.0), call(tol=float("nan")), call(tol=float("inf"))]

    codes, n = _launches(refused)
    assert codes == [-1] * 9 + [-2] * 5 and n == 0
    assert all(bool((t == (99 if t.dtype == torch.uint8 else -12345)).all()) for t in out.values())


def test_python_checks_launch_nothing():
    from openmpl_amd import bundle_adjust, refine_cameras
    c = cc.case(2, 3, 5, "h36m")
    P, X, Cm, D = _dev(c["points"]), _dev(c["pixels"]), _dev(c["cams0"]), _dev(c["dist"])

    def refused():
        for fn in (refine_cameras, bundle_adjust):
            for bad in (Cm[:2], Cm.float(), Cm.cpu(), Cm[:, :15]):
                with pytest.raises(RuntimeError, match="cams must be float64"):
                    fn(P, X, None, bad)
            for bad in (D[:2], D[:, :4], D.float(), D.cpu(), D.reshape(-1)):
                with pytest.raises(RuntimeError, match="distortion must"):
                    fn(P, X, None, Cm, distortion=bad)
            with pytest.raises(RuntimeError, match="no CPU path: conf must live on a GPU"):
                fn(P, X, torch.ones(2, 3, 5), Cm)
            with pytest.raises(NotImplementedError, match="at most 32 views, 64 joints"):
                fn(torch.zeros(1, 65, 3, device="cuda"), torch.zeros(1, 2, 65, 2, device="cuda"), None, Cm[:2])
            for bad in ((3,), (-1,), (0.0,)):
                with pytest.raises(RuntimeError, match="fixed holds view indices"):
                    fn(P, X, None, Cm, fixed=bad)
            with pytest.raises(RuntimeError, match="huber must be"):
                fn(P, X, None, Cm, huber=0.0)
        for bad in (-1, float("nan"), None, "2"):
            with pytest.raises(RuntimeError, match="rounds must be"):
                bundle_adjust(P, X, None, Cm, rounds=bad)

    _, n = _launches(refused)
    assert n == 0
    assert C.sizeof(C.c_int) == 4 and C.sizeof(C.c_uint) == 4      # out_used, out_iterations and fixed_mask on both sides


# --------------------------------------------------------------------------------------------------------------- bundle_adjust
def test_bundle_adjust_launches_and_rounds_zero():
    from openmpl_amd import bundle_adjust
    c = cc.case(6, 3, 17, "per_view", conf="uniform")
    x0 = rc.linear_points(c["pixels"], c["conf"], c["cams0"], c["dist"]).astype(np.float32)
    P, X, Cf, Cm, D = _dev(x0), _dev(c["pixels"]), _dev(c["conf"]), _dev(c["cams0"]), _dev(c["dist"])
    for rounds, huber in ((3, None), (2, 6.0), (1, None)):
        r, n = _launches(lambda: bundle_adjust(P, X, Cf, Cm, D, huber=huber, rounds=rounds))
        assert n == 2 * rounds + 1
        assert r.cost.shape == (rounds + 1,) and r.cost.dtype == torch.float64 and r.cost.is_cuda
        cost = r.cost.cpu().numpy()
        ref = cc.bundle_adjust(x0, c["pixels"], c["conf"], c["cams0"], c["dist"], huber, rounds)
        print("rounds %d huber %s: cost %s (restated %s)" % (rounds, huber, cost, ref["cost"]))
        assert cost[-1] < cost[0] and (cost[1:] <= cost[:-1] + ref["slack"] * 2).all()
        np.testing.assert_allclose(cost, ref["cost"], rtol=1e-4)                 # fp32 points on both sides, see DESIGN.md section 2
        assert r.points.dtype == torch.float32 and r.cams.dtype == torch.float64
        assert r.cameras.cams is r.cams and r.refined.points is r.points
        assert torch.equal(r.cost[rounds - 1], r.cameras.cost0.sum())
    z, n = _launches(lambda: bundle_adjust(P, X, Cf, Cm, D, rounds=0))
    assert n == 1 and z.cameras is None and z.refined is None and z.cost.shape == (1,)
    assert torch.equal(z.points.view(torch.int32), P.view(torch.int32)) and torch.equal(z.cams.view(torch.int64), Cm.view(torch.int64))
    np.testing.assert_allclose(z.cost.cpu().numpy(), cc.cost(x0, c["pixels"], c["conf"], c["cams0"], c["dist"]).sum()[None], rtol=RTOL)


def test_closed_loop_from_triangulation_under_a_perturbed_rig():
    """(64,4,17), H36M-like lens, 2 px of noise; cameras 2 and 3 turned by 2 degrees and moved by 0.05 units, cameras 0 and 1 exact and
    fixed.  triangulate_pixels under the perturbed rig -> bundle_adjust(rounds=8): the device's mean point error is at most 1.05 x
    the restatement's (the same algorithm in fp64; the differences are the fp32 rounding of the points and the summation order)."""
    from openmpl_amd import bundle_adjust, triangulate_pixels
    c, cams0 = cc.closed_loop_case()
    X, Cm, D = _dev(c["pixels"]), _dev(cams0), _dev(c["dist"])
    lin, _, _ = triangulate_pixels(X, None, Cm, rc.WH, distortion=D)
    r, n = _launches(lambda: bundle_adjust(lin, X, None, Cm, D, rounds=8, fixed=(0, 1)))
    assert n == 17
    lin64 = rc.linear_points(c["pixels"], None, cams0, c["dist"]).astype(np.float32)
    ref = cc.bundle_adjust(lin64, c["pixels"], None, cams0, c["dist"], None, 8, (0, 1))
    e0, e1 = rc.mean_error(lin.cpu().numpy(), c["truth"])[0], rc.mean_error(r.points.cpu().numpy(), c["truth"])[0]
    e0_ref, e1_ref = rc.mean_error(lin64, c["truth"])[0], rc.mean_error(ref["points"], c["truth"])[0]
    cost = r.cost.cpu().numpy()
    print("closed loop on the device: mean point error %.5f -> %.5f (x %.3f); restated %.5f -> %.5f; RMS %.2f -> %.2f px"
          % (e0, e1, e1 / e0, e0_ref, e1_ref, np.sqrt(cost[0] / 4352), np.sqrt(cost[-1] / 4352)))
    assert e1 <= 1.05 * e1_ref and e1_ref < 0.15 * e0_ref
    assert cost[-1] < cost[0] and (cost[1:] <= cost[:-1] + 2 * ref["slack"]).all()
    assert torch.equal(r.cams[:2].view(torch.int64), Cm[:2].view(torch.int64)) and bool((r.cameras.status[:2] == 2).all())
    assert bool((r.cameras.status[2:] == 0).all()) and bool((r.refined.status == 0).all())
