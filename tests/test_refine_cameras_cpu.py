"""Camera-pose refinement and alternating bundle adjustment (csrc/refine_cameras.hip) without a GPU: the float64 restatement of
tests/refine_cameras_cases.py -- its 6-parameter Jacobian, its Levenberg-Marquardt loop, its statuses and what the alternation buys
--, the new C prototype against its binding and its refusals, and the argument checks of the Python surface, which are raised
before any device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from openmpl_amd import cabi
from tests import distortion_cases as dc
from tests import refine_cameras_cases as cc
from tests import refine_cases as rc

HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mpl_hip.h")).read()
NOISE = 2.0            # px per axis, the default of the cases


# ----------------------------------------------------------------------------------------------------------------- the boundary
def test_exported_bound_and_declared():
    import openmpl_amd
    from openmpl_amd import geometry
    lib = cabi.load()
    assert "mpl_refine_cameras" in cabi.EXPORTS and hasattr(lib, "mpl_refine_cameras")
    assert re.search(r"#define MPL_HIP_ABI_VERSION 14\b", HEADER) and cabi.ABI_VERSION == 14 and lib.mpl_hip_abi_version() == 14
    m = re.search(r"\bint mpl_refine_cameras\(([^;]*)\);", HEADER)
    assert m, "mpl_refine_cameras is not declared in include/mpl_hip.h"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    want = ["const float *points", "const float *pixels", "const float *conf", "const double *cams_dev", "const double *dist_dev",
            "int batch", "int views", "int joints", "double huber", "int max_iterations", "double step_tolerance", "unsigned fixed_mask",
            "double *out_cams", "double *out_error", "double *out_cost0", "double *out_cost", "int *out_used", "int *out_iterations",
            "unsigned char *out_status", "void *stream"]
    assert params == want
    ctype = lambda p: cabi._fp if "*" in p else {"int": C.c_int, "double": C.c_double, "unsigned": C.c_uint}[p.rsplit(" ", 1)[0]]      # noqa: E731
    assert [ctype(p) for p in params] == list(lib.mpl_refine_cameras.argtypes) and lib.mpl_refine_cameras.restype is C.c_int
    assert "refine_cameras.hip" in __import__("openmpl_amd.build", fromlist=["SOURCES"]).SOURCES
    assert openmpl_amd.refine_cameras is geometry.refine_cameras and openmpl_amd.bundle_adjust is geometry.bundle_adjust
    assert geometry.CamerasRefined._fields == ("cams", "error", "cost0", "cost", "used", "iterations", "status")
    assert geometry.BundleAdjusted._fields == ("points", "cams", "cost", "cameras", "refined")
    assert "similarity" in geometry.bundle_adjust.__doc__ and "scale free" in geometry.bundle_adjust.__doc__        # the gauge is stated


def test_c_abi_refusals_need_no_device():
    lib = cabi.load()
    p = lambda a: None if a is None else C.c_void_p(a)            # never dereferenced by a refused call      # noqa: E731

    def call(points=8, pixels=8, conf=8, cams=8, dist=8, B=2, V=3, J=17, huber=0.0, it=20, tol=1e-8, mask=0, out=8, err=8):
        return lib.mpl_refine_cameras(p(points), p(pixels), p(conf), p(cams), p(dist), B, V, J, huber, it, tol, mask, p(out), p(err), None,
                                      None, None, None, None, None)
    assert call(points=None) == -1 and call(pixels=None) == -1 and call(cams=None) == -1 and call(out=None) == -1 and call(err=None) == -1
    assert call(B=0) == -1 and call(V=0) == -1 and call(J=-1) == -1 and call(V=33) == -1 and call(J=65) == -1
    assert call(B=1 << 20, V=32, J=64) == -1                                                     # 2^31 observations
    assert call(it=-1) == -2 and call(it=1001) == -2
    assert call(tol=-1e-9) == -2 and call(tol=float("nan")) == -2 and call(tol=float("inf")) == -2
    assert call(points=None, it=-1) == -1                                                        # the pointers come first
    assert call(it=-1, mask=0xffffffff) == -2                                                    # any mask is a mask


# ------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", dc.SETS)
def test_pose_jacobian_matches_central_differences(name):
    c = cc.case(3, 5, 17, name, noise=0.0)
    X = c["points"].astype(np.float64)
    Jm = cc.jacobian(X, c["cams0"], c["dist"])
    h = 1e-6
    num = np.empty_like(Jm)
    for k in range(6):
        e = np.zeros(6)
        e[k] = h
        num[..., k] = (dc.project(X, cc.apply(c["cams0"], e), c["dist"])[0] - dc.project(X, cc.apply(c["cams0"], -e), c["dist"])[0]) / (2 * h)
    # central differences of a smooth function in fp64: truncation h^2 f''' / 6 ~ 1e-10 of the scale, rounding eps |px| / h ~ 1e-7 px
    # against |J| of 1e3 .. 1e4 px per radian or unit
    err = float(np.abs(Jm - num).max() / np.abs(num).max())
    print("%s: analytic against central differences, max-scaled %.2e (|J| up to %.0f)" % (name, err, np.abs(num).max()))
    assert err <= 1e-8
    assert np.abs(Jm[..., :3]).max() > 100.0 and np.abs(Jm[..., 3:]).max() > 100.0       # both halves are there
    if name != "zeros":        # the lens is in it
        assert np.abs(Jm - cc.jacobian(X, c["cams0"], dc.table("zeros", 5))).max() / np.abs(num).max() > 1e-4


def test_apply_is_a_rotation_and_a_shift():
    rs = np.random.RandomState(3)
    c = cc.case(1, 4, 3)
    for scale in (1e-6, 1e-3, 0.3, 3.0):                   # across the series branch (|w|^2 < 1e-8) and beyond
        d = rs.randn(4, 6) * scale
        out = cc.apply(c["cams"], d)
        assert cc.rotation_error(out) <= 1e-14
        assert np.array_equal(out[:, :4], c["cams"][:, :4]) and np.allclose(out[:, 13:] - c["cams"][:, 13:], d[:, 3:], atol=1e-15)
        back = cc.apply(out, -np.concatenate([d[:, :3], d[:, 3:]], axis=1))
        assert np.abs(back - c["cams"]).max() <= 1e-14 * max(1.0, scale)
    # the two branches agree where they meet
    w = np.array([1e-4 / np.sqrt(3)] * 3)
    assert np.abs(cc.rodrigues(w * (1 - 1e-9)) - cc.rodrigues(w * (1 + 1e-9))).max() <= 1e-12


@pytest.mark.parametrize("name", ["zeros", "h36m", "per_view"])
def test_noise_free_rig_is_a_fixed_point(name):
    c = cc.case(4, 4, 17, name, noise=0.0, degrees=0.0, shift=0.0)
    # pixels in float64, not rounded: the float32 rounding of a pixel is itself 3e-5 px of noise, which moves a pose by 1e-7
    px = dc.project(c["points"], c["cams"], c["dist"])[0]
    r = cc.refine(c["points"], px, None, c["cams"], c["dist"])
    moved = float(np.abs(r["cams"] - c["cams"]).max())
    print("%s: trials %s, pose moved by %.1e, error up to %.1e px" % (name, r["iterations"], moved, r["error"].max()))
    assert (r["status"] == 0).all() and r["iterations"].max() <= 2 and moved <= 1e-12 and r["error"].max() <= 1e-9


@pytest.mark.parametrize("huber", [None, 6.0])
@pytest.mark.parametrize("conf,outliers", [("none", 0), ("uniform", 0), ("mixed", 0), ("uniform", 1)])
def test_cost_never_rises(huber, conf, outliers):
    c = rc.case(8, 4, 17, "per_view", conf=conf, outliers=outliers, start="exact")
    cams0 = cc.perturb(c["cams"], 2.0, 0.05, 11)
    r = cc.refine(c["truth"], c["pixels"], c["conf"], cams0, c["dist"], huber=huber)
    assert (r["status"] < 2).all() and (r["cost"] <= r["cost0"]).all() and (r["cost"] < r["cost0"]).all()
    # the cost the loop tracked is the cost of the pose it returns, whichever mode; and so is the error
    err, E = cc.score(c["truth"], c["pixels"], c["conf"], r["cams"], c["dist"], huber)
    np.testing.assert_array_equal(r["cost"], E)
    np.testing.assert_array_equal(r["error"], err)
    np.testing.assert_array_equal(r["cost0"], cc.cost(c["truth"], c["pixels"], c["conf"], cams0, c["dist"], huber))
    assert cc.rotation_error(r["cams"]) <= 1e-12


def test_recovery_from_five_degrees():
    c = cc.case(4, 4, 17, "h36m", degrees=5.0, shift=0.2)
    r = cc.refine(c["points"], c["pixels"], None, c["cams0"], c["dist"], None, 50)
    off0 = np.linalg.norm(c["cams0"][:, 13:] - c["cams"][:, 13:], axis=1)
    off = np.linalg.norm(r["cams"][:, 13:] - c["cams"][:, 13:], axis=1)
    rms0 = np.sqrt(r["cost0"] / r["used"])
    print("5 degrees / 0.2 units, 68 observations per view: trials %s, RMS %s -> %s px (per axis %s), centre off by %s -> %s"
          % (r["iterations"], np.round(rms0, 1), np.round(r["error"], 3), np.round(r["error"] / np.sqrt(2), 3), off0, np.round(off, 4)))
    assert (r["status"] == 0).all() and (r["iterations"] <= 20).all()
    # The final RMS, sqrt(E / N) of |r|, is below 1.5 x the noise level: asserted over the observations of the rig.  Per view the same
    # bound is not a property of the fit: |r| under NOISE px per axis has RMS NOISE sqrt(2) = 2.83 px, and 68 observations (136
    # residuals) spread a view's RMS by 1 / sqrt(2 * 136) = 6 %; at the TRUE camera view 1 of this case already stands at 3.15 px.  So
    # per view: no worse than the true camera (the fit minimises what `error` measures), and within k = 3 of those spreads
    pooled = float(np.sqrt(r["cost"].sum() / r["used"].sum()))
    at_truth = cc.score(c["points"], c["pixels"], None, c["cams"], c["dist"])[0]
    print("pooled RMS %.3f px; at the true cameras %s" % (pooled, np.round(at_truth, 3)))
    assert pooled < 1.5 * NOISE
    assert (r["error"] <= at_truth).all()
    assert (r["error"] < NOISE * np.sqrt(2.0) * (1.0 + 3.0 / np.sqrt(2.0 * 2.0 * 68.0))).all()
    assert (rms0 > 10 * NOISE).all() and (off < 0.25 * off0).all()


def test_statuses_of_the_restatement():
    c = cc.case(2, 5, 5, "h36m")
    X, px, cams = c["points"].copy(), c["pixels"].copy(), c["cams0"].copy()
    cf = np.ones((2, 5, 5), np.float32)
    cf[:, 1] = 0.0
    cf[0, 1, :2] = 1.0                                     # view 1: two observations
    cf[:, 2] = 0.0                                         # view 2: none
    X[1, 4] = cams[3, 13:16] - 2.0 * cams[3, 10:13]        # behind camera 3 ...
    cf[1, (0, 1, 2, 4), 4] = 0.0                           # ... and taking part only there
    r = cc.refine(X, px, cf, cams, c["dist"], fixed=(4,))
    assert list(r["status"]) == [0, 2, 3, 3, 2] and list(r["used"]) == [9, 2, 0, 10, 9]
    assert np.array_equal(r["cams"][1:], cams[1:]) and not np.array_equal(r["cams"][0], cams[0])
    assert np.isnan(r["error"][2:4]).all() and np.isnan(r["cost0"][2:4]).all() and np.isnan(r["cost"][2:4]).all()
    assert np.isfinite(r["error"][[0, 1, 4]]).all() and r["cost"][1] == r["cost0"][1] and r["cost"][4] == r["cost0"][4]
    assert r["cost"][0] < r["cost0"][0] and (r["iterations"][1:] == 0).all()
    z = cc.refine(X, px, cf, cams, c["dist"], max_iterations=0)
    assert list(z["status"]) == [2, 2, 3, 3, 2] and (z["iterations"] == 0).all() and np.array_equal(z["cams"], cams)
    np.testing.assert_array_equal(z["cost0"][[0, 1, 4]], r["cost0"][[0, 1, 4]])
    bad = cams.copy()
    bad[0, 7] = np.nan                                     # a record that is not finite
    n = cc.refine(X, px, cf, bad, c["dist"])
    assert n["status"][0] == 3 and np.array_equal(n["cams"][:4], bad[:4], equal_nan=True) and np.isnan(n["error"][0])
    # a NaN point drops out of every view and nothing else changes
    Xn = c["points"].copy()
    Xn[0, 0, 1] = np.nan
    a, b = cc.refine(Xn, px, None, cams, c["dist"]), cc.refine(c["points"], px, np.where(np.arange(10).reshape(2, 1, 5) == 0, 0, 1)
                                                              * np.ones((2, 5, 5), np.float32), cams, c["dist"])
    assert (a["used"] == 9).all() and np.array_equal(a["cams"], b["cams"])


# --------------------------------------------------------------------------------------------------------------- the alternation
@pytest.fixture(scope="module")
def closed_loop():
    c, cams0 = cc.closed_loop_case()
    lin = rc.linear_points(c["pixels"], None, cams0, c["dist"]).astype(np.float32)
    return c, cams0, lin, cc.bundle_adjust(lin, c["pixels"], None, cams0, c["dist"], None, 8, (0, 1))


def test_alternation_cost_does_not_rise(closed_loop):
    c, cams0, lin, ba = closed_loop
    cost, slack = ba["cost"], ba["slack"]
    print("total cost per round %s, float32 rounding slack up to %.2e" % (np.round(cost, 1), slack.max()))
    assert cost.shape == (9,) and (cost[1:] <= cost[:-1] + slack).all() and cost[-1] < 0.05 * cost[0]
    assert np.array_equal(ba["cams"][:2], cams0[:2]) and (ba["cameras"]["status"][:2] == 2).all()
    for huber in (None, 6.0):                              # and on a small case in both modes, no camera fixed
        s = cc.case(6, 3, 17, "per_view", conf="uniform")
        x0 = rc.linear_points(s["pixels"], s["conf"], s["cams0"], s["dist"]).astype(np.float32)
        b = cc.bundle_adjust(x0, s["pixels"], s["conf"], s["cams0"], s["dist"], huber, 3)
        assert (b["cost"][1:] <= b["cost"][:-1] + b["slack"]).all() and b["cost"][-1] < b["cost"][0]


def test_closed_loop_two_fixed_cameras_bring_the_points_back(closed_loop):
    c, cams0, lin, ba = closed_loop
    e_true = rc.mean_error(rc.linear_points(c["pixels"], None, c["cams"], c["dist"]), c["truth"])[0]
    e0, e1 = rc.mean_error(lin, c["truth"])[0], rc.mean_error(ba["points"], c["truth"])[0]
    rms = np.sqrt(ba["cost"] / c["pixels"][..., 0].size)
    print("closed loop (perturbation seed 5): mean point error %.4f under the perturbed rig -> %.4f after 8 rounds (x %.3f; %.4f under "
          "the true rig); RMS %.1f -> %.2f px" % (e0, e1, e1 / e0, e_true, rms[0], rms[-1]))
    assert e1 < 0.15 * e0


def test_one_fixed_camera_leaves_the_scale_free():
    """the gauge, as a fact: with one fixed camera the cost falls just as well as with two, but the points stay several times
    further from the truth"""
    c, _ = cc.closed_loop_case()
    c = {k: (v[:16] if k in ("pixels", "truth", "points0") else v) for k, v in c.items()}
    runs = {}
    for keep in ((0,), (0, 1)):
        cams1 = cc.perturb(c["cams"], 2.0, 0.05, 5, keep=keep)
        lin = rc.linear_points(c["pixels"], None, cams1, c["dist"]).astype(np.float32)
        ba = cc.bundle_adjust(lin, c["pixels"], None, cams1, c["dist"], None, 8, keep)
        runs[keep] = (ba["cost"], rc.mean_error(lin, c["truth"])[0], rc.mean_error(ba["points"], c["truth"])[0])
        print("fixed %s: cost %.0f -> %.0f, mean point error %.4f -> %.4f" % ((keep, ba["cost"][0], ba["cost"][-1]) + runs[keep][1:]))
    (cost1, _, e1), (cost2, _, e2) = runs[(0,)], runs[(0, 1)]
    assert cost1[-1] < 0.1 * cost1[0] and cost2[-1] < 0.1 * cost2[0] and cost1[-1] < 1.5 * cost2[-1]
    assert e1 > 3.0 * e2


# ------------------------------------------------------------------------------------------------------- the Python surface
def test_argument_checks_raise_before_any_device_is_touched():
    from openmpl_amd import bundle_adjust, refine_cameras
    B, V, J = 2, 3, 5
    P, X, Cf = torch.zeros(B, J, 3), torch.zeros(B, V, J, 2), torch.ones(B, V, J)
    Cm, D = torch.zeros(V, 16, dtype=torch.float64), torch.zeros(V, 5, dtype=torch.float64)
    for fn in (refine_cameras, bundle_adjust):
        # the checks of _observations: shapes first, then dtypes, then devices
        with pytest.raises(RuntimeError, match=r"pixels: expected shape \(B,V,J,2\)"):
            fn(P, X[..., :1], Cf, Cm)
        with pytest.raises(RuntimeError, match=r"points: expected shape \(2, 5, 3\)"):
            fn(P[:, :4], X, Cf, Cm)
        with pytest.raises(RuntimeError, match=r"conf: expected shape \(2, 3, 5\)"):
            fn(P, X, Cf[:, :2], Cm)
        with pytest.raises(RuntimeError, match="points must be a tensor"):
            fn(None, X, Cf, Cm)
        with pytest.raises(RuntimeError, match=r"float32 tensors required \(points is torch.float64\)"):
            fn(P.double(), X, Cf, Cm)
        with pytest.raises(RuntimeError, match="no CPU path: points must live on a GPU"):
            fn(P, X, Cf, Cm, D)
        # the options of refine_points
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(RuntimeError, match="huber must be a positive finite number"):
                fn(P, X, Cf, Cm, huber=bad)
        for bad in (-1, 1001, 2.5):
            with pytest.raises(RuntimeError, match="max_iterations must be an integer"):
                fn(P, X, Cf, Cm, max_iterations=bad)
        for bad in (-1e-9, float("nan"), float("inf")):
            with pytest.raises(RuntimeError, match="step_tolerance must be a finite number"):
                fn(P, X, Cf, Cm, step_tolerance=bad)
        # fixed: view indices in 0 .. V-1
        for bad in ((3,), (-1,), (0, 1.0), (True,), ("0",)):
            with pytest.raises(RuntimeError, match=r"fixed holds view indices, integers in \[0, 2\]"):
                fn(P, X, Cf, Cm, fixed=bad)
        with pytest.raises(RuntimeError, match="fixed must be a sequence"):
            fn(P, X, Cf, Cm, fixed=1)
        with pytest.raises(RuntimeError, match="no CPU path"):                     # a good `fixed` gets as far as the devices
            fn(P, X, Cf, Cm, fixed=[0, 2])
    for bad in (-1, 1.5, 1001, True, float("nan"), float("inf"), None, "2", [2]):
        with pytest.raises(RuntimeError, match="rounds must be an integer"):
            bundle_adjust(P, X, Cf, Cm, rounds=bad)
