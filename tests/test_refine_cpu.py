"""Reprojection-error refinement (csrc/refine.hip) without a GPU: the float64 restatement of tests/refine_cases.py -- its Jacobian,
its Levenberg-Marquardt loop and what the refinement buys --, the new C prototype against its binding and its refusals, and the
argument checks of the Python surface, which are raised before any device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from openmpl_amd import cabi
from tests import distortion_cases as dc
from tests import refine_cases as rc

HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mpl_hip.h")).read()


# ----------------------------------------------------------------------------------------------------------------- the boundary
def test_exported_bound_and_declared():
    import openmpl_amd
    from openmpl_amd import geometry
    lib = cabi.load()
    assert "mpl_refine_points" in cabi.EXPORTS and hasattr(lib, "mpl_refine_points")
    assert re.search(r"#define MPL_HIP_ABI_VERSION 14\b", HEADER) and cabi.ABI_VERSION == 14 and lib.mpl_hip_abi_version() == 14
    m = re.search(r"\bint mpl_refine_points\(([^;]*)\);", HEADER)
    assert m, "mpl_refine_points is not declared in include/mpl_hip.h"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    want = ["const float *points", "const float *pixels", "const float *conf", "const double *cams_dev", "const double *dist_dev",
            "int batch", "int views", "int joints", "double huber", "int max_iterations", "double step_tolerance", "float *out_points",
            "float *out_error", "float *out_errors", "int *out_iterations", "unsigned char *out_status", "void *stream"]
    assert params == want
    ctype = lambda p: cabi._fp if "*" in p else {"int": C.c_int, "double": C.c_double}[p.rsplit(" ", 1)[0]]      # noqa: E731
    assert [ctype(p) for p in params] == list(lib.mpl_refine_points.argtypes) and lib.mpl_refine_points.restype is C.c_int
    assert "refine.hip" in __import__("openmpl_amd.build", fromlist=["SOURCES"]).SOURCES
    assert openmpl_amd.refine_points is geometry.refine_points and openmpl_amd.reprojection_errors is geometry.reprojection_errors
    assert geometry.Refined._fields == ("points", "error", "errors", "iterations", "status")


def test_c_abi_refusals_need_no_device():
    lib = cabi.load()
    p = lambda a: None if a is None else C.c_void_p(a)            # never dereferenced by a refused call      # noqa: E731

    def call(points=8, pixels=8, conf=8, cams=8, dist=8, B=2, V=3, J=17, huber=0.0, it=20, tol=1e-8, out=8, err=8):
        return lib.mpl_refine_points(p(points), p(pixels), p(conf), p(cams), p(dist), B, V, J, huber, it, tol, p(out), p(err), None, None,
                                     None, None)
    assert call(points=None) == -1 and call(pixels=None) == -1 and call(cams=None) == -1 and call(out=None) == -1 and call(err=None) == -1
    assert call(B=0) == -1 and call(V=0) == -1 and call(J=-1) == -1 and call(V=33) == -1 and call(J=65) == -1
    assert call(B=1 << 20, V=32, J=64) == -1                                                     # 2^31 observations
    assert call(it=-1) == -2 and call(it=1001) == -2
    assert call(tol=-1e-9) == -2 and call(tol=float("nan")) == -2 and call(tol=float("inf")) == -2
    assert call(points=None, it=-1) == -1                                                        # the pointers come first


# ------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", dc.SETS)
def test_analytic_jacobian_matches_central_differences(name):
    c = rc.case(3, 5, 17, name, noise=0.0, start="truth")
    X = c["points0"].astype(np.float64)
    Jm = rc.jacobian(X, c["cams"], c["dist"])
    h = 1e-6
    num = np.empty_like(Jm)
    for k in range(3):
        e = np.zeros(3)
        e[k] = h
        num[..., k] = (dc.project(X + e, c["cams"], c["dist"])[0] - dc.project(X - e, c["cams"], c["dist"])[0]) / (2 * h)
    # central differences of a smooth function: truncation h^2 f''' / 6 ~ 1e-9 px per unit, rounding eps |px| / h ~ 1e-7
    err = float(np.abs(Jm - num).max() / np.abs(num).max())
    print("%s: analytic against central differences, max-scaled %.2e (|J| up to %.0f px per unit)" % (name, err, np.abs(num).max()))
    assert err <= 1e-8
    if name != "zeros":        # the lens is in it: the pinhole Jacobian at the same points differs by more than the bound
        assert np.abs(Jm - rc.jacobian(X, c["cams"], dc.table("zeros", 5))).max() / np.abs(num).max() > 1e-4


@pytest.mark.parametrize("V", [1, 2, 4])
@pytest.mark.parametrize("name", ["zeros", "h36m", "per_view"])
def test_noise_free_input_is_a_fixed_point(V, name):
    c = rc.case(4, V, 17, name, noise=0.0, start="linear" if V >= 2 else "exact")     # one view has no linear point: the true one
    r = rc.refine(c["points0"], c["pixels"], None, c["cams"], c["dist"])
    print("%s V %d: trials up to %d, error up to %.2e px, status %s" % (name, V, r["iterations"].max(), np.nanmax(r["errors"]),
                                                                         np.unique(r["status"])))
    assert np.isin(r["status"], (0, 2)).all() and (r["status"] == (2 if V < 2 else 0)).all()
    assert r["iterations"].max() <= 2
    assert np.nanmax(r["errors"]) < 1e-3 and r["error"].max() < 1e-3
    if V < 2:
        assert np.array_equal(r["points"], c["points0"].astype(np.float64))


@pytest.mark.parametrize("huber", [None, 6.0])
@pytest.mark.parametrize("conf,outliers", [("none", 0), ("mixed", 0), ("uniform", 1)])
def test_cost_never_rises(huber, conf, outliers):
    c = rc.case(8, 4, 17, "per_view", conf=conf, outliers=outliers)
    r = rc.refine(c["points0"], c["pixels"], c["conf"], c["cams"], c["dist"], huber=huber)
    live = r["status"] < 3
    assert live.all() and (r["E"] <= r["E0"]).all() and (r["E"] < r["E0"]).any()
    # the cost the loop tracked is the cost of the point it returns, whichever mode
    np.testing.assert_array_equal(r["E"], rc.cost(r["points"], c["pixels"], c["conf"], c["cams"], c["dist"], huber))


def test_newton_step_vanishes_at_a_converged_point():
    c, r = rc.plain_case_converging(8, 4, 17, "h36m", conf="uniform")
    delta, zmin = rc.newton_step(r["points"], c["pixels"], c["conf"], c["cams"], c["dist"])
    rel = np.abs(delta).max(axis=-1) / zmin
    print("Newton step at the converged points: up to %.2e of the nearest depth" % rel.max())
    assert (r["status"] == 0).all() and (rel <= 1e-6).all()


def test_plain_refinement_is_no_worse_than_the_linear_point():
    lines = []
    for V in (2, 3, 4, 8):
        c = rc.case(64, V, 17, "h36m", seed=13)
        r = rc.refine(c["points0"], c["pixels"], None, c["cams"], c["dist"])
        e0, e1 = rc.mean_error(c["points0"], c["truth"])[0], rc.mean_error(r["points"], c["truth"])[0]
        ev = rc.evaluate(c["points0"], c["pixels"], None, c["cams"], c["dist"])
        rms0, rms1 = np.sqrt(ev["S"].sum() / ev["w"].sum()), np.sqrt(np.mean(r["error"] ** 2))
        lines.append("V %d: mean 3D error after / before %.3f (%.5f / %.5f), RMS reprojection %.2f -> %.2f px, trials mean %.1f max %d"
                     % (V, e1 / e0, e1, e0, rms0, rms1, r["iterations"].mean(), r["iterations"].max()))
        assert (r["status"] == 0).all() and (r["E"] <= r["E0"]).all()
        if V == 4:
            assert e1 <= e0
    print("\n".join(lines))


@pytest.mark.parametrize("V", [4, 8])
def test_huber_refinement_halves_the_error_under_one_displaced_view(V):
    c = rc.case(64, V, 17, "h36m", seed=13, outliers=1)
    r = rc.refine(c["points0"], c["pixels"], None, c["cams"], c["dist"], huber=6.0)
    (e0, m0), (e1, m1) = rc.mean_error(c["points0"], c["truth"]), rc.mean_error(r["points"], c["truth"])
    print("Huber 6 px, V %d, one view of every joint 40 .. 120 px off: mean 3D error %.4f -> %.4f (x %.3f), medians %.4f -> %.4f, "
          "trials mean %.1f max %d" % (V, e0, e1, e1 / e0, m0, m1, r["iterations"].mean(), r["iterations"].max()))
    assert e1 <= 0.5 * e0 and (r["E"] <= r["E0"]).all()
    # the plain cost from the same start does not get there: the displaced view keeps its full pull
    p = rc.refine(c["points0"], c["pixels"], None, c["cams"], c["dist"])
    assert rc.mean_error(p["points"], c["truth"])[0] > 2 * e1


def test_statuses_of_the_restatement():
    c = rc.case(2, 3, 5, "h36m")
    x0, px, cams, dist = c["points0"].copy(), c["pixels"].copy(), c["cams"], c["dist"]
    cf = np.ones((2, 3, 5), np.float32)
    x0[0, 0, 1] = np.nan                                   # a point that is not finite
    x0[0, 1] = cams[1, 13:16] - 2.0 * cams[1, 10:13]       # behind camera 1
    cf[0, :, 2] = 0.0                                      # no view takes part
    cf[0, 1:, 3] = (np.nan, -1.0)                          # one view left
    px[1, 0, 0] = np.inf                                   # a pixel that is not finite: two views left
    r = rc.refine(x0, px, cf, cams, dist)
    assert list(r["status"][0]) == [3, 3, 3, 2, 0] and (r["status"][1] == 0).all()
    assert np.isnan(r["points"][0, :3]).all() and np.isnan(r["error"][0, :3]).all() and np.isnan(r["errors"][0, :, :3]).all()
    assert np.array_equal(r["points"][0, 3], x0[0, 3].astype(np.float64)) and r["iterations"][0, 3] == 0
    assert np.isfinite(r["errors"][0, 0, 3]) and np.isnan(r["errors"][0, 1:, 3]).all() and r["error"][0, 3] == r["errors"][0, 0, 3]
    assert np.isnan(r["errors"][1, 0, 0]) and np.isfinite(r["errors"][1, 1:, 0]).all()
    z = rc.refine(x0, px, cf, cams, dist, max_iterations=0)
    assert list(z["status"][0]) == [3, 3, 3, 2, 2] and (z["iterations"] == 0).all()
    assert np.array_equal(z["points"][1], x0[1].astype(np.float64))


# ------------------------------------------------------------------------------------------------------- the Python surface
def test_argument_checks_raise_before_any_device_is_touched():
    from openmpl_amd import refine_points, reprojection_errors, triangulate_pixels
    B, V, J = 2, 3, 5
    P, X, Cf = torch.zeros(B, J, 3), torch.zeros(B, V, J, 2), torch.ones(B, V, J)
    Cm, D = torch.zeros(V, 16, dtype=torch.float64), torch.zeros(V, 5, dtype=torch.float64)
    # shapes first, each complaint naming its argument
    with pytest.raises(RuntimeError, match=r"pixels: expected shape \(B,V,J,2\)"):
        refine_points(P, X[..., :1], Cf, Cm)
    with pytest.raises(RuntimeError, match=r"points: expected shape \(2, 5, 3\)"):
        refine_points(P[:, :4], X, Cf, Cm)
    with pytest.raises(RuntimeError, match=r"conf: expected shape \(2, 3, 5\)"):
        refine_points(P, X, Cf[:, :2], Cm)
    with pytest.raises(RuntimeError, match="points must be a tensor"):
        refine_points(None, X, Cf, Cm)
    # then dtypes: a wrong shape is reported before a wrong dtype of an earlier argument
    with pytest.raises(RuntimeError, match=r"conf: expected shape"):
        refine_points(P.double(), X, Cf[:, :2], Cm)
    with pytest.raises(RuntimeError, match=r"float32 tensors required \(points is torch.float64\)"):
        refine_points(P.double(), X, Cf, Cm)
    with pytest.raises(RuntimeError, match=r"float32 tensors required \(conf is torch.float16\)"):
        reprojection_errors(P, X, Cf.half(), Cm)
    # then devices
    with pytest.raises(RuntimeError, match="no CPU path: points must live on a GPU"):
        refine_points(P, X, Cf, Cm)
    with pytest.raises(RuntimeError, match="no CPU path: points must live on a GPU"):
        reprojection_errors(P, X, None, Cm, D)
    # the options
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="huber must be a positive finite number"):
            refine_points(P, X, Cf, Cm, huber=bad)
    for bad in (-1, 1001, 2.5):
        with pytest.raises(RuntimeError, match="max_iterations must be an integer"):
            refine_points(P, X, Cf, Cm, max_iterations=bad)
    for bad in (-1e-9, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="step_tolerance must be a finite number"):
            refine_points(P, X, Cf, Cm, step_tolerance=bad)
    with pytest.raises(RuntimeError, match="huber is an option of the refinement"):
        triangulate_pixels(X, Cf, Cm, huber=6.0)

