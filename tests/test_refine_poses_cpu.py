"""Whole-pose refinement under bone-length constraints (csrc/refine_poses.hip) without a GPU: the float64 restatement of
tests/refine_poses_cases.py -- its gradient, its tree solve, its monotonicity, what it buys --, the C prototype against its binding
and its refusals, and the argument checks of the Python surface, which are raised before any device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from openmpl_amd import cabi
from tests import distortion_cases as dc
from tests import refine_cases as rc
from tests import refine_poses_cases as pc

HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mpl_hip.h")).read()


# ----------------------------------------------------------------------------------------------------------------- the boundary
def test_exported_bound_and_declared():
    import openmpl_amd
    from openmpl_amd import geometry, rpsm
    lib = cabi.load()
    assert "mpl_refine_poses" in cabi.EXPORTS and hasattr(lib, "mpl_refine_poses")
    assert re.search(r"#define MPL_HIP_ABI_VERSION 14\b", HEADER) and cabi.ABI_VERSION == 14 and lib.mpl_hip_abi_version() == 14
    m = re.search(r"\bint mpl_refine_poses\(([^;]*)\);", HEADER)
    assert m, "mpl_refine_poses is not declared in include/mpl_hip.h"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    want = ["const float *points", "const float *pixels", "const float *conf", "const double *cams_dev", "const double *dist_dev",
            "const float *limb", "long long limb_stride", "const int *parents", "int batch", "int views", "int joints", "double huber",
            "double bone_weight", "int max_iterations", "double step_tolerance", "float *out_points", "float *out_error",
            "float *out_bone_error", "double *out_cost0", "double *out_cost", "int *out_iterations", "unsigned char *out_status",
            "void *stream"]
    assert params == want

    def ctype(p):
        if p == "const int *parents":                      # a host array
            return C.POINTER(C.c_int)
        return cabi._fp if "*" in p else {"int": C.c_int, "double": C.c_double, "long long": C.c_longlong}[p.rsplit(" ", 1)[0]]
    assert [ctype(p) for p in params] == list(lib.mpl_refine_poses.argtypes) and lib.mpl_refine_poses.restype is C.c_int
    assert "refine_poses.hip" in __import__("openmpl_amd.build", fromlist=["SOURCES"]).SOURCES
    assert openmpl_amd.refine_poses is geometry.refine_poses and openmpl_amd.bone_lengths is geometry.bone_lengths
    assert geometry.PosesRefined._fields == ("points", "error", "bone_error", "cost0", "cost", "iterations", "status")
    assert tuple(pc.HUMAN) == tuple(rpsm.HUMAN_BODY_PARENTS)


def test_c_abi_refusals_need_no_device():
    lib = cabi.load()
    p = lambda a: None if a is None else C.c_void_p(a)            # never dereferenced by a refused call      # noqa: E731
    human = list(pc.HUMAN)
    tree = lambda q: None if q is None else (C.c_int * len(q))(*q)      # noqa: E731

    def call(points=8, pixels=8, cams=8, limb=8, stride=0, parents=human, B=2, V=3, J=17, bw=1e4, it=20, tol=1e-8, out=8, err=8):
        return lib.mpl_refine_poses(p(points), p(pixels), None, p(cams), None, p(limb), stride, tree(parents), B, V, J, 0.0, bw, it, tol,
                                    p(out), p(err), None, None, None, None, None, None)
    assert call(points=None) == -1 and call(pixels=None) == -1 and call(cams=None) == -1 and call(out=None) == -1 and call(err=None) == -1
    assert call(limb=None) == -1 and call(parents=None) == -1
    assert call(B=0) == -1 and call(V=0) == -1 and call(J=0) == -1 and call(V=33) == -1 and call(J=65, parents=pc.tree("chain", 65)) == -1
    assert call(B=1 << 20, V=32, J=64, parents=pc.tree("chain", 64)) == -1                       # 2^31 observations
    assert call(stride=16) == -1 and call(stride=-1) == -1 and call(stride=1) == -1              # neither 0 nor >= joints
    assert call(it=-1) == -2 and call(it=1001) == -2
    assert call(tol=-1e-9) == -2 and call(tol=float("nan")) == -2 and call(tol=float("inf")) == -2
    assert call(bw=-1e-9) == -2 and call(bw=float("nan")) == -2 and call(bw=float("inf")) == -2
    assert call(limb=None, it=-1) == -1                                                          # the pointers come first
    bad = []
    for j, q in ((5, -1), (0, 3), (4, 4), (6, 17), (6, -2)):                   # two roots, none (a cycle), itself, out of range twice
        t = list(human)
        t[j] = q
        bad.append(t)
    cyc = list(human)
    cyc[1], cyc[2] = 2, 1                                                      # a cycle beside the root's component
    for t in bad + [cyc]:
        assert call(parents=t) == -1, t
    assert call(J=1, parents=[0]) == -1 and call(J=2, parents=[-1, -1]) == -1


# ------------------------------------------------------------------------------------------------------- the Python surface
def test_argument_checks_raise_before_any_device_is_touched():
    from openmpl_amd import bone_lengths, refine_poses
    B, V, J = 2, 3, 17
    P, X, Cf, L = torch.zeros(B, J, 3), torch.zeros(B, V, J, 2), torch.ones(B, V, J), torch.ones(J)
    Cm, D = torch.zeros(V, 16, dtype=torch.float64), torch.zeros(V, 5, dtype=torch.float64)
    with pytest.raises(RuntimeError, match=r"pixels: expected shape \(B,V,J,2\)"):
        refine_poses(P, X[..., :1], Cf, Cm, L)
    with pytest.raises(RuntimeError, match=r"points: expected shape \(2, 17, 3\)"):
        refine_poses(P[:, :4], X, Cf, Cm, L)
    with pytest.raises(RuntimeError, match=r"conf: expected shape \(2, 3, 17\)"):
        refine_poses(P, X, Cf[:, :2], Cm, L)
    with pytest.raises(RuntimeError, match=r"float32 tensors required \(points is torch.float64\)"):
        refine_poses(P.double(), X, Cf, Cm, L)
    with pytest.raises(RuntimeError, match="no CPU path: points must live on a GPU"):
        refine_poses(P, X, Cf, Cm, L, distortion=D)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="huber must be a positive finite number"):
            refine_poses(P, X, Cf, Cm, L, huber=bad)
    for bad in (-1, 1001, 2.5):
        with pytest.raises(RuntimeError, match="max_iterations must be an integer"):
            refine_poses(P, X, Cf, Cm, L, max_iterations=bad)
    for bad in (-1e-9, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="step_tolerance must be a finite number"):
            refine_poses(P, X, Cf, Cm, L, step_tolerance=bad)
    for bad in (-1e-9, float("nan"), float("inf"), None, "x"):
        with pytest.raises(RuntimeError, match="bone_weight must be a finite number >= 0"):
            refine_poses(P, X, Cf, Cm, L, bone_weight=bad)
    for bad in (torch.ones(J - 1), torch.ones(B + 1, J), torch.ones(B, J, 1), None, [1.0] * J):
        with pytest.raises(RuntimeError, match=r"limb_length: expected a tensor of shape \(17,\) or \(2, 17\)"):
            refine_poses(P, X, Cf, Cm, bad)
    with pytest.raises(RuntimeError, match=r"float32 tensors required \(limb_length is torch.float64\)"):
        refine_poses(P, X, Cf, Cm, L.double())
    with pytest.raises(RuntimeError, match="no CPU path"):                         # good lengths of both forms get as far as the devices
        refine_poses(P, X, Cf, Cm, torch.ones(B, J))
    # the tree: the checks and the messages of rpsm
    human = list(pc.HUMAN)
    with pytest.raises(ValueError, match="exactly one root"):
        refine_poses(P, X, Cf, Cm, L, parents=[-1, -1] + human[2:])
    with pytest.raises(ValueError, match="exactly one root"):
        refine_poses(P, X, Cf, Cm, L, parents=[1] + human[1:])
    with pytest.raises(ValueError, match="is no joint of 0..16"):
        refine_poses(P, X, Cf, Cm, L, parents=human[:16] + [17])
    with pytest.raises(ValueError, match="is no joint of 0..16"):
        refine_poses(P, X, Cf, Cm, L, parents=human[:16] + [16])
    with pytest.raises(ValueError, match="has a cycle"):
        refine_poses(P, X, Cf, Cm, L, parents=[-1, 2, 1] + human[3:])
    with pytest.raises(ValueError, match="parents has 16 entries, the points 17 joints"):
        refine_poses(P, X, Cf, Cm, L, parents=human[:16])
    with pytest.raises(ValueError, match="the default tree has 17 joints, the points 5: pass parents"):
        refine_poses(P[:, :5], X[:, :, :5], Cf[:, :, :5], Cm, L[:5])
    with pytest.raises(ValueError, match="the default tree has 17 joints"):
        bone_lengths(P[:, :5])
    with pytest.raises(RuntimeError, match=r"points: expected a tensor of shape \(B,J,3\)"):
        bone_lengths(P[0])
    # a good tree gets as far as the devices
    with pytest.raises(RuntimeError, match="no CPU path"):
        refine_poses(P[:, :5], X[:, :, :5], Cf[:, :, :5], Cm, L[:5], parents=[-1, 0, 1, 2, 3])


def test_bone_lengths_is_the_restatements():
    from openmpl_amd import bone_lengths
    c = pc.case(4, 2, 17)
    x = c["truth"].copy()
    x[1, 9] = np.nan                                        # its own bone and that of its child
    got = bone_lengths(torch.from_numpy(x)).numpy()
    want = pc.bone_lengths(x.astype(np.float64), pc.HUMAN)
    assert got.dtype == np.float32 and got.shape == (4, 17) and (got[:, 0] == 0).all()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got[1, [9, 10]]).all() and np.isnan(got).sum() == 2
    np.testing.assert_allclose(got[~np.isnan(got)], want[~np.isnan(want)], rtol=1e-6)
    chain = bone_lengths(torch.from_numpy(x[:, :5]), parents=pc.tree("chain", 5)).numpy()
    np.testing.assert_allclose(chain[:, 1:], np.linalg.norm(x[:, 1:5] - x[:, :4], axis=-1), rtol=1e-6)
    # the median over a sequence is what feeds limb_length
    med = bone_lengths(torch.from_numpy(x)).nanmedian(0).values
    assert med.shape == (17,) and bool(torch.isfinite(med).all())


# ------------------------------------------------------------------------------------------------------------- the restatement
def _eval(c, X, huber=None, limb=None, bone_weight=pc.BONE_WEIGHT):
    L = c["limb"] if limb is None else limb
    P = pc.participation(c["points0"], c["pixels"], c["conf"], L, c["parents"])
    return P, pc.evaluate(X, c["pixels"], c["cams"], c["dist"], huber, P, L, c["parents"], bone_weight)


@pytest.mark.parametrize("name", dc.SETS)
def test_gradient_matches_central_differences(name):
    """E = sum of squares, so dE / dX = 2 g (plain) and, beyond the Huber corner, 2 g with the IRLS weights as well"""
    c = pc.case(2, 3, 17, name=name, conf="uniform", limb_error=0.05)
    X = c["points0"].astype(np.float64)
    for huber in (None, 2.5):
        _, ev = _eval(c, X, huber)
        h = 1e-6
        num = np.empty_like(ev["g"])
        for j in range(17):
            for k in range(3):
                e = np.zeros_like(X)
                e[:, j, k] = h
                num[:, j, k] = (_eval(c, X + e, huber)[1]["E"] - _eval(c, X - e, huber)[1]["E"]) / (2 * h)
        err = float(np.abs(2.0 * ev["g"] - num).max() / np.abs(num).max())
        print("%s huber=%s: analytic against central differences, max-scaled %.2e (|dE| up to %.0f)" % (name, huber, err, np.abs(num).max()))
        assert err <= 1e-6
    # both terms are in it
    _, no_bones = _eval(c, X, bone_weight=0.0)
    assert np.abs(ev["g"] - no_bones["g"]).max() > 1e-3 * np.abs(ev["g"]).max() and np.abs(no_bones["g"]).max() > 0


@pytest.mark.parametrize("kind,J", [("human", 17), ("chain", 64), ("star", 64), ("random", 64)])
def test_tree_solve_is_the_dense_solve(kind, J):
    c = pc.case(3, 3, J, kind, conf="mixed", limb_error=0.03)
    cf = c["conf"].copy()
    cf[0, 1:, J - 1] = 0.0                                 # a joint held by its bone alone
    cf[1, :, J // 2] = 0.0                                 # a joint that takes no part, its bones dropped
    c["conf"] = cf
    P, ev = _eval(c, c["points0"].astype(np.float64))
    assert not P["joint"][1, J // 2] and P["joint"][0, J - 1] and P["live"].sum() >= 3 * (J - 1) - 4
    for lam in (1e-3, 1e-9, 10.0):
        lams = np.full(3, lam)
        A, rhs = pc.dense_system(ev, lams, P, c["parents"])
        assert np.abs(A - np.transpose(A, (0, 2, 1))).max() <= 1e-12 * np.abs(A).max()
        dense = np.linalg.solve(A, rhs[..., None])[..., 0].reshape(3, J, 3)
        got = pc.tree_solve(ev, lams, P, c["parents"])
        err = float(np.abs(got - dense).max() / np.abs(dense).max())
        print("%s J=%d lambda=%g: tree solve against numpy.linalg.solve, %.2e relative" % (kind, J, lam, err))
        assert err <= 1e-10 and (got[1, J // 2] == 0).all()
    # a pivot that is not positive gives a step that is not a number
    assert np.isnan(pc.solve3(np.diag([1.0, 0.0, 1.0]), np.ones(3))).all() and np.isnan(pc.solve3(-np.eye(3), np.ones(3))).all()
    np.testing.assert_allclose(pc.solve3(np.diag([1.0, 2.0, 4.0]), np.ones(3)), [1.0, 0.5, 0.25])


def test_participation_rules():
    c = pc.case(1, 3, 17, conf="uniform")
    x0, cf, L = c["points0"].copy(), c["conf"].copy(), c["limb"].copy()
    cf[0, 1:, 3] = 0.0               # a leaf seen once, held by its bone
    cf[0, :, 6] = 0.0                # a leaf no view sees: out, its bone dead
    cf[0, 1:, 10] = 0.0              # a leaf seen once ...
    L[0, 10] = np.nan                # ... whose length is not known: out
    cf[0, 1:, 12] = 0.0              # an inner joint seen once whose own length is unknown, held by its child's bone
    L[0, 12] = -1.0
    x0[0, 15, 2] = np.inf            # a point that is not finite: out, and the bone of its child dead, which two views still hold
    P = pc.participation(x0, c["pixels"], cf, L, c["parents"])
    out = np.zeros(17, bool)
    out[[6, 10, 15]] = True
    dead = np.zeros(17, bool)
    dead[[0, 6, 10, 12, 15, 16]] = True
    assert np.array_equal(~P["joint"][0], out) and np.array_equal(~P["live"][0], dead)
    assert not P["view"][0, :, out].any() and P["view"][0, :, 3].sum() == 1 and P["view"][0, :, 16].sum() == 3
    r = pc.refine(x0, c["pixels"], cf, c["cams"], L, c["parents"], c["dist"])
    assert r["status"][0] == 0 and np.array_equal(r["points"][0, out].astype(np.float32).view(np.uint32), x0[0, out].view(np.uint32))
    assert np.isnan(r["error"][0, out]).all() and np.isfinite(r["error"][0, ~out]).all()
    assert np.array_equal(np.isnan(r["bone_error"][0]), dead)
    # a pose one joint of which is behind a camera that takes part: every output NaN
    x1 = c["points0"].copy()
    x1[0, 5] = (c["cams"][1, 13:16] - 2.0 * c["cams"][1, 10:13]).astype(np.float32)
    r = pc.refine(x1, c["pixels"], c["conf"], c["cams"], c["limb"], c["parents"], c["dist"])
    assert r["status"][0] == 3 and all(np.isnan(r[k]).all() for k in ("points", "error", "bone_error", "cost0", "cost"))
    # nothing takes part: passed through, scored as nothing
    r = pc.refine(c["points0"], c["pixels"], np.zeros_like(c["conf"]), c["cams"], c["limb"], c["parents"], c["dist"])
    assert r["status"][0] == 2 and r["cost"][0] == 0.0 and np.isnan(r["error"]).all()
    assert np.array_equal(r["points"].astype(np.float32).view(np.uint32), c["points0"].view(np.uint32))


@pytest.mark.parametrize("huber", [None, 2.5])
def test_cost_never_rises(huber):
    for c in (pc.case(6, 2, 17, conf="mixed"), pc.case(3, 3, 64, "random", conf="uniform", limb="shared"), pc.occlusion_case(B=6)[0],
              pc.case(4, 1, 17, start="truth")):                    # the last: one camera, which stays underdetermined
        r = pc.run(c, huber=huber, max_iterations=30)
        assert (r["cost"] <= r["cost0"]).all() and (r["status"] < 2).all() and (r["cost"] < r["cost0"]).any()
        # the cost the loop tracked is the cost of the pose it returns
        E = pc.cost(r["points"], c["pixels"], c["conf"], c["cams"], c["dist"], huber, c["limb"], c["parents"], given=c["points0"])
        np.testing.assert_allclose(E, r["cost"], rtol=1e-12)
        np.testing.assert_array_equal(r["cost0"], pc.cost(c["points0"], c["pixels"], c["conf"], c["cams"], c["dist"], huber, c["limb"], c["parents"]))
        z = pc.run(c, huber=huber, max_iterations=0)
        assert (z["status"] == 2).all() and np.array_equal(z["cost"], z["cost0"]) and np.array_equal(z["cost0"], r["cost0"])


def test_without_bone_weight_it_is_refine_points():
    c = pc.case(6, 3, 17, conf="uniform")
    r = pc.run(c, bone_weight=0.0)
    q = rc.refine(c["points0"], c["pixels"], c["conf"], c["cams"], c["dist"], None, 50, 1e-8)
    assert (r["status"] == 0).all() and (q["status"] == 0).all() and r["joint"].all()
    d = np.abs(r["points"] - q["points"]).max(axis=(1, 2))
    print("bone_weight=0 against refine_points: max |d| %.2e units, bound %.2e" % (d.max(), (10 * 1e-8 * r["zmin"]).min()))
    assert (d <= 10 * 1e-8 * r["zmin"]).all()
    np.testing.assert_allclose(r["error"], q["error"], rtol=1e-6)
    np.testing.assert_allclose(r["cost"], q["E"].sum(axis=1), rtol=1e-9)


# ----------------------------------------------------------------------------------------------------------------- what it buys
def test_two_views_gain_from_the_bones():
    c, ref, pts = pc.two_view_loop()
    e_pose, e_pts = pc.joint_errors(ref["points"], c["truth"]).mean(), pc.joint_errors(pts["points"], c["truth"]).mean()
    print("(32,2,17): refine_points %.5f, whole-pose refinement %.5f (x %.3f), at most %d trials"
          % (e_pts, e_pose, e_pose / e_pts, ref["iterations"].max()))
    assert e_pose <= 0.75 * e_pts and (ref["cost"] <= ref["cost0"]).all()


def test_four_views_lose_nothing():
    c, ref, pts = pc.four_view_loop()
    e_pose, e_pts = pc.joint_errors(ref["points"], c["truth"]).mean(), pc.joint_errors(pts["points"], c["truth"]).mean()
    print("(32,4,17): refine_points %.5f, whole-pose refinement %.5f (x %.3f)" % (e_pts, e_pose, e_pose / e_pts))
    assert e_pose <= e_pts


def test_occluded_joints_come_back():
    c, one, ref = pc.occlusion_loop()
    e0, e1 = pc.joint_errors(c["points0"], c["truth"]), pc.joint_errors(ref["points"], c["truth"])
    leaf = ~np.isin(np.arange(17), c["parents"])[None, :] & np.ones_like(one)
    print("occlusion (32,4,17), %d one-view joints: %.4f -> %.4f (x %.3f); inner %.4f, leaves %.4f; fully seen %.4f"
          % (one.sum(), e0[one].mean(), e1[one].mean(), e1[one].mean() / e0[one].mean(), e1[one & ~leaf].mean(), e1[one & leaf].mean(),
             e1[~one].mean()))
    assert ref["joint"].all() and 0.2 < one.mean() < 0.4
    assert e1[one].mean() <= 0.5 * e0[one].mean()
    assert (ref["cost"] <= ref["cost0"]).all()
