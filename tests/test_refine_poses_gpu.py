"""Whole-pose refinement under bone-length constraints on the device (csrc/refine_poses.hip, openmpl_amd.geometry.refine_poses)
against the float64 restatement of tests/refine_poses_cases.py.

Parity is the rule of DESIGN.md section 2 (geometry_cases.rel_errors): max|d| <= 1e-4 max|ref| and norm-wise 1e-4, NaN in the same
places.  Trial counts are never compared: the device contracts multiply-adds and sums a pose in another order, and a trial whose
cost ties with the current one to the last bits may be accepted on one side only.  What does not depend on the restatement's
trajectory is checked beside it: the restatement's cost at the pose the device returns is no higher than at the pose it was given."""
import numpy as np
import pytest
import torch

from tests import geometry_cases as gc
from tests import refine_poses_cases as pc

pytestmark = pytest.mark.gpu

# two views; five poses; the joint limit on three trees (levels and children of every count); the view limit; the smallest pose
# with a bone; one joint seen once, which takes no part (passed through)
SHAPES = [(3, 2, 17, "human"), (5, 3, 17, "human"), (2, 4, 64, "random"), (2, 3, 64, "chain"), (2, 3, 64, "star"), (1, 32, 3, "chain"),
          (2, 2, 2, "chain"), (1, 1, 1, "human")]
TOL = 1e-4
HUBER = 2.5
COST0_TOL = 1e-10          # the same fp64 sum over at most 2112 terms from the same fp32 inputs
COST_TOL = 5.15e-13        # 10 x the worst value measured over the grid below on an MI355X, 5.15e-14


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


def _run(c, lens=True, **kw):
    """refine_poses on a case of refine_poses_cases -> (dict of numpy arrays, launches); points, pixels, conf, limb, parents of the
    case unless given"""
    from openmpl_amd import refine_poses
    get = lambda k, d: kw.pop(k) if k in kw else c[d]      # noqa: E731
    args = (_dev(get("points", "points0")), _dev(get("pixels", "pixels")), _dev(get("conf", "conf")), _dev(c["cams"]), _dev(get("limb", "limb")))
    parents = get("parents", "parents")
    D = _dev(c["dist"]) if lens else None
    r, n = _launches(lambda: refine_poses(*args, parents=parents, distortion=D, **kw))
    assert r.points.dtype == torch.float32 and r.error.dtype == torch.float32 and r.bone_error.dtype == torch.float32
    assert r.cost0.dtype == torch.float64 and r.cost.dtype == torch.float64 and r.iterations.dtype == torch.int32 and r.status.dtype == torch.uint8
    return {k: getattr(r, k).cpu().numpy() for k in r._fields}, n


def _assert_parity(got, ref, what):
    """-> the relative distance of the two final costs"""
    for k in ("points", "error", "bone_error"):
        m, nrm = gc.rel_errors(got[k], ref[k])
        print("%s %s: max-scaled %.2e, norm-wise %.2e" % (what, k, m, nrm))
        assert m <= TOL and nrm <= TOL, (what, k, m, nrm)
    assert np.array_equal(np.isnan(got["cost0"]), np.isnan(ref["cost0"])) and np.array_equal(np.isnan(got["cost"]), np.isnan(ref["cost"]))
    ok = ~np.isnan(ref["cost0"])
    scale = np.maximum(np.abs(ref["cost0"][ok]), 1e-300)
    d0 = float(np.max(np.abs(got["cost0"][ok] - ref["cost0"][ok]) / scale, initial=0.0))
    d1 = float(np.max(np.abs(got["cost"][ok] - ref["cost"][ok]) / np.maximum(np.abs(ref["cost"][ok]), 1e-300), initial=0.0))
    print("%s cost0: %.2e relative, cost: %.2e relative" % (what, d0, d1))
    assert d0 <= COST0_TOL and d1 <= COST_TOL, (what, d0, d1)
    assert (got["cost"][ok] <= got["cost0"][ok]).all(), what
    return d1


def _assert_cost_did_not_rise(got, c, huber, bone_weight, lens, what, points0=None, conf="case", limb=None):
    """the restatement's E at the device's fp32 pose against E at the given pose plus one fp32 rounding of every coordinate"""
    x0 = c["points0"] if points0 is None else points0
    cf = c["conf"] if isinstance(conf, str) else conf
    L = c["limb"] if limb is None else limb
    ok = got["status"] < 3
    X = np.where(ok[:, None, None], got["points"].astype(np.float64), x0.astype(np.float64))
    dist = c["dist"] if lens else None
    E = pc.cost(X, c["pixels"], cf, c["cams"], dist, huber, L, c["parents"], bone_weight, given=x0)
    E0 = pc.cost(x0, c["pixels"], cf, c["cams"], dist, huber, L, c["parents"], bone_weight)
    slack = pc.rounding_slack(X, c["pixels"], cf, c["cams"], dist, huber, L, c["parents"], bone_weight, given=x0)
    worst = float(np.max((E - E0)[ok], initial=-np.inf))
    print("%s: E(device pose) - E(given pose) at most %.3e px^2 (slack up to %.1e)" % (what, worst, float(np.max(slack[ok], initial=0.0))))
    assert (E[ok] <= E0[ok] + slack[ok]).all(), what


# --------------------------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("B,V,J,kind", SHAPES)
@pytest.mark.parametrize("name", ["h36m", None])
def test_refine_poses_matches_the_restatement(B, V, J, kind, name):
    worst = 0.0
    for conf in ("none", "uniform", "mixed"):
        for limb in ("pose", "shared"):
            for huber in (None, HUBER):
                c, ref, kw = pc.parity_case(B, V, J, kind, name or "zeros", conf, limb, huber)
                got, n = _run(c, lens=name is not None, **kw)
                what = "%s %s %s conf=%s limb=%s" % ((B, V, J, kind), name, "plain" if huber is None else "huber", conf, limb)
                assert n == 1, what
                assert got["points"].shape == (B, J, 3) and got["cost"].shape == (B,)
                worst = max(worst, _assert_parity(got, ref, what))
                if huber is None:                       # the builder asserted that these converge with room to spare
                    assert np.array_equal(got["status"], ref["status"]), what
                else:
                    assert np.array_equal(got["status"] >= 2, ref["status"] >= 2) and np.array_equal(got["status"][ref["status"] >= 2],
                                                                                                      ref["status"][ref["status"] >= 2]), what
                assert (got["iterations"][ref["status"] >= 2] == 0).all() and (got["iterations"] <= kw["max_iterations"]).all()
                _assert_cost_did_not_rise(got, c, huber, kw["bone_weight"], name is not None, what)
                if J > 1:
                    assert (ref["accepted"] > 0).any() and ref["live"].any() and (huber is not None or (ref["status"] == 0).all())
                else:
                    assert (got["status"] == 2).all() and np.array_equal(got["points"].view(np.uint32), c["points0"].view(np.uint32))
    print("%s %s: final cost off the restatement's by at most %.2e relative" % ((B, V, J, kind), name, worst))


# ------------------------------------------------------------------------------------------------------------- 2. bit for bit
def test_joints_that_take_no_part_and_zero_iterations_return_the_given_bits():
    B, V, J = 4, 3, 17
    c = pc.case(B, V, J, conf="uniform")
    x0, cf, L = c["points0"].copy(), c["conf"].copy(), c["limb"].copy()
    x0[0, 3, 1] = np.nan                                   # a NaN point: out, and its bone with it
    cf[1, :, 6] = 0.0                                      # a leaf no view sees
    cf[2, 1:, 16] = 0.0                                    # a leaf one view sees ...
    L[2, 16] = np.nan                                      # ... whose bone is switched off
    cf[3, 1:, 10] = 0.0                                    # a leaf one view sees, held by its bone: it takes part
    out = np.zeros((B, J), bool)
    out[0, 3] = out[1, 6] = out[2, 16] = True
    ref = pc.run(c, points=x0, conf=cf, limb=L)
    assert np.array_equal(~ref["joint"], out) and ref["joint"][3, 10] and (ref["status"] == 0).all()
    got, n = _run(c, points=x0, conf=cf, limb=L)
    assert n == 1 and np.array_equal(got["status"], ref["status"])
    assert np.array_equal(got["points"].view(np.uint32)[out], x0.view(np.uint32)[out]) and np.isnan(got["error"][out]).all()
    assert np.isfinite(got["error"][~out]).all() and not np.array_equal(got["points"][3, 10], x0[3, 10])
    assert np.isnan(got["bone_error"][0, 3]) and np.isnan(got["bone_error"][1, 6]) and np.isnan(got["bone_error"][2, 16])
    assert np.isnan(got["bone_error"][:, 0]).all() and np.isfinite(got["bone_error"][3, 1:]).all()
    _assert_parity(got, ref, "disturbed")
    _assert_cost_did_not_rise(got, c, None, pc.BONE_WEIGHT, True, "disturbed", points0=x0, conf=cf, limb=L)
    # max_iterations = 0: the given bits, everything scored
    zero, n = _run(c, points=x0, conf=cf, limb=L, max_iterations=0)
    zref = pc.run(c, points=x0, conf=cf, limb=L, max_iterations=0)
    assert n == 1 and (zero["status"] == 2).all() and (zero["iterations"] == 0).all()
    assert np.array_equal(zero["points"].view(np.uint32), x0.view(np.uint32)) and np.array_equal(zero["cost"], zero["cost0"])
    assert np.array_equal(zero["cost0"], got["cost0"])
    _assert_parity(zero, zref, "max_iterations=0")


def test_a_pose_behind_a_camera_is_invalid_and_alone():
    B, V, J = 3, 3, 17
    c = pc.case(B, V, J)
    base, _ = _run(c)
    x0 = c["points0"].copy()
    x0[1, 5] = (c["cams"][1, 13:16] - 2.0 * c["cams"][1, 10:13]).astype(np.float32)      # behind camera 1, which takes part
    got, n = _run(c, points=x0)
    ref = pc.run(c, points=x0)
    assert n == 1 and list(got["status"]) == [base["status"][0], 3, base["status"][2]] and np.array_equal(got["status"], ref["status"])
    for k in ("points", "error", "bone_error", "cost0", "cost"):
        assert np.isnan(got[k][1]).all(), k
        assert np.array_equal(got[k][[0, 2]], base[k][[0, 2]], equal_nan=True), k       # the other poses: the bits of the undisturbed run
    assert got["iterations"][1] == 0 and np.array_equal(got["iterations"][[0, 2]], base["iterations"][[0, 2]])


def test_a_nan_length_switches_its_bone_off():
    """parents must be one tree, so a bone cannot be taken out of them; what can be said on the device is that NaN is every other
    way of saying "no length" (not finite, not positive), bit for bit -- and against the restatement, which does take a forest,
    that the result is that of the tree without the bone"""
    B, V, J = 3, 3, 17
    c = pc.case(B, V, J, conf="uniform")
    L = c["limb"].copy()
    L[:, 12] = np.nan                                      # an inner bone: lsho - lelb
    got, n = _run(c, limb=L)
    assert n == 1 and np.isnan(got["bone_error"][:, 12]).all() and np.isfinite(got["bone_error"][:, 13]).all()
    for off in (np.inf, 0.0, -1.0):
        L2 = c["limb"].copy()
        L2[:, 12] = off
        other, _ = _run(c, limb=L2)
        for k in got:
            assert np.array_equal(got[k], other[k], equal_nan=True), (k, off)
    forest = list(c["parents"])
    forest[12] = -1
    ref = pc.run(c, parents=forest)
    ref["bone_error"][:, 12] = np.nan
    _assert_parity(got, ref, "bone 12 removed")
    assert np.array_equal(got["status"], ref["status"])
    full, _ = _run(c)
    assert not np.array_equal(full["points"], got["points"])


def test_runs_and_batchings_give_identical_bits():
    B, V, J = 5, 3, 17
    c = pc.case(B, V, J, conf="mixed")
    for kw in (dict(), dict(huber=HUBER)):
        a, n = _run(c, **kw)
        b, _ = _run(c, **kw)
        assert n == 1
        parts = [_run(c, points=c["points0"][s], pixels=c["pixels"][s], conf=c["conf"][s], limb=c["limb"][s], **kw)[0]
                 for s in (slice(0, 1), slice(1, B))]
        for k in a:
            assert np.array_equal(a[k], b[k], equal_nan=True), k
            assert np.array_equal(a[k], np.concatenate([p[k] for p in parts], axis=0), equal_nan=True), k


# ------------------------------------------------------------------------------------------------------------- 3. the closed loop
def test_closed_loop_two_views():
    """(32,2,17), 2 px of noise, true bone lengths: the device lands on the restatement's mean error, and on its own output the
    whole-pose refinement is at most 0.75 x refine_points' error"""
    from openmpl_amd import refine_points
    c, ref, _ = pc.two_view_loop()
    got, n = _run(c, max_iterations=100)
    pts = refine_points(_dev(c["points0"]), _dev(c["pixels"]), None, _dev(c["cams"]), distortion=_dev(c["dist"])).points.cpu().numpy()
    e_dev, e_ref, e_pts = (float(pc.joint_errors(x, c["truth"]).mean()) for x in (got["points"], ref["points"], pts))
    print("two views: refine_points %.5f, refine_poses %.5f (x %.3f); restatement %.5f" % (e_pts, e_dev, e_dev / e_pts, e_ref))
    assert n == 1 and (got["status"] == 0).all()
    assert abs(e_dev - e_ref) <= 0.01 * e_ref
    assert e_dev <= 0.75 * e_pts


def test_closed_loop_occluded_joints():
    """(32,4,17), 30 % of the joints seen by one view, the start a prediction 0.05 units off: the one-view joints end at no more than
    half of their start error on the device's own output, and every class of joint on the restatement's mean"""
    c, one, ref = pc.occlusion_loop()
    got, n = _run(c, max_iterations=100)
    e0, e_dev, e_ref = (pc.joint_errors(x, c["truth"]) for x in (c["points0"], got["points"], ref["points"]))
    print("occlusion: one-view joints %.5f -> %.5f (x %.3f; restatement %.5f), fully seen %.5f (restatement %.5f)"
          % (e0[one].mean(), e_dev[one].mean(), e_dev[one].mean() / e0[one].mean(), e_ref[one].mean(), e_dev[~one].mean(), e_ref[~one].mean()))
    assert n == 1 and (got["cost"] <= got["cost0"]).all() and (got["status"] < 2).all()
    assert abs(e_dev[one].mean() - e_ref[one].mean()) <= 0.01 * e_ref[one].mean()
    assert abs(e_dev[~one].mean() - e_ref[~one].mean()) <= 0.01 * e_ref[~one].mean()
    assert e_dev[one].mean() <= 0.5 * e0[one].mean()


# ------------------------------------------------------------------------------------------------------------------ the refusals
def test_refusals_of_the_c_abi_launch_nothing():
    import ctypes as C
    from openmpl_amd import cabi
    lib = cabi.load()
    B, V, J = 2, 3, 17
    c = pc.case(B, V, J)
    P, X, Cm, D, L = _dev(c["points0"]), _dev(c["pixels"]), _dev(c["cams"]), _dev(c["dist"]), _dev(c["limb"])
    out = torch.full((8, B * J), -12345.0, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    tree = lambda q: (C.c_int * len(q))(*q)      # noqa: E731

    def call(limb=L.data_ptr(), stride=J, parents=tree(c["parents"]), bw=1e4, it=20, joints=J):
        return lib.mpl_refine_poses(P.data_ptr(), X.data_ptr(), None, Cm.data_ptr(), D.data_ptr(), limb, stride, parents, B, V, joints, 0.0, bw,
                                    it, 1e-8, out[0].data_ptr(), out[3].data_ptr(), out[4].data_ptr(), None, None, None, None, st)

    two_roots, cycle, self_parent = list(c["parents"]), list(c["parents"]), list(c["parents"])
    two_roots[5] = -1
    cycle[1], cycle[2] = 2, 1
    self_parent[4] = 4
    codes, n = _launches(lambda: [call(limb=None), call(parents=None), call(stride=J - 1), call(stride=-1), call(parents=tree(two_roots)),
                                  call(parents=tree(cycle)), call(parents=tree(self_parent)), call(joints=65), call(bw=-1.0),
                                  call(bw=float("nan")), call(bw=float("inf")), call(it=1001)])
    assert codes == [-1] * 8 + [-2] * 4 and n == 0 and bool((out == -12345.0).all())
    ok, n = _launches(lambda: [call(), call(stride=0), call(bw=0.0)])
    assert ok == [0, 0, 0] and n == 3 and bool((out[5:] == -12345.0).all()) and bool((out[3] != -12345.0).all())
