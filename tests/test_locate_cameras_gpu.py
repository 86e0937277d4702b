"""Cameras located from scratch on the device (csrc/locate_cameras.hip, openmpl_amd.geometry.locate_cameras) against the float64
restatement of tests/locate_cameras_cases.py.

The hypothesis kernel runs one lane per hypothesis, 64 to a workgroup, and stages the observations 64 at a time; the cases of
locate_cameras_cases.gpu_cases() are the shapes at which that can go wrong.  A hypothesis is compared pose by pose where the
restatement calls its 12 x 12 system well-conditioned, to POSE_TOL = 100 times the distance between two float64 formulations of the
restatement (measured over the same cases in test_locate_cameras_cases_cpu.py).  Everything after the poses is compared with the
restated steps applied to the DEVICE's poses: counts exactly, costs and errors to the rounding of an fp64 sum in another order."""
import numpy as np
import pytest
import torch

from tests import locate_cameras_cases as lc
from tests import refine_cameras_cases as cc
from tests import refine_cases as rc

pytestmark = pytest.mark.gpu

RTOL = 1e-10           # cost, error: fp64 sums of at most 2e3 non-negative terms in another order, and contracted multiply-adds
CASES = lc.gpu_cases()
_RUNS = {}


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


def _numpy(r):
    return {k: getattr(r, k).cpu().numpy() for k in r._fields if isinstance(getattr(r, k), torch.Tensor)}


def _locate(c, **kw):
    """locate_cameras(return_hypotheses=True) on a case -> (dict of numpy arrays, the CamerasLocated)"""
    from openmpl_amd import locate_cameras
    args = dict(lc.call_args(c), return_hypotheses=True)
    args.update(kw)
    r = locate_cameras(_dev(c["points"]), _dev(c["pixels"]), _dev(c["conf"]), _dev(c["cams"]), _dev(c["dist"]), **args)
    B, V, J = c["pixels"].shape[:3]
    H = args["hypotheses"]
    assert r.cams.dtype == torch.float64 and r.cams.shape == (V, 16) and r.error.dtype == torch.float64 and r.error.shape == (V,)
    assert r.inliers.dtype == torch.float32 and r.inliers.shape == (B, V, J)
    assert r.count.dtype == torch.int32 and r.best.dtype == torch.int32 and r.status.dtype == torch.uint8 and r.count.shape == (V,)
    assert r.poses.dtype == torch.float64 and r.poses.shape == (V, H, 12) and r.scores.dtype == torch.float64 and r.scores.shape == (V, H, 2)
    return _numpy(r), r


def _case(name):
    """the device's run and the restated one of a case of gpu_cases(), each made once"""
    if name not in _RUNS:
        c = CASES[name]
        _RUNS[name] = (c, _locate(c)[0], lc.locate(c["points"], c["pixels"], c["conf"], c["cams"], c["dist"], **lc.call_args(c)))
    return _RUNS[name]


def _bits(a):
    return np.ascontiguousarray(a).view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def _same_bits(a, b):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in a)


def _check_against_own_poses(c, d):
    """scores, winner and outputs of a device run against the restated steps 5 and 6 on the device's own poses"""
    V, H = d["poses"].shape[:2]
    void = np.isnan(d["poses"]).any(axis=-1)
    assert np.array_equal(void, np.isnan(d["poses"]).all(axis=-1))
    s = lc.score(c["points"], c["pixels"], c["conf"], c["cams"], c["dist"], d["poses"], c["threshold"])
    np.testing.assert_array_equal(d["scores"][..., 0], s["count"])
    assert (d["scores"][void] == [0.0, np.inf]).all() and np.isfinite(d["scores"][~void]).all()
    np.testing.assert_allclose(d["scores"][..., 1][~void], s["cost"][~void], rtol=RTOL)
    want = lc.finish(c["points"], c["pixels"], c["conf"], c["cams"], c["dist"], d["poses"], dict(s, count=d["scores"][..., 0],
                     cost=d["scores"][..., 1]), c["threshold"], c["fixed"])
    for v in range(V):
        count, cost = d["scores"][v, :, 0], d["scores"][v, :, 1]
        if v in c["fixed"]:
            assert d["best"][v] == -1 and void[v].all()
        else:
            ok = np.isfinite(cost)
            order = np.lexsort((np.arange(H), cost, -count))
            assert d["best"][v] == (order[ok[order]][0] if ok.any() else -1)
    np.testing.assert_array_equal(d["best"], want["best"])
    np.testing.assert_array_equal(d["status"], want["status"])
    np.testing.assert_array_equal(d["count"], want["count"])
    np.testing.assert_array_equal(d["inliers"], want["inliers"])
    assert np.array_equal(_bits(d["cams"]), _bits(want["cams"]))          # the winner's pose, or the given row, bit for bit
    np.testing.assert_allclose(d["error"], want["error"], rtol=RTOL, equal_nan=True)
    bad = d["status"] == 3
    assert (d["count"][bad] == 0).all() and np.isnan(d["error"][bad]).all() and not d["inliers"][:, bad].any()
    return want


# ------------------------------------------------------------------------------------------------------------ the case set
@pytest.mark.parametrize("name", sorted(CASES))
def test_hypotheses_match_the_restatement(name):
    c, d, ref = _case(name)
    hyp = ref["hyp"]
    well = hyp["well"]
    void = np.isnan(d["poses"]).any(axis=-1)
    np.testing.assert_array_equal(void[well], ~hyp["valid"][well])
    assert void[~hyp["drawn"]].all()
    both = well & hyp["valid"]
    gap = float(np.abs(d["poses"] - ref["poses"])[both].max()) if both.any() else 0.0
    print("%s: %d of %d hypotheses compared, poses within %.2e (allowed %.2e)" % (name, both.sum(), both.size, gap, lc.POSE_TOL))
    assert gap <= lc.POSE_TOL
    R = d["poses"][~void][:, :9].reshape(-1, 3, 3)
    assert np.abs(np.einsum("nij,nkj->nik", R, R) - np.eye(3)).max() <= 1e-12 and np.allclose(np.linalg.det(R), 1.0, atol=1e-12)


@pytest.mark.parametrize("name", sorted(CASES))
def test_scores_winner_and_outputs_are_those_of_the_devices_own_poses(name):
    c, d, ref = _case(name)
    _check_against_own_poses(c, d)
    live = [v for v in range(len(c["cams"])) if v not in c["fixed"]]
    # and the outcome is the restatement's, where its own winner is clear of a tie and of the pose tolerance: printed, not asserted
    print("%s: status %s, best %s (restated %s), count %s (restated %s)" % (name, d["status"], d["best"][live], ref["best"][live],
                                                                            d["count"], ref["count"]))
    np.testing.assert_array_equal(d["status"], ref["status"])
    for v in c["fixed"]:
        assert np.array_equal(_bits(d["cams"][v]), _bits(c["cams"][v])) and d["status"][v] == 2


def test_outliers_stay_out_on_the_device():
    c, d, _ = _case("outliers")
    deg, off = lc.pose_errors(d["cams"], c["truth_cams"])
    print("winners %s with %s inliers, off by %s degrees and %s units" % (d["best"], d["count"], np.round(deg, 2), np.round(off, 3)))
    assert (d["status"] == 0).all() and not (d["inliers"].astype(bool) & c["planted"]).any()
    assert (deg <= lc.WINNER_DEGREES).all() and (off <= lc.WINNER_UNITS).all()


def test_a_hypothesis_does_not_depend_on_the_grid():
    """H = 1, 63, 64, 65 and 256 on the same data are grids of 1, 1, 1, 2 and 4 workgroups a view: hypothesis h is the same bits"""
    big = _case("small_h256")[1]
    for H in (1, 63, 64, 65):
        d = _case("small_h%d" % H)[1]
        assert np.array_equal(_bits(d["poses"]), _bits(big["poses"][:, :H])) and np.array_equal(_bits(d["scores"]), _bits(big["scores"][:, :H]))


# ------------------------------------------------------------------------------------------------------------------ the edges
def _invalid(d, c, v=0):
    return d["status"][v] == 3 and d["count"][v] == 0 and np.isnan(d["error"][v]) and not d["inliers"][:, v].any() and \
        np.array_equal(_bits(d["cams"][v]), _bits(c["cams"][v]))


def test_invalid_views():
    five = lc.case(1, 1, 5)
    d = _locate(five)[0]
    assert _invalid(d, five) and d["best"][0] == -1 and (d["scores"][0] == [0.0, np.inf]).all() and np.isnan(d["poses"]).all()
    # an all-NaN view, a view without confidence and a view whose intrinsics are not finite, beside one that is located
    c = lc.case(2, 4, 17, hypotheses=65)
    c["pixels"] = c["pixels"].copy()
    c["pixels"][:, 1] = np.nan
    c["conf"] = np.ones((2, 4, 17), np.float32)
    c["conf"][:, 2] = 0.0
    c["conf"][0, 2, :3] = np.nan
    c["cams"][3, 1] = np.inf
    d = _locate(c)[0]
    assert d["status"].tolist() == [0, 3, 3, 3] and all(_invalid(d, c, v) for v in (1, 2, 3)) and (d["best"][1:] == -1).all()
    _check_against_own_poses(c, d)
    alone = _locate({k: (x[:, :1] if k in ("pixels", "conf") else x[:1] if k in ("cams", "dist") else x) for k, x in c.items()})[0]
    assert np.array_equal(_bits(alone["cams"][0]), _bits(d["cams"][0])) and np.array_equal(alone["inliers"][:, 0], d["inliers"][:, 0])


def test_points_behind_every_hypothesis():
    c = lc.behind_case()
    d = _locate(c)[0]
    assert _invalid(d, c) and d["best"][0] == -1 and (d["scores"][0] == [0.0, np.inf]).all() and np.isnan(d["poses"]).all()


def test_hypotheses_void_by_the_draw():
    c = lc.void_draw_case()
    d = _locate(c)[0]
    ref = lc.locate(c["points"], c["pixels"], None, c["cams"], c["dist"], **lc.call_args(c))
    void = np.isnan(d["poses"]).any(axis=-1)
    assert 0 < (~ref["hyp"]["drawn"]).sum() < 8 and void[~ref["hyp"]["drawn"]].all()
    np.testing.assert_array_equal(void, ~ref["hyp"]["valid"])
    _check_against_own_poses(c, d)
    assert _invalid(d, c) and d["best"][0] >= 0                  # a winner with fewer than six inliers


def test_seeds_differ_and_runs_give_identical_bits():
    c = CASES["outliers"]
    a, b, other = _locate(c)[0], _locate(c)[0], _locate(c, seed=7)[0]
    assert _same_bits(a, b) and _same_bits(a, _case("outliers")[1])
    assert (a["best"] != other["best"]).all() and (other["status"] == 0).all()
    assert not (other["inliers"].astype(bool) & c["planted"]).any()


# ----------------------------------------------------------------------------------------------------------------- the polish
def test_polish_is_refine_cameras_on_the_inliers():
    from openmpl_amd import locate_cameras, refine_cameras
    c = CASES["outliers"]
    P, X, Cm, D = _dev(c["points"]), _dev(c["pixels"]), _dev(c["cams"]), _dev(c["dist"])
    plain, n0 = _launches(lambda: locate_cameras(P, X, None, Cm, D, hypotheses=256))
    r, n1 = _launches(lambda: locate_cameras(P, X, None, Cm, D, hypotheses=256, refine=True, huber=6.0))
    assert n0 == 3 and n1 == 4 and plain.refined is None and plain.poses is None and plain.scores is None
    hand = refine_cameras(P, X, plain.inliers, plain.cams, D, huber=6.0)
    for k in hand._fields:
        assert torch.equal(getattr(r.refined, k).view(torch.uint8), getattr(hand, k).view(torch.uint8)), k
    assert r.cams is r.refined.cams
    for k in ("inliers", "count", "best", "error", "status"):
        assert torch.equal(getattr(r, k).view(torch.uint8), getattr(plain, k).view(torch.uint8)), k
    truth = refine_cameras(P, X, plain.inliers, _dev(c["truth_cams"]), D, huber=6.0)
    gap = float((r.cams - truth.cams).abs().max())
    deg, off = lc.pose_errors(r.cams.cpu().numpy(), c["truth_cams"])
    print("polished records within %.1e of refine_cameras from the true poses; trials %s; off by %s degrees, %s units"
          % (gap, r.refined.iterations.tolist(), np.round(deg, 3), np.round(off, 4)))
    assert gap <= 1e-6 and bool((r.refined.status == 0).all())
    # with confidences the weights are conf * inliers
    cf = _dev(np.random.RandomState(1).uniform(0.3, 1.0, c["pixels"].shape[:3]).astype(np.float32))
    w = locate_cameras(P, X, cf, Cm, D, hypotheses=256, refine=True)
    hand = refine_cameras(P, X, cf * w.inliers, locate_cameras(P, X, cf, Cm, D, hypotheses=256).cams, D)
    assert torch.equal(w.cams.view(torch.uint8), hand.cams.view(torch.uint8))


def test_closed_loop_from_two_calibrated_cameras():
    """refine_cameras_cases.closed_loop_case: (64,4,17), H36M-like lens, 2 px of noise.  Cameras 2 and 3 have no pose at all; the
    points come from cameras 0 and 1 alone.  locate_cameras(fixed=(0, 1), refine=True) -> bundle_adjust(fixed=(0, 1), rounds=8) ends
    within 10 % of the point error the same bundle adjustment reaches from the 2-degree perturbation of that case (0.0067)."""
    from openmpl_amd import bundle_adjust, locate_cameras, triangulate_pixels
    c, cams0 = cc.closed_loop_case()
    X, D = _dev(c["pixels"]), _dev(c["dist"])
    lin4, _, _ = triangulate_pixels(X, None, _dev(cams0), rc.WH, distortion=D)
    e_ref = rc.mean_error(bundle_adjust(lin4, X, None, _dev(cams0), D, rounds=8, fixed=(0, 1)).points.cpu().numpy(), c["truth"])[0]
    blank = lc.blank(c["cams"], keep=(0, 1))
    lin2, _, _ = triangulate_pixels(X[:, :2].contiguous(), None, _dev(c["cams"][:2]), rc.WH, distortion=D[:2].contiguous())
    loc = locate_cameras(lin2, X, None, _dev(blank), D, fixed=(0, 1), refine=True)
    assert loc.status.tolist() == [2, 2, 0, 0] and torch.equal(loc.cams[:2].view(torch.int64), _dev(blank)[:2].view(torch.int64))
    r = bundle_adjust(lin2, X, None, loc.cams, D, rounds=8, fixed=(0, 1))
    cost = r.cost.cpu().numpy()
    ref = cc.bundle_adjust(lin2.cpu().numpy(), c["pixels"], None, loc.cams.cpu().numpy(), c["dist"], None, 8, (0, 1))
    e0, e1 = rc.mean_error(lin2.cpu().numpy(), c["truth"])[0], rc.mean_error(r.points.cpu().numpy(), c["truth"])[0]
    deg, off = lc.pose_errors(loc.cams.cpu().numpy(), c["cams"])
    print("located cameras off by %s degrees and %s units; mean point error %.5f -> %.5f (from the 2-degree perturbation: %.5f); cost %s"
          % (np.round(deg[2:], 3), np.round(off[2:], 4), e0, e1, e_ref, np.round(cost, 1)))
    assert (cost[1:] <= cost[:-1] + 2 * ref["slack"]).all()
    assert abs(e_ref - 0.0067) < 0.0005 and e1 <= 1.1 * e_ref
    assert torch.equal(r.cams[:2].view(torch.int64), _dev(c["cams"])[:2].view(torch.int64))


# ------------------------------------------------------------------------------------------------------------- argument errors
def test_argument_errors_launch_nothing():
    from openmpl_amd import locate_cameras
    c = CASES["small_h1"]
    P, X, Cm, D = _dev(c["points"]), _dev(c["pixels"]), _dev(c["cams"]), _dev(c["dist"])

    def refused():
        for kw, msg in ((dict(threshold=0.0), "threshold must be"), (dict(threshold=float("nan")), "threshold must be"),
                        (dict(hypotheses=0), "hypotheses must be"), (dict(hypotheses=65537), "hypotheses must be"),
                        (dict(hypotheses=2.5), "hypotheses must be"), (dict(fixed=(2,)), "fixed holds view indices"),
                        (dict(fixed=3), "fixed must be a sequence"), (dict(huber=6.0), "huber is an option of the refinement"),
                        (dict(refine=True, huber=0.0), "huber must be"), (dict(seed=0.5), "seed must be")):
            with pytest.raises(RuntimeError, match=msg):
                locate_cameras(P, X, None, Cm, D, **kw)
        with pytest.raises(RuntimeError, match="cams must be float64"):
            locate_cameras(P, X, None, Cm.float(), D)
        with pytest.raises(NotImplementedError, match="at most 32 views, 64 joints"):
            locate_cameras(torch.zeros(1, 65, 3, device="cuda"), torch.zeros(1, 2, 65, 2, device="cuda"), None, Cm)

    _, n = _launches(refused)
    assert n == 0
