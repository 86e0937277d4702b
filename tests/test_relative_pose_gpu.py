"""The relative pose of two views on the device (csrc/relative_pose.hip, csrc/five_point.hpp, openmpl_amd.geometry.relative_pose)
against the float64 restatement of tests/relative_pose_cases.py.

The hypothesis kernel runs one lane per hypothesis, 64 to a workgroup, and stages the correspondences 64 at a time; the cases of
relative_pose_cases.gpu_cases() are the shapes at which that can go wrong.  A hypothesis is compared pose by pose where the
restatement calls it well-conditioned, to POSE_TOL = 100 times the distance between two float64 formulations of the restatement
(measured over the same cases in test_relative_pose_cases_cpu.py).  Everything after the poses is compared with the restated steps
applied to the DEVICE's poses: counts exactly, costs and errors to the rounding of an fp64 sum in another order."""
import numpy as np
import pytest
import torch

from tests import relative_pose_cases as rp

pytestmark = pytest.mark.gpu

RTOL = 1e-10           # cost, error: fp64 sums of at most 2e3 non-negative terms in another order, and contracted multiply-adds
ZERO = 1e-15           # px^2: a cost that is zero but for rounding -- a pair of exactly five, every candidate fits them by construction
CASES = rp.gpu_cases()
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


def _relative(c, **kw):
    """relative_pose(return_hypotheses=True) on a case -> (dict of numpy arrays, the RelativePose)"""
    from openmpl_amd import relative_pose
    args = dict(rp.call_args(c), return_hypotheses=True)
    args.update(kw)
    r = relative_pose(_dev(c["pixels"]), _dev(c["conf"]), _dev(c["cams"]), distortion=_dev(c["dist"]), **args)
    B, V, J = c["pixels"].shape[:3]
    P, H = len(args["pairs"]), args["hypotheses"]
    assert r.rotation.dtype == torch.float64 and r.rotation.shape == (P, 3, 3) and r.direction.shape == (P, 3)
    assert r.cams.dtype == torch.float64 and r.cams.shape == (P, 2, 16) and r.error.dtype == torch.float64 and r.error.shape == (P,)
    assert r.inliers.dtype == torch.float32 and r.inliers.shape == (B, P, J)
    assert r.count.dtype == torch.int32 and r.best.dtype == torch.int32 and r.status.dtype == torch.uint8 and r.count.shape == (P,)
    assert r.poses.dtype == torch.float64 and r.poses.shape == (P, H, 12) and r.scores.dtype == torch.float64 and r.scores.shape == (P, H, 2)
    assert r.roots.dtype == torch.int32 and r.roots.shape == (P, H)
    return _numpy(r), r


def _case(name):
    """the device's run and the restated one of a case of gpu_cases(), each made once"""
    if name not in _RUNS:
        c = CASES[name]
        _RUNS[name] = (c, _relative(c)[0], rp.run(c))
    return _RUNS[name]


def _bits(a):
    return np.ascontiguousarray(a).view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def _same_bits(a, b):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in a)


def _check_against_own_poses(c, d, pairs=None, baseline=1.0):
    """scores, winner and outputs of a device run against the restated steps 4 and 5 on the device's own poses"""
    pairs = c["pairs"] if pairs is None else pairs
    P, H = d["poses"].shape[:2]
    void = np.isnan(d["poses"]).any(axis=-1)
    assert np.array_equal(void, np.isnan(d["poses"]).all(axis=-1))
    obs = rp.observations(c["pixels"], c["conf"], c["cams"], c["dist"], pairs)
    s = rp.score(obs, c["cams"], pairs, d["poses"], c["threshold"])
    np.testing.assert_array_equal(d["scores"][..., 0], s["count"])
    assert (d["scores"][void] == [0.0, np.inf]).all() and np.isfinite(d["scores"][~void]).all()
    got, cost = d["scores"][..., 1][~void], s["cost"][~void]
    zero = cost <= ZERO                                                  # nothing to be relative to: the device's is zero as well
    assert (got[zero] <= ZERO).all()
    np.testing.assert_allclose(got[~zero], cost[~zero], rtol=RTOL)
    want = rp.finish(obs, c["cams"], pairs, d["poses"], d["scores"], c["threshold"], baseline)
    for p in range(P):
        count, cost = d["scores"][p, :, 0], d["scores"][p, :, 1]
        ok = np.isfinite(cost) & obs["usable"][p]
        order = np.lexsort((np.arange(H), cost, -count))
        assert d["best"][p] == (order[ok[order]][0] if ok.any() else -1)
    np.testing.assert_array_equal(d["best"], want["best"])
    np.testing.assert_array_equal(d["status"], want["status"])
    np.testing.assert_array_equal(d["count"], want["count"])
    np.testing.assert_array_equal(d["inliers"], want["inliers"])
    for k in ("cams", "rotation", "direction"):                          # the winner's pose and the records, bit for bit
        assert np.array_equal(_bits(d[k]), _bits(want[k])), k
    np.testing.assert_allclose(d["error"], want["error"], rtol=RTOL, equal_nan=True)
    bad = d["status"] == 3
    assert (d["count"][bad] == 0).all() and np.isnan(d["error"][bad]).all() and not d["inliers"][:, bad].any()
    assert np.isnan(d["rotation"][bad]).all() and np.isnan(d["direction"][bad]).all() and np.isnan(d["cams"][bad][:, :, 4:]).all()
    return want


# ------------------------------------------------------------------------------------------------------------ the case set
@pytest.mark.parametrize("name", sorted(CASES))
def test_hypotheses_match_the_restatement(name):
    c, d, ref = _case(name)
    hyp = ref["hyp"]
    well = hyp["well"]
    void = np.isnan(d["poses"]).any(axis=-1)
    np.testing.assert_array_equal(void[well], ~hyp["valid"][well])
    assert void[~hyp["drawn"]].all() and (d["roots"][~hyp["drawn"]] == 0).all()
    np.testing.assert_array_equal(d["roots"][well], ref["roots"][well])
    both = well & hyp["valid"]
    gaps = rp.pose_gap(d["poses"], ref["poses"])
    # where every candidate has all participants as inliers, which of them is best is rounding: the device's is one of the restated
    with np.errstate(all="ignore"):
        nearest = np.nanmin(rp.pose_gap(hyp["candidates"]["poses"], d["poses"][:, :, None, :]), axis=2)
    gaps = np.where(hyp["tied"], nearest, gaps)
    gap = float(gaps[both].max()) if both.any() else 0.0
    print("%s: %d of %d hypotheses compared, poses within %.2e (allowed %.2e)" % (name, both.sum(), both.size, gap, rp.POSE_TOL))
    assert gap <= rp.POSE_TOL
    R, t = d["poses"][~void][:, :9].reshape(-1, 3, 3), d["poses"][~void][:, 9:]
    assert np.abs(np.einsum("nij,nkj->nik", R, R) - np.eye(3)).max() <= 1e-12 and np.allclose(np.linalg.det(R), 1.0, atol=1e-12)
    assert np.abs(np.linalg.norm(t, axis=1) - 1.0).max() <= 1e-12


@pytest.mark.parametrize("name", sorted(CASES))
def test_scores_winner_and_outputs_are_those_of_the_devices_own_poses(name):
    c, d, ref = _case(name)
    _check_against_own_poses(c, d)
    print("%s: status %s, best %s (restated %s), count %s (restated %s)" % (name, d["status"], d["best"], ref["best"], d["count"], ref["count"]))
    np.testing.assert_array_equal(d["status"], ref["status"])


def test_five_participants_are_one_short_and_six_are_enough():
    c, d, ref = _case("five")
    drawn = ref["hyp"]["drawn"][0]
    assert d["status"][0] == 3 and d["best"][0] >= 0 and drawn.any() and (d["scores"][0, drawn, 0] == 5).all()
    c, d, ref = _case("six")
    deg = rp.pose_errors(d["rotation"][0], d["direction"][0], c["truth_cams"], (0, 1))
    print("six participants, 2 px of noise: located %s degrees from the true pose" % (np.round(deg, 3),))
    # several hypotheses draw the same five of the six in another order and differ by rounding only: the winner's pose is compared
    assert d["status"][0] == 0 and d["count"][0] == 6
    assert rp.pose_gap(np.concatenate([d["rotation"][0].reshape(9), d["direction"][0]]), ref["poses"][0, ref["best"][0]]) <= rp.POSE_TOL


def test_outliers_and_the_winners_bounds_on_the_device():
    c, d, _ = _case("outliers")
    both = ~c["planted"][:, [0, 2]] & ~c["planted"][:, [1, 3]]
    for p, pair in enumerate(c["pairs"]):
        rot, way = rp.pose_errors(d["rotation"][p], d["direction"][p], c["truth_cams"], pair)
        planted = int((d["inliers"][:, p].astype(bool) & ~both[:, p]).sum())
        print("pair %s: winner %d with %d inliers, %d of them planted, off by %.2f degrees of rotation and %.2f of direction"
              % (pair, d["best"][p], d["count"][p], planted, rot, way))
        assert d["status"][p] == 0 and planted <= rp.WINNER_PLANTED and rot <= rp.WINNER_DEGREES[0] and way <= rp.WINNER_DEGREES[1]


def test_a_hypothesis_does_not_depend_on_the_grid():
    """H = 1, 63, 64, 65 and 256 on the same data are grids of 1, 1, 1, 2 and 4 workgroups a pair: hypothesis h is the same bits"""
    big = _case("small_h256")[1]
    for H in (1, 63, 64, 65):
        d = _case("small_h%d" % H)[1]
        for k in ("poses", "scores", "roots"):
            assert np.array_equal(_bits(d[k]), _bits(big[k][:, :H])), (H, k)


def test_seeds_differ_runs_give_identical_bits_and_three_launches():
    from openmpl_amd import relative_pose
    c = CASES["outliers"]
    a, b, other = _relative(c)[0], _relative(c)[0], _relative(c, seed=7)[0]
    assert _same_bits(a, b) and _same_bits(a, _case("outliers")[1])
    assert (a["best"] != other["best"]).all() and (other["status"] == 0).all()
    X, Cm, D = _dev(c["pixels"]), _dev(c["cams"]), _dev(c["dist"])
    plain, n = _launches(lambda: relative_pose(X, None, Cm, c["pairs"], D, hypotheses=256))
    assert n == 3 and plain.poses is None and plain.scores is None and plain.roots is None
    assert torch.equal(plain.cams.view(torch.int64), _dev(a["cams"]).view(torch.int64))


def test_the_swapped_pair_has_the_inverse_pose():
    """(1, 0) against (0, 1), each as pair 0 of its call and so with the same draws: R_10 = R_01^T, t_10 = -R_01^T t_01, hypothesis
    by hypothesis where both are well-conditioned"""
    c = CASES["small_h256"]
    d01, ref01 = _case("small_h256")[1:]
    d10 = _relative(c, pairs=((1, 0),))[0]
    ref10 = rp.run(c, pairs=((1, 0),))
    both = ref01["hyp"]["well"][0] & ref10["hyp"]["well"][0] & ref01["hyp"]["valid"][0] & ref10["hyp"]["valid"][0]
    R01, t01 = d01["poses"][0, both, :9].reshape(-1, 3, 3), d01["poses"][0, both, 9:]
    R10, t10 = d10["poses"][0, both, :9].reshape(-1, 3, 3), d10["poses"][0, both, 9:]
    gap = max(np.abs(R10 - R01.transpose(0, 2, 1)).max(), np.abs(t10 + np.einsum("nji,nj->ni", R01, t01)).max())
    print("%d hypotheses: the swapped pair's pose is the inverse within %.2e (allowed %.2e)" % (both.sum(), gap, rp.POSE_TOL))
    assert both.sum() >= 200 and gap <= rp.POSE_TOL
    np.testing.assert_array_equal(d10["scores"][0, both, 0], d01["scores"][0, both, 0])
    # and in one call, as pairs 0 and 1 with draws of their own, the winners are the two directions of one pose to a few degrees
    d = _relative(c, pairs=((0, 1), (1, 0)))[0]
    cos = (np.trace(d["rotation"][1] @ d["rotation"][0]) - 1.0) / 2.0
    assert (d["status"] == 0).all() and np.degrees(np.arccos(np.clip(cos, -1.0, 1.0))) <= 2.0 * rp.WINNER_DEGREES[0]
    assert np.array_equal(_bits(d["poses"][0]), _bits(d01["poses"][0]))


def test_baseline_scales_the_second_centre_only():
    c = CASES["small_h64"]
    d = _relative(c, baseline=2.5)[0]
    _check_against_own_poses(c, d, baseline=2.5)
    one = _case("small_h64")[1]
    assert np.array_equal(_bits(d["rotation"]), _bits(one["rotation"])) and np.array_equal(_bits(d["cams"][:, 0]), _bits(one["cams"][:, 0]))
    np.testing.assert_allclose(d["cams"][:, 1, 13:], 2.5 * one["cams"][:, 1, 13:], rtol=1e-15)


# ------------------------------------------------------------------------------------------------------------------ the edges
def _invalid(d, c, p, pair):
    return d["status"][p] == 3 and d["count"][p] == 0 and np.isnan(d["error"][p]) and not d["inliers"][:, p].any() and \
        np.isnan(d["rotation"][p]).all() and np.isnan(d["direction"][p]).all() and np.isnan(d["cams"][p, :, 4:]).all() and \
        np.array_equal(_bits(d["cams"][p, 0, :4]), _bits(c["cams"][pair[0], :4])) and \
        np.array_equal(_bits(d["cams"][p, 1, :4]), _bits(c["cams"][pair[1], :4]))


def test_invalid_pairs():
    four = rp.few_case(4)
    d = _relative(four)[0]
    assert _invalid(d, four, 0, (0, 1)) and d["best"][0] == -1 and (d["scores"][0] == [0.0, np.inf]).all() and np.isnan(d["poses"]).all()
    assert (d["roots"] == 0).all()
    # an all-NaN view, a view without confidence and a view whose intrinsics are not finite, beside a pair that is located
    c = rp.case(2, 5, 17, pairs=((0, 1), (0, 2), (3, 0), (1, 4), (4, 1)), hypotheses=65)
    c["pixels"] = c["pixels"].copy()
    c["pixels"][:, 2] = np.nan
    c["conf"] = np.ones((2, 5, 17), np.float32)
    c["conf"][:, 3] = 0.0
    c["conf"][0, 3, :3] = np.nan
    c["cams"][4, 1] = np.inf
    d = _relative(c)[0]
    assert d["status"].tolist() == [0, 3, 3, 3, 3] and all(_invalid(d, c, p, c["pairs"][p]) for p in (1, 2, 3, 4)) and (d["best"][1:] == -1).all()
    _check_against_own_poses(c, d)
    alone = _relative(c, pairs=((0, 1),))[0]
    for k in ("rotation", "direction", "cams", "inliers", "count", "best", "error", "poses", "scores", "roots"):
        assert np.array_equal(_bits(alone[k][:1] if k != "inliers" else alone[k][:, :1]), _bits(d[k][:1] if k != "inliers" else d[k][:, :1])), k


# ----------------------------------------------------------------------------------------------------------------- the polish
def _refined(c, rotation, direction, **kw):
    from openmpl_amd import refine_relative_pose
    return refine_relative_pose(_dev(c["pixels"]), _dev(c["conf"]), _dev(c["cams"]), c["pairs"], _dev(rotation), _dev(direction),
                                distortion=_dev(c["dist"]), **kw)


def test_polish_is_refine_relative_pose_on_the_inliers():
    from openmpl_amd import relative_pose
    c = CASES["outliers"]
    X, Cm, D = _dev(c["pixels"]), _dev(c["cams"]), _dev(c["dist"])
    plain, n0 = _launches(lambda: relative_pose(X, None, Cm, c["pairs"], D, hypotheses=256))
    r, n1 = _launches(lambda: relative_pose(X, None, Cm, c["pairs"], D, hypotheses=256, refine=True, huber=6.0))
    assert n0 == 3 and n1 == 4 and plain.refined is None
    hand = _refined(c, plain.rotation.cpu().numpy(), plain.direction.cpu().numpy(), huber=6.0, weight=plain.inliers)
    for k in hand._fields:
        assert torch.equal(getattr(r.refined, k).view(torch.uint8), getattr(hand, k).view(torch.uint8)), k
    assert r.cams is r.refined.cams and r.rotation is r.refined.rotation and r.direction is r.refined.direction
    for k in ("inliers", "count", "best", "error", "status"):
        assert torch.equal(getattr(r, k).view(torch.uint8), getattr(plain, k).view(torch.uint8)), k
    truth = [rp.true_pose(c["truth_cams"], pair) for pair in c["pairs"]]
    t = _refined(c, np.stack([x[0] for x in truth]), np.stack([x[1] for x in truth]), huber=6.0, weight=plain.inliers)
    gap = max(float((r.rotation - t.rotation).abs().max()), float((r.direction - t.direction).abs().max()))
    R, w = r.rotation.cpu().numpy(), r.direction.cpu().numpy()
    deg = [rp.pose_errors(R[p], w[p], c["truth_cams"], pair) for p, pair in enumerate(c["pairs"])]
    print("polished poses within %.1e of refine_relative_pose from the true poses (allowed %.1e); trials %s; %s degrees from the truth"
          % (gap, 100.0 * rp.POLISH_SPREAD, r.refined.iterations.tolist(), np.round(deg, 2).tolist()))
    assert gap <= 100.0 * rp.POLISH_SPREAD and bool((r.refined.status == 0).all()) and bool((r.refined.cost <= r.refined.cost0).all())
    assert torch.equal(r.refined.used, plain.count)
    assert np.abs(np.einsum("pij,pkj->pik", R, R) - np.eye(3)).max() <= 1e-12 and np.abs(np.linalg.norm(w, axis=1) - 1.0).max() <= 1e-12
    # against the restatement: costs and error at the given pose, and the final pose
    ref = rp.refine(c["pixels"], c["conf"], c["cams"], c["pairs"], plain.rotation.cpu().numpy(), plain.direction.cpu().numpy(), c["dist"], 6.0,
                    weight=plain.inliers.cpu().numpy())
    np.testing.assert_allclose(hand.cost0.cpu().numpy(), ref["cost0"], rtol=RTOL)
    np.testing.assert_allclose(hand.cost.cpu().numpy(), ref["cost"], rtol=1e-8)
    assert max(np.abs(R - ref["rotation"]).max(), np.abs(w - ref["direction"]).max()) <= 100.0 * rp.POLISH_SPREAD
    assert hand.status.tolist() == ref["status"].tolist() and hand.used.tolist() == ref["used"].tolist()
    # with confidences the weights are conf_a * conf_b * inliers
    cf = _dev(np.random.RandomState(1).uniform(0.3, 1.0, c["pixels"].shape[:3]).astype(np.float32))
    wr = relative_pose(X, cf, Cm, c["pairs"], D, hypotheses=256, refine=True)
    base = relative_pose(X, cf, Cm, c["pairs"], D, hypotheses=256)
    from openmpl_amd import refine_relative_pose
    hand = refine_relative_pose(X, cf, Cm, c["pairs"], base.rotation, base.direction, distortion=D, weight=base.inliers)
    assert torch.equal(wr.cams.view(torch.uint8), hand.cams.view(torch.uint8))


def test_polish_passes_through_and_says_what_is_invalid():
    c, d, _ = _case("small_h64")
    zero = _refined(c, d["rotation"], d["direction"], max_iterations=0)
    assert zero.status.tolist() == [2] and zero.iterations.tolist() == [0] and torch.equal(zero.cost, zero.cost0)
    assert np.array_equal(_bits(zero.rotation.cpu().numpy()), _bits(d["rotation"]))
    assert np.array_equal(_bits(zero.direction.cpu().numpy()), _bits(d["direction"]))
    ref = rp.refine(c["pixels"], c["conf"], c["cams"], c["pairs"], d["rotation"], d["direction"], c["dist"], max_iterations=0)
    np.testing.assert_allclose(zero.cost0.cpu().numpy(), ref["cost0"], rtol=RTOL)
    np.testing.assert_allclose(zero.error.cpu().numpy(), ref["error"], rtol=RTOL)
    assert zero.used.tolist() == ref["used"].tolist()
    two = _numpy(_refined(c, d["rotation"], d["direction"])), _numpy(_refined(c, d["rotation"], d["direction"]))
    assert _same_bits(*two) and two[0]["status"].tolist() == [0] and (two[0]["cost"] <= two[0]["cost0"]).all()
    nan = _refined(c, np.full((1, 3, 3), np.nan), d["direction"])
    assert nan.status.tolist() == [3] and bool(nan.error.isnan().all()) and bool(nan.cams[:, :, 4:].isnan().all())
    five = CASES["five"]
    few = _refined(five, d["rotation"], d["direction"])
    assert few.status.tolist() == [2] and few.used.tolist() == [5]
    # an invalid pair of relative_pose stays invalid through refine=True
    four = rp.few_case(4)
    r = _relative(four, refine=True)[1]
    assert r.status.tolist() == [3] and r.refined.status.tolist() == [3] and bool(r.rotation.isnan().all())


# ----------------------------------------------------------------------------------------------------------- the closed loop
def test_closed_loop_from_pixels_and_intrinsics():
    """refine_cameras_cases.closed_loop_case, (64,4,17), H36M-like lens, 2 px of noise, every pose blanked.  relative_pose on views
    0 and 1 with refine=True, huber=6.0 -> triangulate_pixels on the pair under its two records -> locate_cameras(fixed=(0, 1), refine=True) ->
    bundle_adjust(fixed=(0, 1), rounds=8); the points against the truth after one global similarity (the baseline is a free gauge).
    The aligned mean point error is at most 1.1 times that of the same chain with the pair's true relative pose handed in (view a
    the identity, unit baseline).  Measured: see DESIGN.md section 7"""
    from openmpl_amd import bundle_adjust, locate_cameras, relative_pose, triangulate_pixels
    from tests import locate_cameras_cases as lc
    from tests import refine_cameras_cases as cc
    from tests import refine_cases as rc
    c, _ = cc.closed_loop_case()
    X, D = _dev(c["pixels"]), _dev(c["dist"])
    blank = lc.blank(c["cams"])

    def chain(pair):
        cams = blank.copy()
        cams[:2] = pair
        lin2, _, _ = triangulate_pixels(X[:, :2].contiguous(), None, _dev(cams[:2]), rc.WH, distortion=D[:2].contiguous())
        loc = locate_cameras(lin2, X, None, _dev(cams), D, fixed=(0, 1), refine=True)
        assert loc.status.tolist() == [2, 2, 0, 0]
        return rp.aligned_mean_error(bundle_adjust(lin2, X, None, loc.cams, D, rounds=8, fixed=(0, 1)).points.cpu().numpy(), c["truth"])

    rel = relative_pose(X, None, _dev(blank), ((0, 1),), D, refine=True, huber=6.0)
    assert rel.status.tolist() == [0] and rel.refined.status.tolist() == [0]
    deg = rp.pose_errors(rel.rotation[0].cpu().numpy(), rel.direction[0].cpu().numpy(), c["cams"], (0, 1))
    R, t, _ = rp.true_pose(c["cams"], (0, 1))
    true_pair = np.zeros((2, 16))
    true_pair[:, :4] = c["cams"][:2, :4]
    true_pair[0, 4:13], true_pair[1, 4:13], true_pair[1, 13:] = np.eye(3).reshape(9), R.reshape(9), -R.T @ t
    e, e_true = chain(rel.cams[0].cpu().numpy()), chain(true_pair)
    print("the located pair is %.2f / %.2f degrees off; aligned mean point error %.5f, from the true relative pose %.5f" % (deg + (e, e_true)))
    assert e <= 1.1 * e_true


# ------------------------------------------------------------------------------------------------------------- argument errors
def test_argument_errors_launch_nothing():
    from openmpl_amd import relative_pose
    c = CASES["small_h1"]
    X, Cm, D = _dev(c["pixels"]), _dev(c["cams"]), _dev(c["dist"])

    def refused():
        for kw, msg in ((dict(threshold=0.0), "threshold must be"), (dict(threshold=float("nan")), "threshold must be"),
                        (dict(hypotheses=0), "hypotheses must be"), (dict(hypotheses=65537), "hypotheses must be"),
                        (dict(hypotheses=2.5), "hypotheses must be"), (dict(pairs=((0, 0),)), "pairs holds two distinct view indices"),
                        (dict(pairs=((0, 2),)), "pairs holds two distinct view indices"), (dict(pairs=3), "pairs must be a sequence"),
                        (dict(pairs=((0, 1),) * 33), "between 1 and 32 pairs"), (dict(baseline=0.0), "baseline must be"),
                        (dict(baseline=float("inf")), "baseline must be"), (dict(seed=0.5), "seed must be"),
                        (dict(huber=6.0), "huber is an option of the refinement"), (dict(refine=True, huber=0.0), "huber must be")):
            with pytest.raises(RuntimeError, match=msg):
                relative_pose(X, None, Cm, distortion=D, **kw)
        with pytest.raises(RuntimeError, match="cams must be float64"):
            relative_pose(X, None, Cm.float(), distortion=D)
        with pytest.raises(NotImplementedError, match="at most 32 views, 64 joints"):
            relative_pose(torch.zeros(1, 2, 65, 2, device="cuda"), None, Cm)

    _, n = _launches(refused)
    assert n == 0
