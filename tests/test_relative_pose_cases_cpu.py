"""The relative pose of two views (csrc/relative_pose.hip, csrc/five_point.hpp) without a GPU: the float64 restatement of
tests/relative_pose_cases.py pinned on its own -- exact data brings the true pose back under both formulations of the solver, the
winner is the lexicographic one, the winners of the outlier case lie within the recorded bounds --, the properties of the GPU cases
that their comparisons rest on, the C prototype against its binding and its refusals, and the argument checks of the Python surface,
which are raised before any device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from openmpl_amd import cabi
from tests import locate_cameras_cases as lc
from tests import relative_pose_cases as rp

HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mpl_hip.h")).read()


# ----------------------------------------------------------------------------------------------------------------- the boundary
def test_exported_bound_and_declared():
    import openmpl_amd
    from openmpl_amd import geometry
    lib = cabi.load()
    assert "mpl_relative_pose" in cabi.EXPORTS and hasattr(lib, "mpl_relative_pose") and cabi.ABI_VERSION == 14
    m = re.search(r"\bint mpl_relative_pose\(([^;]*)\);", HEADER)
    assert m, "mpl_relative_pose is not declared in include/mpl_hip.h"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    kinds = {"int": C.c_int, "double": C.c_double, "unsigned": C.c_uint, "size_t": C.c_size_t}

    def ctype(p):
        if "*" not in p:
            return kinds[p.rsplit(" ", 1)[0]]
        return C.POINTER(C.c_uint64) if "long long" in p else C.POINTER(C.c_int) if p.startswith("const int") else cabi._fp
    assert [ctype(p) for p in params] == list(lib.mpl_relative_pose.argtypes) and lib.mpl_relative_pose.restype is C.c_int
    assert re.search(r"size_t mpl_relative_pose_workspace_bytes\(int batch, int pairs, int joints\);", HEADER)
    sources = __import__("openmpl_amd.build", fromlist=["SOURCES"])
    assert "relative_pose.hip" in sources.SOURCES and any(h.endswith("five_point.hpp") for h in sources.HEADERS)
    assert openmpl_amd.relative_pose is geometry.relative_pose
    assert geometry.RelativePose._fields == ("rotation", "direction", "cams", "inliers", "count", "best", "error", "status", "refined",
                                             "poses", "scores", "roots")
    m = re.search(r"\bint mpl_refine_relative_pose\(([^;]*)\);", HEADER)
    assert m, "mpl_refine_relative_pose is not declared in include/mpl_hip.h"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert [ctype(p) for p in params] == list(lib.mpl_refine_relative_pose.argtypes) and lib.mpl_refine_relative_pose.restype is C.c_int
    assert "mpl_refine_relative_pose" in cabi.EXPORTS and "refine_relative_pose.hip" in sources.SOURCES
    assert openmpl_amd.refine_relative_pose is geometry.refine_relative_pose
    assert geometry.RelativeRefined._fields == ("rotation", "direction", "cams", "error", "cost0", "cost", "used", "iterations", "status")
    assert lib.mpl_relative_pose_workspace_bytes(8, 2, 17) == 2 * (8 + 9 * 136) * 8
    assert lib.mpl_relative_pose_workspace_bytes(0, 2, 17) == 0 and lib.mpl_relative_pose_workspace_bytes(1, 33, 17) == 0
    assert lib.mpl_relative_pose_workspace_bytes(1, 1, 65) == 0


def test_c_abi_refusals_need_no_device():
    lib = cabi.load()
    p = lambda a: None if a is None else C.c_void_p(a)            # never dereferenced by a refused call      # noqa: E731
    keys = (C.c_uint64 * 32)()
    good = (C.c_int * 4)(0, 1, 2, 0)

    def call(pixels=8, cams=8, B=2, V=3, J=17, pairs=good, P=2, tau=6.0, H=64, k=keys, base=1.0, ws=8, wsb=1 << 30, rot=8, inl=8, roots=8):
        return lib.mpl_relative_pose(p(pixels), None, p(cams), None, B, V, J, pairs, P, tau, H, k, base, p(ws), wsb, p(rot), p(8), p(8),
                                     p(inl), p(8), p(8), p(8), p(8), p(8), p(8), p(roots), None)
    assert call(pixels=None) == -1 and call(cams=None) == -1 and call(pairs=None) == -1 and call(k=None) == -1
    assert call(rot=None) == -1 and call(inl=None) == -1 and call(roots=None) == -1
    assert call(B=0) == -1 and call(V=33) == -1 and call(J=65) == -1 and call(P=0) == -1 and call(P=33) == -1
    assert call(B=1 << 20, V=32, J=64) == -1
    for bad in ((0, 0, 1, 2), (0, 3, 1, 2), (-1, 0, 1, 2), (0, 1, 2, 2)):
        assert call(pairs=(C.c_int * 4)(*bad)) == -1              # not two distinct views of the rig
    for tau in (0.0, -1.0, float("nan"), float("inf")):
        assert call(tau=tau) == -2 and call(base=tau) == -2
    assert call(H=0) == -2 and call(H=65537) == -2
    assert call(pixels=None, H=0) == -1                           # the pointers come first
    small = call(ws=None)
    assert small != 0 and small == call(wsb=lib.mpl_relative_pose_workspace_bytes(2, 2, 17) - 1)
    assert call(H=0, ws=None) == -2                               # and the workspace last


def test_c_abi_refusals_of_the_polish_need_no_device():
    lib = cabi.load()
    p = lambda a: None if a is None else C.c_void_p(a)            # noqa: E731
    good = (C.c_int * 4)(0, 1, 2, 0)

    def call(pixels=8, cams=8, B=2, V=3, J=17, pairs=good, P=2, rot=8, way=8, it=20, tol=1e-8, base=1.0, out=8, err=8):
        return lib.mpl_refine_relative_pose(p(pixels), None, None, p(cams), None, B, V, J, pairs, P, p(rot), p(way), 0.0, it, tol, base,
                                            p(out), p(8), p(8), p(err), None, None, None, None, None, None)
    assert call(pixels=None) == -1 and call(cams=None) == -1 and call(pairs=None) == -1 and call(rot=None) == -1 and call(way=None) == -1
    assert call(out=None) == -1 and call(err=None) == -1 and call(B=0) == -1 and call(V=33) == -1 and call(J=65) == -1 and call(P=33) == -1
    assert call(pairs=(C.c_int * 4)(0, 0, 1, 2)) == -1 and call(pairs=(C.c_int * 4)(0, 3, 1, 2)) == -1
    assert call(it=-1) == -2 and call(it=1001) == -2 and call(tol=-1.0) == -2 and call(tol=float("nan")) == -2
    assert call(base=0.0) == -2 and call(base=float("inf")) == -2
    assert call(pixels=None, it=-1) == -1                         # the pointers come first


# ------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("method", ["action", "poly"])
@pytest.mark.parametrize("lens", [True, False])
def test_exact_data_brings_the_true_pose_back(method, lens):
    c = rp.case(4, 3, 17, pairs=((0, 1), (2, 1)), noise=0.0, lens=lens, exact=True, hypotheses=32)
    r = rp.run(c, method=method)
    hyp = r["hyp"]
    worst, nearest = 0.0, []
    for p, pair in enumerate(c["pairs"]):
        R, t, _ = rp.true_pose(c["truth_cams"], pair)
        truth = np.concatenate([R.reshape(9), t])
        nearest += list(np.nanmin(rp.pose_gap(hyp["candidates"]["poses"][p], truth), axis=1)[hyp["well"][p]])
        worst = max(worst, float(rp.pose_gap(r["poses"][p], truth)[hyp["well"][p]].max()))
        deg = rp.pose_errors(r["rotation"][p], r["direction"][p], c["truth_cams"], pair)
        assert max(deg) <= 1e-5 and r["count"][p] == 68 and r["status"][p] == 0 and r["error"][p] <= 1e-6
    print("exact, %s, lens %s: the candidate nearest the truth is %.1e off in the median, the best pose of a well-conditioned hypothesis "
          "at most %.1e; %.1f real candidates a sample" % (method, lens, np.median(nearest), worst, hyp["roots"].mean()))
    assert np.median(nearest) <= 1e-9 and worst <= 1e-6 and (hyp["roots"][hyp["drawn"]] % 2 == 0).all()
    assert np.array_equal(r["cams"][:, 0, :4], c["truth_cams"][[0, 2], :4]) and np.array_equal(r["cams"][:, 1, :4], c["truth_cams"][[1, 1], :4])
    # the records are a rig of the pair in the gauge of view a
    assert (r["cams"][:, 0, 4:13] == np.eye(3).reshape(9)).all() and (r["cams"][:, 0, 13:] == 0.0).all()
    for p in range(2):
        R, t = r["rotation"][p], r["direction"][p]
        assert abs(np.linalg.norm(t) - 1.0) <= 1e-12 and np.abs(R @ R.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(R) - 1.0) <= 1e-12
        np.testing.assert_allclose(r["cams"][p, 1, 13:], -R.T @ t, atol=1e-15)


@pytest.fixture(scope="module")
def outliers():
    c = rp.outlier_case()
    return c, rp.run(c)


def test_winner_is_the_lexicographic_one(outliers):
    c, r = outliers
    for p in range(2):
        count, cost = r["scores"][p, :, 0], r["scores"][p, :, 1]
        ok = np.isfinite(cost)
        order = np.lexsort((np.arange(len(cost)), cost, -count))          # the last key is the first criterion
        assert ok.any() and r["best"][p] == order[ok[order]][0] == lc.winner(count, cost)
        assert r["count"][p] == count[r["best"][p]] and (count[~ok] == 0).all()
        np.testing.assert_array_equal(np.concatenate([r["rotation"][p].reshape(9), r["direction"][p]]), r["poses"][p, r["best"][p]])


def test_the_winners_of_the_outlier_case_lie_within_the_recorded_bounds(outliers):
    c, r = outliers
    both = ~c["planted"][:, [0, 2]] & ~c["planted"][:, [1, 3]]
    for p, pair in enumerate(c["pairs"]):
        rot, way = rp.pose_errors(r["rotation"][p], r["direction"][p], c["truth_cams"], pair)
        inl = r["inliers"][:, p].astype(bool)
        print("outlier case, pair %s: winner %d with %d inliers of %d clean correspondences, %d planted among them; rotation off by %.2f "
              "degrees, direction by %.2f; error %.2f px" % (pair, r["best"][p], r["count"][p], both[:, p].sum(), (inl & ~both[:, p]).sum(),
                                                             rot, way, r["error"][p]))
        assert r["status"][p] == 0 and r["count"][p] >= rp.MIN_INLIERS
        assert (inl & ~both[:, p]).sum() <= rp.WINNER_PLANTED and rot <= rp.WINNER_DEGREES[0] and way <= rp.WINNER_DEGREES[1]


@pytest.mark.parametrize("huber", [None, 6.0])
def test_the_restated_polish_from_the_winner_and_from_the_true_pose_agree(outliers, huber):
    c, r = outliers
    args = (c["pixels"], c["conf"], c["cams"], c["pairs"])
    truth = [rp.true_pose(c["truth_cams"], pair) for pair in c["pairs"]]
    a = rp.refine(*args, r["rotation"], r["direction"], c["dist"], huber, weight=r["inliers"])
    b = rp.refine(*args, np.stack([t[0] for t in truth]), np.stack([t[1] for t in truth]), c["dist"], huber, weight=r["inliers"])
    gap = max(np.abs(a["rotation"] - b["rotation"]).max(), np.abs(a["direction"] - b["direction"]).max())
    deg = [rp.pose_errors(a["rotation"][p], a["direction"][p], c["truth_cams"], pair) for p, pair in enumerate(c["pairs"])]
    print("huber %s: trials %s from the winners, %s from the truth; the poses agree to %.2e (recorded %.2e); %s degrees from the truth"
          % (huber, a["iterations"], b["iterations"], gap, rp.POLISH_SPREAD, np.round(deg, 2).tolist()))
    assert (a["status"] == 0).all() and (b["status"] == 0).all() and (a["cost"] <= a["cost0"]).all() and (a["used"] == r["count"]).all()
    assert rp.POLISH_SPREAD / 4.0 <= gap <= 4.0 * rp.POLISH_SPREAD
    for p in range(2):
        R, t = a["rotation"][p], a["direction"][p]
        assert abs(np.linalg.norm(t) - 1.0) <= 1e-12 and np.abs(R @ R.T - np.eye(3)).max() <= 1e-12


def test_the_analytic_jacobian_of_the_sampson_distance(outliers):
    c, r = outliers
    obs = rp.observations(c["pixels"], c["conf"], c["cams"], c["dist"], c["pairs"])
    ya, yb, w = obs["ya"][:, 0].reshape(-1, 2), obs["yb"][:, 0].reshape(-1, 2), obs["w"][:, 0].reshape(-1)
    pose = np.concatenate([r["rotation"][0].reshape(9), r["direction"][0]])
    ev = lambda q: rp.refine_evaluate(ya, yb, w, c["cams"][0], c["cams"][1], q)      # noqa: E731
    J, num = ev(pose)["J"], np.zeros((int((w > 0).sum()), 5))
    for k in range(5):
        step = np.zeros(5)
        step[k] = 1e-6
        num[:, k] = (ev(rp.apply_step(pose, step))["d"] - ev(rp.apply_step(pose, -step))["d"]) / 2e-6
    assert np.abs(num - J).max() <= 1e-9 * np.abs(J).max() + 1e-6        # central differences: O(h^2) and the rounding of d over h
    # the distances of the evaluation are those of the scorer
    s = rp.score(obs, c["cams"], c["pairs"], pose[None, None].repeat(2, axis=0), c["threshold"])
    np.testing.assert_allclose(ev(pose)["d"] ** 2, s["d2"][:, 0, 0].reshape(-1)[w > 0], rtol=1e-6, atol=1e-12)      # two orders of one cancellation


def test_statuses_of_the_restated_polish():
    c = rp.case(2, 2, 17, hypotheses=32)
    r = rp.run(c)
    args = (c["pixels"], c["conf"], c["cams"], c["pairs"])
    zero = rp.refine(*args, r["rotation"], r["direction"], c["dist"], max_iterations=0)
    assert zero["status"][0] == 2 and zero["iterations"][0] == 0 and zero["cost"][0] == zero["cost0"][0]
    assert np.array_equal(zero["rotation"], r["rotation"]) and np.array_equal(zero["direction"], r["direction"])
    nan = rp.refine(*args, np.full((1, 3, 3), np.nan), r["direction"], c["dist"])
    assert nan["status"][0] == 3 and np.isnan(nan["error"][0]) and np.isnan(nan["cost"][0])
    few = rp.few_case(5)
    r5 = rp.refine(few["pixels"], few["conf"], few["cams"], few["pairs"], r["rotation"], r["direction"], None)
    assert r5["status"][0] == 2 and r5["used"][0] == 5
    none = rp.refine(*args, r["rotation"], r["direction"], c["dist"], weight=np.zeros((2, 1, 17), np.float32))
    assert none["status"][0] == 3 and none["used"][0] == 0


def test_five_and_six_participants():
    five, six = rp.few_case(5), rp.few_case(6)
    r5, r6 = rp.run(five), rp.run(six)
    R, t, _ = rp.true_pose(five["truth_cams"], (0, 1))
    truth = np.concatenate([R.reshape(9), t])
    # five: every candidate of the one sample fits its five correspondences, so the best of them is a matter of rounding; the true
    # pose is among the candidates of the winner, and nothing is located for want of a sixth inlier
    assert r5["status"][0] == 3 and r5["count"][0] == 0 and r5["best"][0] >= 0
    drawn = r5["hyp"]["drawn"][0]                                    # with 5 of 17 slots taking part, 16 attempts do not always find the fifth
    assert 0 < drawn.sum() and (r5["scores"][0, drawn, 0] == 5).all() and (r5["scores"][0, ~drawn] == [0.0, np.inf]).all()
    assert np.isnan(r5["rotation"]).all() and np.isnan(r5["cams"][0, :, 4:]).all() and not r5["inliers"].any()
    cands = r5["hyp"]["candidates"]["poses"][0, r5["best"][0]]
    assert np.nanmin(rp.pose_gap(cands, truth)) <= 1e-4              # float32 pixels
    assert r6["status"][0] == 0 and r6["count"][0] == 6 and rp.pose_gap(np.concatenate([r6["rotation"][0].reshape(9), r6["direction"][0]]), truth) <= 1e-4
    four = rp.run(rp.few_case(4))
    assert four["status"][0] == 3 and four["best"][0] == -1 and (four["scores"][0] == [0.0, np.inf]).all() and (four["roots"] == 0).all()


# --------------------------------------------------------------------------------------- what the GPU comparisons rest on
@pytest.fixture(scope="module")
def gpu_runs():
    return {k: (c, rp.run(c), rp.run(c, method="poly")) for k, c in rp.gpu_cases().items()}


def test_gpu_cases_are_well_conditioned_and_clear_of_the_edges(gpu_runs):
    for name, (c, r, _) in gpu_runs.items():
        hyp = r["hyp"]
        share = hyp["well"].sum() / max(hyp["drawn"].sum(), 1)
        cs = hyp["cand_score"]
        t2 = c["threshold"] ** 2
        with np.errstate(all="ignore"):
            part = np.broadcast_to(hyp["obs"]["part"][:, :, None, :], cs["d2"].shape)
            near = np.abs(cs["d2"] / t2 - 1.0)[part & np.isfinite(cs["d2"])].min()
        P, H = hyp["drawn"].shape
        count, cost = cs["count"].reshape(P, H, -1), cs["cost"].reshape(P, H, -1)
        ties = 0
        for p in range(P):
            for h in range(H):
                k = hyp["best_candidate"][p, h]                      # the best candidate shares its (count, cost) with no other
                ties += k >= 0 and int(((count[p, h] == count[p, h, k]) & (cost[p, h] == cost[p, h, k])).sum()) != 1
        print("%-20s %4d hypotheses a pair: %5.1f %% drawn, %5.1f %% valid, %5.1f %% of the drawn well-conditioned; d^2 no nearer to the "
              "threshold than %.1e relative; %d ties" % (name, c["hypotheses"], 100.0 * hyp["drawn"].mean(), 100.0 * hyp["valid"].mean(),
                                                         100.0 * share, near, ties))
        assert share >= 0.9
        assert near > rp.NEAR_THRESHOLD and ties == 0


def test_two_float64_formulations_set_the_pose_tolerance(gpu_runs):
    worst = 0.0
    for name, (c, r, e) in gpu_runs.items():
        well = r["hyp"]["well"]
        assert np.array_equal(r["hyp"]["valid"][well], e["hyp"]["valid"][well])          # the two agree on which hypotheses are void
        assert np.array_equal(r["roots"][well], e["roots"][well])                        # and on the number of real candidates
        both = well & r["hyp"]["valid"] & e["hyp"]["valid"] & ~r["hyp"]["tied"]       # tied: which candidate is best is rounding
        if both.any():
            d = float(rp.pose_gap(r["poses"], e["poses"])[both].max())
            print("%-20s action matrix against Nister's polynomial: the best poses differ by up to %.2e over %d hypotheses" % (name, d, both.sum()))
            worst = max(worst, d)
    print("the spread over the case set: %.2e; recorded %.2e, the device is allowed %.2e" % (worst, rp.FORMULATION_SPREAD, rp.POSE_TOL))
    # the recorded figure is the measured one: within a factor of 4 either way, which is the room another LAPACK build's rounding
    # gets (the figure is a maximum of rounding errors, not a constant of nature)
    assert rp.FORMULATION_SPREAD / 4.0 <= worst <= 4.0 * rp.FORMULATION_SPREAD and rp.POSE_TOL == 100.0 * rp.FORMULATION_SPREAD


def test_the_two_root_finders_agree_without_the_polish(monkeypatch):
    """Both formulations polish (x, y, z) on the same cubics, which would hide a defect of either root finder.  Without the polish
    the action matrix's eigenvectors and the roots of Nister's polynomial are two independent routes: where the roots are well
    apart (0.1) and both eliminations have pivots of at least 1e-3 of the largest -- without the polish a pair of candidates with
    nearly the same z is up to 1e-4 off --, they give the same best pose to the spread of the polished ones"""
    monkeypatch.setattr(rp, "POLISH", 0)
    worst, n = 0.0, 0
    for name, c in rp.gpu_cases().items():
        if name.startswith("small_h") and name != "small_h256":
            continue
        r, e = rp.run(c), rp.run(c, method="poly")
        cand = r["hyp"]["candidates"]
        both = r["hyp"]["well"] & e["hyp"]["well"] & r["hyp"]["valid"] & e["hyp"]["valid"] & ~r["hyp"]["tied"] & (cand["sep"] >= 0.1) & \
            (cand["ratio"] >= 1e-3)
        n += int(both.sum())
        worst = max(worst, float(rp.pose_gap(r["poses"], e["poses"])[both].max()) if both.any() else 0.0)
    print("without the polish: the best poses of %d well-separated hypotheses differ by up to %.2e" % (n, worst))
    assert n >= 500 and worst <= 4.0 * rp.FORMULATION_SPREAD


def test_swapped_pair_is_the_inverse_pose():
    c = rp.case(4, 2, 17, pairs=((0, 1), (1, 0)), noise=0.0, exact=True, hypotheses=8)
    r = rp.run(c)
    R01, t01, R10, t10 = r["rotation"][0], r["direction"][0], r["rotation"][1], r["direction"][1]
    assert np.abs(R10 - R01.T).max() <= 1e-6 and np.abs(t10 + R01.T @ t01).max() <= 1e-6


# ------------------------------------------------------------------------------------------------------- the Python surface
def test_argument_checks_raise_before_any_device_is_touched():
    from openmpl_amd import relative_pose
    B, V, J = 2, 3, 5
    X, Cf = torch.zeros(B, V, J, 2), torch.ones(B, V, J)
    Cm, D = torch.zeros(V, 16, dtype=torch.float64), torch.zeros(V, 5, dtype=torch.float64)
    with pytest.raises(RuntimeError, match=r"pixels: expected shape \(B,V,J,2\)"):
        relative_pose(X[..., :1], Cf, Cm)
    with pytest.raises(RuntimeError, match=r"conf: expected shape \(2, 3, 5\)"):
        relative_pose(X, Cf[:, :2], Cm)
    with pytest.raises(RuntimeError, match=r"float32 tensors required \(pixels is torch.float64\)"):
        relative_pose(X.double(), Cf, Cm)
    with pytest.raises(RuntimeError, match="no CPU path: pixels must live on a GPU"):
        relative_pose(X, Cf, Cm, distortion=D)
    for bad in (0.0, -1.0, float("nan"), float("inf"), None):
        with pytest.raises(RuntimeError, match="threshold must be a positive finite number"):
            relative_pose(X, Cf, Cm, threshold=bad)
        with pytest.raises(RuntimeError, match="baseline must be a positive finite length"):
            relative_pose(X, Cf, Cm, baseline=bad)
    for bad in (0, -1, 65537, 2.5, True, None, "8"):
        with pytest.raises(RuntimeError, match="hypotheses must be an integer"):
            relative_pose(X, Cf, Cm, hypotheses=bad)
    for bad in (1.5, None, "0"):
        with pytest.raises(RuntimeError, match="seed must be an integer"):
            relative_pose(X, Cf, Cm, seed=bad)
    for bad in (((0, 0),), ((0, 3),), ((-1, 0),), ((0, 1.0),), ((True, 0),), ((0, 1, 2),), ((0,),)):
        with pytest.raises(RuntimeError, match=r"pairs holds two distinct view indices, integers in \[0, 2\]"):
            relative_pose(X, Cf, Cm, pairs=bad)
    with pytest.raises(RuntimeError, match="pairs must be a sequence"):
        relative_pose(X, Cf, Cm, pairs=1)
    with pytest.raises(RuntimeError, match="between 1 and 32 pairs"):
        relative_pose(X, Cf, Cm, pairs=((0, 1),) * 33)
    with pytest.raises(RuntimeError, match="between 1 and 32 pairs"):
        relative_pose(X, Cf, Cm, pairs=())
    with pytest.raises(RuntimeError, match="huber is an option of the refinement"):
        relative_pose(X, Cf, Cm, huber=6.0)
    with pytest.raises(RuntimeError, match="huber must be a positive finite number"):
        relative_pose(X, Cf, Cm, refine=True, huber=-1.0)
    with pytest.raises(RuntimeError, match="no CPU path"):                         # good options get as far as the devices
        relative_pose(X, Cf, Cm, pairs=[(0, 2), (2, 1)], threshold=4, hypotheses=8, seed=7, baseline=2.5, refine=True, huber=6.0)
    from openmpl_amd import refine_relative_pose
    R, t = torch.zeros(1, 3, 3, dtype=torch.float64), torch.zeros(1, 3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="pairs holds two distinct view indices"):
        refine_relative_pose(X, Cf, Cm, ((1, 1),), R, t)
    with pytest.raises(RuntimeError, match="max_iterations must be an integer"):
        refine_relative_pose(X, Cf, Cm, ((0, 1),), R, t, max_iterations=-1)
    with pytest.raises(RuntimeError, match="step_tolerance must be"):
        refine_relative_pose(X, Cf, Cm, ((0, 1),), R, t, step_tolerance=-1.0)
    with pytest.raises(RuntimeError, match="baseline must be"):
        refine_relative_pose(X, Cf, Cm, ((0, 1),), R, t, baseline=0.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        refine_relative_pose(X, Cf, Cm, ((0, 1),), R, t, huber=6.0)
