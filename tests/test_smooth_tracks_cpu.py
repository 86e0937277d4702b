"""The float64 restatement of smooth_tracks (tests/smooth_tracks_cases.py) against what can be said without a device: closed forms,
the gradient at its minimiser, the cost trace of the IRLS loop, the statuses of the degenerate cases, the distance between its two
formulations, and the accuracy condition that fixes the smoothness the documents quote."""
import os
import re

import numpy as np
import pytest

from tests import smooth_tracks_cases as sc


def test_the_binding_states_the_thresholds_of_the_header():
    from openmpl_amd import cabi
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mpl_hip.h")).read()
    val = lambda name: eval(re.search(r"#define %s (.+?)\s*(/\*|$)" % name, text, re.M).group(1).rstrip("u"))      # noqa: E731
    assert val("MPL_SMOOTH_LANES") == cabi.SMOOTH_LANES and val("MPL_SMOOTH_SINGLE_MAX") == cabi.SMOOTH_SINGLE_MAX
    assert val("MPL_SMOOTH_CHUNK_MIN") == cabi.SMOOTH_CHUNK_MIN and val("MPL_SMOOTH_MAX_SEGMENT") == cabi.SMOOTH_MAX_SEGMENT
    assert val("MPL_SMOOTH_MAX_FRAMES") == cabi.SMOOTH_MAX_FRAMES and val("MPL_SMOOTH_MAX_JOINTS") == cabi.SMOOTH_MAX_JOINTS
    assert val("MPL_SMOOTH_F_SINGLE_LANE") == cabi.SMOOTH_F_SINGLE_LANE
    for t in cabi.smooth_thresholds():
        assert {t - 1, t, t + 1} <= set(sc.LENGTHS)
    assert sc.chunking(cabi.SMOOTH_SINGLE_MAX) == (cabi.SMOOTH_SINGLE_MAX, 1) and sc.chunking(cabi.SMOOTH_SINGLE_MAX + 1)[1] > 1
    assert sc.chunking(512) == (8, 64) and sc.chunking(513) == (9, 57) and sc.chunking(65536) == (1024, 64)


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("gaps", ["none", "ends9", "middle40", "every_second", "all_but_two"])
def test_the_null_space_comes_back_unchanged(order, gaps):
    """a straight line under order 2 and a constant under order 1 have no penalty: they are the minimiser whatever the smoothness,
    and the gaps are filled with the line"""
    T = 130
    t = np.arange(T, dtype=np.float64)[:, None]
    line = np.array([0.25, -1.0, 3.0]) + (t * np.array([0.01, -0.02, 0.005]) if order == 2 else 0.0 * t)
    w = np.where(sc.gap_mask(T, gaps), 0.0, 1.5)
    for lam in sc.SMOOTHNESS:
        for huber in (None, sc.HUBER):
            for solver in ("dense", "banded"):
                r = sc.smooth_track(line, w, lam, order, huber, solver=solver)
                assert r["status"] == sc.CONVERGED and np.abs(r["points"] - line).max() <= 1e-9 * np.abs(line).max(), (lam, huber, solver)
                assert r["cost"] <= 1e-16 * lam + 1e-20


def test_the_gradient_vanishes_at_the_minimiser():
    worst = 0.0
    for name, ckw, kw in sc.grid()[::7]:
        c, kw, ref = sc.reference(name)
        if kw["huber"]:
            continue                                   # the IRLS fixed point is reached to step_tolerance only
        t0 = 0
        for n in c["segments"]:
            for j in range(c["J"]):
                Y = c["points"][t0:t0 + n, j].astype(np.float64)
                w = np.ones(n) if c["weight"] is None else c["weight"][t0:t0 + n, j].astype(np.float64)
                if ref["passed"][t0, j]:
                    continue
                X = ref["points"][t0:t0 + n, j]
                g = sc.gradient(X, Y, w, kw["smoothness"], kw["order"], 0.0)
                part = sc.takes_part(Y, w)
                scale = 2.0 * (np.where(part, w, 0.0).max() + 16.0 * kw["smoothness"]) * max(np.abs(X).max(), 1.0)
                worst = max(worst, float(np.abs(g).max() / scale))
            t0 += n
    print("largest |dE/dX| at the minimiser over the scale of its terms: %.2e" % worst)
    assert worst <= 1e-9


def test_the_cost_trace_never_rises_and_the_final_cost_is_below_the_first():
    for name, ckw, kw in sc.grid():
        c, kw, ref = sc.reference(name)
        assert (ref["cost"] <= ref["cost0"]).all(), name
        if not kw["huber"] or c["T"] > 300:
            continue
        for j in range(min(c["J"], 2)):
            n = c["segments"][0]
            trace = []
            sc.smooth_track(c["points"][:n, j], None if c["weight"] is None else c["weight"][:n, j], kw["smoothness"], kw["order"], kw["huber"],
                            trace=trace)
            assert all(b < a for a, b in zip(trace, trace[1:])), (name, trace)


def test_statuses_of_the_degenerate_cases():
    T = 12
    Y = sc.sinusoids(T, 1)[1][:, 0]
    none, one, two = np.zeros(T), np.zeros(T), np.zeros(T)
    one[4] = 1.0
    two[[2, 9]] = 1.0
    for huber in (None, sc.HUBER):
        for order, want in ((1, (2, 0, 0)), (2, (2, 2, 0))):
            for w, st in zip((none, one, two), want):
                r = sc.smooth_track(Y, w, 1.0, order, huber)
                assert r["status"] == st, (order, w, r["status"])
                if st == sc.PASSED_THROUGH:
                    assert np.array_equal(r["points"], Y) and r["cost"] == 0 and r["cost0"] == 0 and r["iterations"] == 0
                    assert np.array_equal(r["residual"][w > 0], np.zeros(int((w > 0).sum()))) and np.isnan(r["residual"][w == 0]).all()
        r = sc.smooth_track(Y, None, 1.0, 2, huber, max_iterations=0)
        assert r["status"] == sc.PASSED_THROUGH and np.array_equal(r["points"], Y)
        r = sc.smooth_track(Y, None, 1.0, 2, huber, max_iterations=1)
        assert r["status"] == (sc.CAPPED if huber else sc.CONVERGED) and r["iterations"] == 1
    # one frame: order 1 solves it, order 2 passes it through; an extent of zero converges at once under the Huber cost
    assert sc.smooth_track(Y[:1], None, 1.0, 1)["status"] == sc.CONVERGED and sc.smooth_track(Y[:1], None, 1.0, 2)["status"] == sc.PASSED_THROUGH
    flat = np.tile(Y[:1], (T, 1))
    r = sc.smooth_track(flat, None, 1.0, 2, sc.HUBER)
    assert r["status"] == sc.CONVERGED and r["iterations"] == 1
    # a gap is interpolated: linearly at order 1
    w = np.ones(T)
    w[3:8] = 0.0
    r = sc.smooth_track(np.arange(T)[:, None] * np.ones(3) + 0.0, w, 1e-2, 1)
    assert np.abs(np.diff(r["points"][2:9, 0], n=2)).max() <= 1e-9


def test_the_two_formulations_agree():
    """their distance over the grid, printed: the yardstick of the measured parity on the device"""
    worst, at = 0.0, None
    for name, ckw, kw in sc.grid():
        d = sc.formulation_distance(sc.case(**ckw), **kw)
        if d > worst:
            worst, at = d, name
    print("largest max-scaled distance between the dense and the banded formulation: %.3e at %s" % (worst, at))
    assert worst <= 1e-7                               # cond(A) eps at smoothness 1e4: far below the 1e-4 of the parity rule


def test_accuracy_of_the_restatement():
    """T = 512, noise 0.01, 5 % outlier frames, 10 % gaps on tracks one unit across: order 2 with the Huber cost brings the mean error
    over ALL frames, gaps included, below the mean error of the raw input at its valid frames.  Measured: 0.0073 against 0.0470"""
    c = sc.accuracy_case()
    r = sc.smooth(c["points"], c["weight"], c["segments"], smoothness=sc.ACCURACY_SMOOTHNESS, order=2, huber=sc.HUBER)
    part = np.isfinite(c["points"]).all(-1) & (c["weight"] > 0)
    after = float(np.linalg.norm(r["points"] - c["truth"], axis=-1).mean())
    before = float(np.linalg.norm(c["points"].astype(np.float64) - c["truth"], axis=-1)[part].mean())
    print("accuracy: mean error at all frames after smoothing %.5f, of the raw input at its valid frames %.5f" % (after, before))
    assert 0.07 <= (~part).mean() <= 0.13             # one draw of 512 frames at 10 %
    assert after < 0.5 * before
