"""Sub-pixel decoding (decode_heatmaps(subpixel=...)): the properties of the two estimators on their numpy restatement
(tests/render_cases.py), the accuracy table that motivated them, and the recorded behaviour of the reference's
find_tensor_peak_batch, which both must beat.  No GPU."""
import numpy as np
import pytest

from tests import heatmap_cases as hc
from tests import render_cases as rc


def _err(coords, means):
    return np.abs(coords.astype(np.float64) - means)


def test_gaussian_recovers_clean_float32_means():
    """the log-quadratic fit is exact for a Gaussian of any sigma; on float32 maps what is left is the rounding of the three values
    (6e-8 relative, a few 1e-7 cell) and of the coordinate itself (half an ulp of 64: 1.9e-6)"""
    means, clean, _ = rc.probe_maps(300)
    r = rc.refine(clean.astype(np.float32), "gaussian")
    assert r["refined"].all() and rc.well_conditioned(r, "gaussian")
    assert _err(r["coords"], means).max() <= 1e-5
    for sigma in (1.0, 3.0):
        hm = hc.gaussian(64, 64, means[:50, 0], means[:50, 1], 0.7, sigma)
        assert _err(rc.refine(hm, "gaussian")["coords"], means[:50]).max() <= 1e-5


def test_centroid_is_exact_on_a_window_symmetric_map():
    hm = np.zeros((3, 16, 12), np.float32)
    for n, (x0, y0) in enumerate(((5, 7), (2, 2), (9, 13))):
        for i in range(-2, 3):
            for j in range(-2, 3):
                hm[n, y0 + j, x0 + i] = 1.0 / (1 + i * i + 2 * j * j)
    for radius in (1, 2):
        r = rc.refine(hm, "centroid", radius)
        assert np.array_equal(r["coords"], np.float32([[5, 7], [2, 2], [9, 13]]))
    # and where it is not symmetric the centroid is the weights' mean: 1 at the peak, 0.5 to its right, 0.25 below
    two = np.zeros((1, 8, 8), np.float32)
    two[0, 3, 4], two[0, 3, 5], two[0, 4, 4] = 1.0, 0.5, 0.25
    c = rc.refine(two, "centroid", 1)["coords"][0]
    assert c[0] == np.float32(4 + 0.5 / (1.75 + 2.22e-16)) and c[1] == np.float32(3 + 0.25 / (1.75 + 2.22e-16))
    c = rc.refine(two, "centroid", 1, threshold=0.3)["coords"][0]                     # F.threshold: 0.25 no longer counts
    assert c[0] == np.float32(4 + 0.5 / (1.5 + 2.22e-16)) and c[1] == 3.0
    c = rc.refine(two[:, :, :6], "centroid", 3)["coords"][0]                          # the window leaves the map: zeros
    assert c[0] == np.float32(4 + 0.5 / (1.75 + 2.22e-16))


@pytest.mark.parametrize("subpixel,radius", [("gaussian", 2), ("centroid", 2), ("centroid", 6)])
def test_shift_equivariance_by_whole_cells(subpixel, radius):
    """a map moved by whole cells, away from the borders, moves its estimate by exactly those cells: the float64 offset is the
    same, and the one rounding of x0 + d is all that may differ (np.roll moves the values themselves, so nothing else does)"""
    from openmpl_amd import detrng
    mx, my = detrng.uniform(2, "shift.mx", (8,), 28.0, 36.0), detrng.uniform(2, "shift.my", (8,), 28.0, 36.0)
    hm = np.zeros((8, 64, 64), np.float32)                              # all of the map's weight lies in the middle: a whole-cell
    hm[:, 20:44, 20:44] = (hc.gaussian(64, 64, mx, my, 0.8) + detrng.uniform(2, "shift.noise", (8, 64, 64), 0.0, 0.004))[:, 20:44, 20:44]
    base = rc.refine(hm, subpixel, radius)["coords"].astype(np.float64)
    for sx, sy in ((5, -3), (-11, 9), (0, 14)):
        moved = rc.refine(np.roll(hm, (sy, sx), axis=(1, 2)), subpixel, radius)["coords"].astype(np.float64)
        assert (np.abs(moved - base - np.array([sx, sy])) <= np.spacing(np.float32(32.0))).all()
        assert (moved != np.round(moved)).any()


def test_rules_on_special_and_edge_maps():
    """a refinement applies only where 0 < maxval < inf; elsewhere the plain decode's coordinates; the log-quadratic offset is 0
    on the border's axis and beside a neighbour that is not positive"""
    for H, W in ((64, 64), (5, 7)):
        s = dict(zip(hc.SPECIAL, hc.special_maps(H, W)))
        inf = s["two_maxima"].copy()
        inf[H // 2, W // 2] = np.inf
        for subpixel in ("gaussian", "centroid"):
            for k in ("all_zero", "all_negative", "signed_zeros", "nan", "nan_neighbour", "all_neg_inf"):
                r = rc.refine(s[k][None], subpixel)
                assert not r["refined"].any() and not r["coords"].any(), k
            r = rc.refine(inf[None], subpixel)
            assert not r["refined"].any() and np.array_equal(r["coords"][0], np.float32([W // 2, H // 2]))
            r = rc.refine(s["two_maxima"][None], subpixel)
            assert r["refined"].all() and np.isfinite(r["coords"]).all()
        e = rc.refine(hc.edge_maps(H, W), "gaussian")
        plain = hc.decode(hc.edge_maps(H, W))["coords"]
        on_border = (plain == 0) | (plain == np.float32([W - 1, H - 1]))
        assert np.array_equal(e["coords"][on_border], plain[on_border])
        assert (e["coords"][~on_border] != plain[~on_border]).all() and (np.abs(e["coords"] - plain) <= 0.5).all()
    hole = hc.gaussian(8, 8, 4.2, 3.8, 1.0)
    hole[4, 3] = 0.0                                                    # left of the peak at (4, 4): no offset in x, one in y
    c = rc.refine(hole[None], "gaussian")["coords"][0]
    assert c[0] == 4.0 and abs(c[1] - 3.8) < 1e-5
    flat = np.full((1, 4, 4), 0.5, np.float32)                          # the peak is the first maximum, so a + b > 0 wherever both
    flat[0, 0, :] = flat[0, :, 0] = 0.4                                 # neighbours count; the extreme is a = 0: half a cell
    assert np.array_equal(rc.refine(flat, "gaussian")["coords"][0], np.float32([1.5, 1.5]))


# the issue's probe: per-axis error in cells, worst / mean, of 4000 Gaussians (sigma 2, amplitude 0.2 .. 1, means 3 cells inside)
TABLE = {"clean fp32": ((0.250, 0.125), (0.0000, 0.0000), (0.114, 0.037), (0.172, 0.008)),
         "clean bf16": ((0.272, 0.123), (0.024, 0.005), (0.113, 0.037), (0.172, 0.008)),
         "+ U(0, 0.004) fp32": ((0.291, 0.125), (0.056, 0.008), (0.119, 0.039), (0.188, 0.012)),
         "+ U(0, 0.02) fp32": ((0.576, 0.133), (0.328, 0.040), (0.234, 0.052), (0.239, 0.026))}


def test_the_probe_table_is_reproduced():
    """The table was probed with a throwaway sketch on other random maps and printed to three decimals.  A mean is a statistic of
    8000 axes (its standard error is under 1 % of the figure): reproduced when within 10 % of the table's figure or within 0.0005,
    half a unit of the table's last digit.  A worst case is the tail of another draw: within 30 %, or 0.0005.  The two figures the
    table gives as 0.0000 must themselves print as 0.0000: below 0.00005."""
    means, clean, u = rc.probe_maps(4000)
    rows = {"clean fp32": (clean.astype(np.float32), 1e-6), "clean bf16": (rc.round_once(clean, "bf16").astype(np.float32), 1e-6),
            "+ U(0, 0.004) fp32": ((clean + 0.004 * u).astype(np.float32), 0.004), "+ U(0, 0.02) fp32": ((clean + 0.02 * u).astype(np.float32), 0.02)}
    print("\n%-20s | %-15s | %-15s | %-15s | %s" % ("maps", "quarter shift", "log-quadratic", "centroid r=4", "centroid r=6, threshold = noise"))
    for name, (hm, level) in rows.items():
        got = [_err(hc.decode(hm, post_process=True)["coords"], means), _err(rc.refine(hm, "gaussian")["coords"], means),
               _err(rc.refine(hm, "centroid", 4)["coords"], means), _err(rc.refine(hm, "centroid", 6, level)["coords"], means)]
        print("%-20s | %s" % (name, " | ".join("%.4f / %.4f  " % (e.max(), e.mean()) for e in got)))
        for e, (worst, mean) in zip(got, TABLE[name]):
            if worst == 0.0:
                assert e.max() < 0.00005, (name, e.max())
                continue
            assert abs(e.mean() - mean) <= max(0.1 * mean, 0.0005), (name, e.mean(), mean)
            assert abs(e.max() - worst) <= max(0.3 * worst, 0.0005), (name, e.max(), worst)
        del got


def test_both_estimators_beat_the_recorded_find_tensor_peak_batch():
    """tests/golden/subpixel.npz: what the reference's function returns in place on 500 clean Gaussians, 0.17 (x) and 0.36 (y)
    cells off on average at radius 2 -- worse than the quarter shift.  It is a record to compare with, not an oracle."""
    g = rc.golden_subpixel()
    means = np.stack([g["mx"], g["my"]], -1).astype(np.float64)
    hm = hc.gaussian(64, 64, g["mx"], g["my"], g["amp"])
    assert len(means) == 500
    for radius in (2, 6):
        ref = _err(g["r%d" % radius], means).mean(0)
        gauss = _err(rc.refine(hm, "gaussian")["coords"], means).mean(0)
        cen = _err(rc.refine(hm, "centroid", radius)["coords"], means).mean(0)
        print("radius %d, mean |error| in cells (x, y): reference %s, gaussian %s, centroid %s" % (radius, ref.round(4), gauss.round(7), cen.round(4)))
        assert (gauss < ref).all() and (cen < ref).all()
    assert _err(g["r2"], means).mean() > 0.125                          # the quarter shift's mean
