"""triangulate_rays_robust on the GPU (openmpl_amd/geometry.py, triangulate_robust_kernel of csrc/geometry.hip) against the float64
restatement of tests/robust_tri_cases.py and the selections of the reference's own triangulate_poses.

`inliers` is compared exactly: the cases carry margins (robust_tri_cases.outlier_case asserts them) no fp64 rounding can cross.
`points` and `residual` fall under the parity rule of DESIGN.md section 2, max|d| <= 1e-4 max|ref| and ||d||_2 <= 1e-4 ||ref||_2,
NaN in the same places; the kernel computes in fp64 and rounds once to fp32, so it sits near 1e-7.  Repeated runs and other
batchings are compared bitwise.  Before every assertion on an error the figures are printed (pytest -s shows them).
"""
import functools

import numpy as np
import pytest
import torch

from tests import geometry_cases as gc
from tests import robust_tri_cases as rc
from tests import synth_cases as sc

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _dev(arrays):
    return None if arrays is None else [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _np(t):
    return t.detach().cpu().numpy()


def _run(*args, **kw):
    from openmpl_amd import triangulate_rays_robust
    return tuple(_np(t) for t in triangulate_rays_robust(*args, **kw))


def _assert_parity(got, ref, what):
    mx, nw = gc.rel_errors(got, ref)
    print("%s: max-scaled %.3e norm-wise %.3e" % (what, mx, nw))
    assert mx <= TOL and nw <= TOL, "%s: max-scaled %.3e norm-wise %.3e (tol %.0e)" % (what, mx, nw, TOL)


def _flat(case):
    return [case["conf"][v] for v in range(len(case["rays"]))]


def _poses(flat, seed=0):
    rs = np.random.RandomState(seed)
    return [np.concatenate([rs.randn(*c.shape, 2).astype(np.float32) * 50, c[..., None]], axis=-1) for c in flat]      # x, y, conf


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


# (B,V,J), redirected views per item: one pair; 85 items across a 64-item tile; the headline rig; more pairs than waves, one
# item; 496 pairs at MPL_MAX_VIEWS; two full tiles at 64 joints
SHAPES = [((3, 2, 17), 0), ((5, 3, 17), 1), ((3, 4, 17), 1), ((2, 5, 1), 1), ((1, 32, 3), 8), ((2, 5, 64), 1)]


@functools.lru_cache(maxsize=None)
def _case(shape, n_out):
    B, V, J = shape
    return rc.outlier_case(B, V, J, n_out=n_out, seed=3, n_zero=max(1, B * V * J // 25))


@pytest.mark.parametrize("shape,n_out", SHAPES)
def test_parity_with_the_restatement(shape, n_out):
    B, V, J = shape
    case = _case(shape, n_out)
    print("margins (conf, conf_threshold, distance, cost):", case["margins"])
    rays, centers, flat = _dev(case["rays"]), _dev(case["centers"]), _flat(case)
    poses = _poses(flat, seed=B + V + J)
    marked = 0
    for name, conf, conf_np, cth in (("none", None, None, None), ("(B,J)", _dev(flat), flat, None), ("(B,J) sel", _dev(flat), flat, 0.5),
                                     ("(B,J,3) sel", _dev(poses), poses, 0.5)):
        what = "B%d V%d J%d conf %s" % (B, V, J, name)
        (x, res, inl), n = _launches(lambda: _run(rays, centers, conf, threshold=case["tau"], conf_threshold=cth))
        assert n == 1 and x.shape == (B, J, 3) and res.shape == (B, J) and inl.shape == (B, V, J) and inl.dtype == np.float32, what
        x_ref, r_ref, i_ref = rc.robust(case["rays"], case["centers"], conf_np, case["tau"], cth)
        assert np.array_equal(inl, i_ref), what
        _assert_parity(x, x_ref, "points " + what)
        _assert_parity(res, r_ref, "residual " + what)
        assert np.array_equal(np.isnan(res), inl.sum(axis=1) == 0) and (inl.sum(axis=1)[~np.isnan(res)] >= 2).all(), what
        marked += int(((inl == 0) & case["out"]).sum())
    assert n_out == 0 or marked > 0.9 * 4 * case["out"].sum()            # the case does what it is there for
    from openmpl_amd import cabi
    assert not cabi.device_error()


def test_off_switches_are_triangulate_rays_and_inliers_reproduce_the_points():
    from openmpl_amd import triangulate_rays
    shape, n_out = SHAPES[1]
    B, V, J = shape
    case = _case(shape, n_out)
    rays, centers = _dev(case["rays"]), _dev(case["centers"])
    flat = [c.copy() for c in _flat(case)]
    flat[0][0, 1], flat[1][0, 2], flat[2][1, 3] = np.nan, -1.0, np.inf
    flat[0][2, 0] = flat[1][2, 0] = 0.0                                  # one view left
    for name, conf_np in (("none", None), ("(B,J)", flat), ("(B,J,3)", _poses(flat))):
        conf = _dev(conf_np)
        x, res, inl = _run(rays, centers, conf)
        p0, r0 = (_np(t) for t in triangulate_rays(rays, centers, conf))
        _assert_parity(x, p0, "both stages off, points, conf " + name)
        _assert_parity(res, r0, "both stages off, residual, conf " + name)
        part = np.transpose(rc.participation(gc.confidence(conf_np, V, B, J)), (1, 0, 2)) & ~np.isnan(r0)[:, None]
        assert np.array_equal(inl, part.astype(np.float32)), name
        assert (conf_np is None) == (not np.isnan(res).any())
        # the inliers handed back as weights reproduce the robust points
        x, res, inl = _run(rays, centers, conf, threshold=case["tau"])
        w = [torch.from_numpy(np.ascontiguousarray(inl[:, v] * (1.0 if conf_np is None else np.nan_to_num(flat[v], nan=0.0, posinf=0.0)))
                              .astype(np.float32)).cuda() for v in range(V)]
        p1, r1 = (_np(t) for t in triangulate_rays(rays, centers, w))
        _assert_parity(p1, x, "conf * inliers through triangulate_rays, points, conf " + name)
        _assert_parity(r1, res, "conf * inliers through triangulate_rays, residual, conf " + name)


@pytest.mark.parametrize("tag", ["v2", "v4", "v8"])
def test_selection_matches_the_reference_golden(tag):
    g = rc.golden_select()
    confs, starts, sel = g[tag + "_confs"], g[tag + "_starts"], g[tag + "_sel"]
    V, J = confs.shape
    S = len(starts)
    case = gc.ring_case(S, V, J, seed=2)
    rays, centers = _dev(case["rays"]), _dev(case["centers"])
    conf_np = [np.repeat(confs[v][None], S, axis=0) for v in range(V)]
    part = rc.participation(confs.astype(np.float64))
    for s, start in enumerate(starts):
        want = sel[s] & part                                             # the recorded set minus the views that never take part
        want &= want.sum(axis=0) >= 2
        for name, conf in (("(B,J)", _dev(conf_np)), ("(B,J,3)", _dev(_poses(conf_np)))):
            x, res, inl = _run(rays, centers, conf, conf_threshold=float(start))
            for b in range(S):                                           # every sample carries the same confidences
                assert np.array_equal(inl[b], want.astype(np.float32)), (tag, start, name, b)
            assert np.array_equal(np.isnan(res[0]), want.sum(axis=0) == 0)
            x_ref, r_ref, i_ref = rc.robust(case["rays"], case["centers"], conf_np, conf_threshold=float(start))
            assert np.array_equal(inl, i_ref)
            _assert_parity(x, x_ref, "golden %s start %.2f conf %s: points" % (tag, start, name))


def _only_these_are_nan(x, res, inl, base, at):
    nan = np.zeros(res.shape, bool)
    for b, j in at:
        nan[b, j] = True
    assert np.array_equal(np.isnan(res), nan) and np.array_equal(np.isnan(x).all(axis=-1), nan)
    assert np.array_equal(np.isnan(x).any(axis=-1), nan)
    assert not inl[:, :].transpose(0, 2, 1)[nan].any()                   # the item's row is all 0
    for got, ref in zip((x, res), base[:2]):
        assert np.array_equal(got[~nan], ref[~nan])                      # bitwise
    assert np.array_equal(inl.transpose(0, 2, 1)[~nan], base[2].transpose(0, 2, 1)[~nan])


def test_nan_cases_stay_in_their_item():
    shape, n_out = SHAPES[2]
    B, V, J = shape
    case = _case(shape, n_out)
    rays, centers = _dev(case["rays"]), _dev(case["centers"])
    tau = case["tau"]
    ones = [np.ones((B, J), np.float32) for _ in range(V)]
    base = _run(rays, centers, _dev(ones), threshold=tau)
    assert not np.isnan(base[1]).any()
    conf = [c.copy() for c in ones]
    for v in range(V):
        conf[v][0, 3] = 0.0                                              # all confidences 0
        conf[v][2, 16] = 0.0 if v else 1.0                               # one view
    _only_these_are_nan(*_run(rays, centers, _dev(conf), threshold=tau), base, [(0, 3), (2, 16)])
    _only_these_are_nan(*_run(rays, centers, _dev(conf)), _run(rays, centers, _dev(ones)), [(0, 3), (2, 16)])
    # min_inliers above the reachable count: V - 1 good views in every item
    count = base[2].sum(axis=1)
    assert count.max() <= V - n_out and (count == V - n_out).any()
    x, res, inl = _run(rays, centers, _dev(ones), threshold=tau, min_inliers=V)
    assert np.isnan(x).all() and np.isnan(res).all() and not inl.any()
    x, res, inl = _run(rays, centers, _dev(ones), threshold=tau, min_inliers=V - n_out)
    _only_these_are_nan(x, res, inl, base, list(zip(*np.nonzero(count < V - n_out))))
    # two exactly parallel lines (dyadic numbers: r - c is exact): the only pair of item (1, 7) is degenerate
    two = gc.ring_case(B, 2, J, seed=8)
    c0, c1 = np.array([1.5, -2.25, 0.5]), np.array([-3.0, 1.75, 2.5])
    two["centers"][0][1, 0], two["centers"][1][1, 0] = c0, c1
    ra, ca = _dev(two["rays"]), _dev(two["centers"])
    wide = 10.0                                                          # no midpoint of this case is that far from its lines
    base2 = _run(ra, ca, threshold=wide)
    assert not np.isnan(base2[1]).any() and (base2[2] == 1).all()
    d = np.array([0.5, 1.0, 0.25])
    two["rays"][0][1, 7], two["rays"][1][1, 7] = c0 + d, c1 - 2 * d
    assert np.array_equal(two["rays"][0][1, 7].astype(np.float64) - c0, d)
    assert np.array_equal(two["rays"][1][1, 7].astype(np.float64) - c1, -2 * d)
    for kw in (dict(threshold=wide), dict()):
        got = _run(_dev(two["rays"]), ca, **kw)
        _only_these_are_nan(*got, base2 if kw else _run(ra, ca), [(1, 7)])
    from openmpl_amd import cabi
    assert not cabi.device_error()


def test_batch_invariance_and_determinism_are_bitwise():
    B, V, J = 70, 4, 17
    case = rc.outlier_case(B, V, J, n_out=1, seed=5, configs=((True, 0.5),))
    flat = _flat(case)

    def run(lo, hi):
        cut = lambda lst: _dev([a[lo:hi] for a in lst])      # noqa: E731
        return _run(cut(case["rays"]), cut(case["centers"]), cut(flat), threshold=case["tau"], conf_threshold=0.5)

    a, b = run(0, B), run(0, B)
    parts = [np.concatenate(p) for p in zip(run(0, 1), run(1, B))]
    for x, y, z in zip(a, b, parts):
        assert np.array_equal(x, y, equal_nan=True) and np.array_equal(x, z, equal_nan=True)
    assert np.isfinite(a[1]).any() and (a[2] == 0).any()


def test_closed_loop_from_synthesized_views_into_the_evaluator():
    """Noise-free views of placed poses, one view of every joint redirected 0.4 .. 1.0 m off -> triangulate_rays_robust -> the
    placed poses, within 4 x what the float64 chain (the restatements of synth_cases and robust_tri_cases) reaches on the same
    rays: the factor covers another summation order over the views."""
    from openmpl_amd import PoseEvaluator, synthesize_views, triangulate_rays, triangulate_rays_robust
    B, V, J = 6, 4, 17
    poses3d, cams = sc.scene(B, V, J, seed=13, focal=600.0)
    kw = dict(seed=21, rotate=True, room=(-0.4, 0.4, -0.3, 0.3))
    placed = sc.synthesize(poses3d, cams, (1000.0, 1000.0), **kw)["placed"]
    r = synthesize_views(torch.from_numpy(poses3d).cuda(), torch.from_numpy(cams).cuda(), (1000.0, 1000.0), **kw)
    rays, centers = [_np(t).copy() for t in r.rays], [_np(t) for t in r.centers]
    rs = np.random.RandomState(4)
    which = rs.randint(0, V, size=(B, J))
    for v in range(V):
        cen = centers[v].astype(np.float64)
        los = placed - cen
        los /= np.linalg.norm(los, axis=-1, keepdims=True)
        off = rs.randn(B, J, 3)
        off -= np.sum(off * los, axis=-1, keepdims=True) * los
        off *= rs.uniform(0.4, 1.0, size=(B, J, 1)) / np.linalg.norm(off, axis=-1, keepdims=True)
        u = placed + off - cen
        u /= np.linalg.norm(u, axis=-1, keepdims=True)
        rays[v] = np.where((which == v)[..., None], (cen + u).astype(np.float32), rays[v])
    tau = 0.05
    x64, _, i64 = rc.robust(rays, centers, threshold=tau)
    e_ref = float(np.linalg.norm(x64 - placed, axis=-1).max())
    pts, res, inl = triangulate_rays_robust(_dev(rays), r.centers, threshold=tau)
    e_dev = float(np.linalg.norm(_np(pts).astype(np.float64) - placed, axis=-1).max())
    plain, _ = triangulate_rays(_dev(rays), r.centers)
    e_plain = float(np.linalg.norm(_np(plain).astype(np.float64) - placed, axis=-1).max())
    print("closed loop: max distance to the placed poses: float64 chain %.3e, device %.3e, least squares %.3e" % (e_ref, e_dev, e_plain))
    assert 0 < e_ref < 1e-4 and e_plain > 0.05
    assert e_dev <= 4 * e_ref
    want = np.stack([(which != v) for v in range(V)], axis=1).astype(np.float32)
    assert np.array_equal(_np(inl), want) and np.array_equal(i64, want)
    ev = PoseEvaluator(J)
    ev.update(pts, r.target)
    rep = ev.compute()
    print("closed loop: mpjpe %.3e" % rep["absolute"]["mpjpe"])
    assert rep["n_samples"] == B and np.isfinite(rep["absolute"]["mpjpe"])


def test_refusals_of_the_c_abi_launch_nothing():
    from openmpl_amd import cabi
    lib = cabi.load()
    B, V, J = 3, 3, 17
    case = gc.ring_case(B, V, J, seed=12)
    rays, centers, conf = _dev(case["rays"]), _dev(case["centers"]), _dev(_flat(case))
    tab = lambda lst: None if lst is None else (cabi._fp * len(lst))(*[t.data_ptr() for t in lst])      # noqa: E731
    out = torch.full((3, B * V * J), -12345.0, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call(conf=None, tau=0.08, cth=-1.0, m=2, views=V, pts=out[0].data_ptr(), res=out[1].data_ptr(), inl=out[2].data_ptr(), r=rays):
        return lib.mpl_triangulate_robust(tab(r), tab(centers), tab(conf), 1, B, views, J, tau, cth, m, pts, res, inl, st)

    def refused():
        return [call(pts=None), call(res=None), call(inl=None), call(cth=0.85), call(m=1), call(m=V + 1), call(r=None),
                call(conf=conf, cth=65.0), call(conf=conf, cth=float("inf"))]

    codes, n = _launches(refused)
    assert codes == [-1] * 7 + [-2] * 2 and n == 0 and bool((out == -12345.0).all())
    # a negative or NaN threshold is "off", not an error
    rcs, n = _launches(lambda: [call(conf=conf, tau=float("nan"), cth=float("nan")), call(tau=-1.0)])
    assert rcs == [0, 0] and n == 2
    torch.cuda.synchronize()
