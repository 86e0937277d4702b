"""triangulate_rays_robust, CPU side: the float64 restatement of tests/robust_tri_cases.py pinned on the selections the reference's
own triangulate_poses produced (tests/golden/make_golden_triangulate_select.py) and on constructed cases, the public surface, and
the raising rules (checked before anything touches a device).  The GPU tests compare the kernel with the restatement."""
import re

import numpy as np
import pytest
import torch

from tests import geometry_cases as gc
from tests import robust_tri_cases as rc

B, V, J = 4, 3, 17


def lines(dtype=torch.float32):
    return [torch.zeros(B, J, 3, dtype=dtype) for _ in range(V)], [torch.zeros(B, 1, 3, dtype=dtype) for _ in range(V)]


def test_the_function_is_exported_and_bound():
    import openmpl_amd
    from openmpl_amd import cabi, geometry
    assert openmpl_amd.triangulate_rays_robust is geometry.triangulate_rays_robust
    assert "mpl_triangulate_robust" in cabi.EXPORTS and cabi.ABI_VERSION == 14
    lib = cabi.load()
    assert len(lib.mpl_triangulate_robust.argtypes) == 14
    header = open(cabi._build.HEADERS[-1]).read()
    assert re.search(r"int mpl_triangulate_robust\(", header)


@pytest.mark.parametrize("tag", ["v2", "v4", "v8"])
def test_restatement_selects_what_the_reference_selects(tag):
    g = rc.golden_select()
    confs, starts, sel = g[tag + "_confs"], g[tag + "_starts"], g[tag + "_sel"]
    n, joints = confs.shape
    assert n == int(tag[1:]) and confs.dtype == np.float32 and sel.shape == (len(starts), n, joints)
    with np.errstate(invalid="ignore"):
        passing = (confs > 0.85).sum(axis=0)
    assert (passing == 0).any() and (passing == 1).any() and (passing >= 2).any()
    assert (confs == confs[:1]).all(axis=0).any()                                  # a joint with all confidences equal
    zero_selected = False
    for s, start in enumerate(starts):
        for j in range(joints):
            got = rc.select(confs[:, j].astype(np.float64), start)
            assert np.array_equal(got, sel[s, :, j]), (tag, start, j, confs[:, j])
            zero_selected |= bool((got & (confs[:, j] == 0)).any())
    assert zero_selected                    # the descent past 0: the reference takes zero-confidence views, the restatement's
    # candidates do not
    case = gc.ring_case(1, n, joints, seed=2)
    conf = [confs[v][None] for v in range(n)]
    x, res, inl = rc.robust(case["rays"], case["centers"], conf, conf_threshold=float(starts[0]))
    want = sel[0] & rc.participation(confs.astype(np.float64))
    want &= want.sum(axis=0) >= 2
    assert np.array_equal(inl[0], want.astype(np.float32))
    assert np.array_equal(np.isnan(res[0]), want.sum(axis=0) == 0) and np.isnan(res).any() and np.isfinite(res).any()


def test_restatement_with_both_stages_off_is_the_plain_triangulation():
    case = gc.ring_case(3, 4, 17, seed=5)
    conf = [case["conf"][v].copy() for v in range(4)]
    conf[1][1, 5] = conf[2][1, 5] = conf[3][1, 5] = 0.0
    conf[0][2, 2] = np.nan
    for cf in (None, conf):
        x0, r0 = gc.triangulate(case["rays"], case["centers"], cf)
        x, r, inl = rc.robust(case["rays"], case["centers"], cf)
        np.testing.assert_array_equal(x, x0)
        np.testing.assert_array_equal(r, r0)
        part = np.transpose(rc.participation(gc.confidence(cf, 4, 3, 17)), (1, 0, 2))
        part = part & ~np.isnan(r0)[:, None]
        np.testing.assert_array_equal(inl, part.astype(np.float32))
    assert np.isnan(r[1, 5]) and inl[1, :, 5].sum() == 0 and inl[2, 0, 2] == 0 and inl[2, :, 2].sum() == 3


@pytest.mark.parametrize("shape,n_out", [((3, 4, 17), 1), ((2, 8, 5), 2), ((1, 31, 3), 7)])
def test_restatement_recovers_exact_points_and_marks_the_redirected_views(shape, n_out):
    case = rc.outlier_case(*shape, n_out=n_out, seed=1, exact=True, configs=())
    x, res, inl = rc.robust(case["rays"], case["centers"], threshold=case["tau"])
    assert np.abs(x - case["points"]).max() < 1e-5 and res.max() < 1e-5
    np.testing.assert_array_equal(inl, (~case["out"]).astype(np.float32))
    x_ls, _ = gc.triangulate(case["rays"], case["centers"])
    assert np.abs(x_ls - case["points"]).max() > 0.02                               # what the outliers do to least squares
    # min_inliers above what any hypothesis reaches: a statement about the joint
    x, res, inl = rc.robust(case["rays"], case["centers"], threshold=case["tau"], min_inliers=shape[1] - n_out + 1)
    assert np.isnan(x).all() and np.isnan(res).all() and not inl.any()


def test_noisy_cases_keep_their_margins_and_beat_least_squares():
    for shape, n_out in (((3, 4, 17), 1), ((2, 8, 5), 2), ((2, 3, 17), 0)):
        case = rc.outlier_case(*shape, n_out=n_out, seed=1)
        assert all(d > rc.MARGIN and c > rc.MARGIN for _, _, d, c in case["margins"])
        x, _, inl = rc.robust(case["rays"], case["centers"], threshold=case["tau"])
        x_ls, _ = gc.triangulate(case["rays"], case["centers"])
        ok = ~np.isnan(x).any(axis=-1)
        e, e_ls = np.linalg.norm(x - case["points"], axis=-1)[ok].mean(), np.linalg.norm(x_ls - case["points"], axis=-1).mean()
        print("%s: mean error %.4f m robust, %.4f m least squares, %d of %d joints" % (shape, e, e_ls, ok.sum(), ok.size))
        assert ok.mean() > 0.9 and e < 0.06 and (n_out == 0 or e < 0.5 * e_ls)
        assert not (inl.astype(bool) & case["out"]).any() or n_out == 0 or (inl.astype(bool) & case["out"]).mean() < 0.02


def test_arguments_are_checked_and_named_before_any_device_is_touched():
    from openmpl_amd import triangulate_rays_robust as fn
    rays, centers = lines()
    conf = [torch.ones(B, J) for _ in range(V)]
    # shapes, then dtypes, then devices: those of triangulate_rays
    with pytest.raises(RuntimeError, match="rays must be a non-empty list"):
        fn(rays[0], centers)
    with pytest.raises(RuntimeError, match=r"rays\[0\]: expected shape \(B,J,3\)"):
        fn([r[..., :2] for r in rays], centers)
    with pytest.raises(RuntimeError, match=r"rays\[2\]: expected shape"):
        fn(rays[:2] + [rays[2][:, :16]], centers, threshold=0.1)
    with pytest.raises(RuntimeError, match="centers holds 2 tensors for 3 views"):
        fn(rays, centers[:2])
    with pytest.raises(RuntimeError, match=r"centers\[1\]: expected shape"):
        fn(rays, [centers[0], centers[1].reshape(B, 3), centers[2]])
    with pytest.raises(RuntimeError, match="conf holds 2 tensors for 3 views"):
        fn(rays, centers, conf[:2], conf_threshold=0.85)
    with pytest.raises(RuntimeError, match=r"conf\[1\]: expected shape"):
        fn(rays, centers, [conf[0], torch.ones(B, J, 3), conf[2]])
    with pytest.raises(RuntimeError, match=r"rays\[2\]: expected shape"):                  # a shape before a dtype
        fn([rays[0].double(), rays[1], rays[2][:1]], centers)
    with pytest.raises(RuntimeError, match=r"float32 tensors required \(rays\[1\]"):
        fn([rays[0], rays[1].double(), rays[2]], centers)
    with pytest.raises(RuntimeError, match=r"float32 tensors required \(centers\[2\]"):
        fn(rays, centers[:2] + [centers[2].half()])
    with pytest.raises(RuntimeError, match=r"float32 tensors required \(conf\[2\]"):
        fn(rays, centers, conf[:2] + [conf[2].double()])
    with pytest.raises(RuntimeError, match=r"no CPU path: rays\[0\]"):                     # a dtype before a device
        fn(rays, centers, conf, threshold=0.08, conf_threshold=0.85, min_inliers=3)
    # the options of the robust call
    with pytest.raises(RuntimeError, match="conf_threshold needs conf"):
        fn(rays, centers, conf_threshold=0.85)
    for bad in (0.0, -0.08, float("nan")):
        with pytest.raises(RuntimeError, match="threshold must be a positive distance"):
            fn(rays, centers, threshold=bad)
    for bad in (float("nan"), 65.0, float("inf")):
        with pytest.raises(RuntimeError, match="conf_threshold must be a number of at most 64"):
            fn(rays, centers, conf, conf_threshold=bad)
    for bad in (1, 0, V + 1, 2.5):
        with pytest.raises(RuntimeError, match=r"min_inliers must be an integer in \[2, 3 views\]"):
            fn(rays, centers, min_inliers=bad)
    with pytest.raises(RuntimeError, match=r"min_inliers must be an integer in \[2, 1 views\]"):
        fn(rays[:1], centers[:1])
