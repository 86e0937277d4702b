"""Geometry entry points, CPU side: the public surface, the raising rules (checked before anything touches a device), the C ABI
bookkeeping, and the float64 restatement of tests/geometry_cases.py pinned on the golden that the reference's own calib.py
produced (tests/golden/make_golden_geometry.py); the GPU tests compare the kernels with both."""
import numpy as np
import pytest
import torch

from tests import geometry_cases as gc

B, V, J = 4, 3, 17


def lines(dtype=torch.float32):
    return [torch.zeros(B, J, 3, dtype=dtype) for _ in range(V)], [torch.zeros(B, 1, 3, dtype=dtype) for _ in range(V)]


def test_the_three_functions_are_exported():
    import openmpl_amd
    from openmpl_amd import geometry
    for name in ("triangulate_rays", "epipolar_errors", "consistency_weights"):
        assert getattr(openmpl_amd, name) is getattr(geometry, name) and callable(getattr(geometry, name))


def test_symbols_are_in_the_binding_and_the_abi_version_stays():
    from openmpl_amd import cabi
    assert "mpl_triangulate_rays" in cabi.EXPORTS and "mpl_epipolar_errors" in cabi.EXPORTS
    assert cabi.ABI_VERSION == 14
    lib = cabi.load()
    assert lib.mpl_hip_abi_version() == 14
    assert len(lib.mpl_triangulate_rays.argtypes) == 10 and len(lib.mpl_epipolar_errors.argtypes) == 12


def test_arguments_are_checked_and_named_before_any_device_is_touched():
    from openmpl_amd import consistency_weights, epipolar_errors, triangulate_rays
    rays, centers = lines()
    conf = [torch.ones(B, J) for _ in range(V)]
    weight = [torch.ones(B, J) for _ in range(V)]
    for fn in (triangulate_rays, epipolar_errors, lambda r, c, cf=None: consistency_weights(r, c, cf, weight)):
        with pytest.raises(RuntimeError, match=r"no CPU path: rays\[0\]"):
            fn(rays, centers)
        with pytest.raises(RuntimeError, match=r"float32 tensors required \(rays\[1\]"):
            fn([rays[0], rays[1].double(), rays[2]], centers)
        with pytest.raises(RuntimeError, match=r"float32 tensors required \(centers\[2\]"):
            fn(rays, centers[:2] + [centers[2].half()])
        with pytest.raises(RuntimeError, match=r"rays\[2\]: expected shape"):
            fn(rays[:2] + [rays[2][:, :16]], centers)
        with pytest.raises(RuntimeError, match=r"rays\[0\]: expected shape \(B,J,3\)"):
            fn([r[..., :2] for r in rays], centers)
        with pytest.raises(RuntimeError, match=r"centers\[1\]: expected shape"):
            fn(rays, [centers[0], centers[1].reshape(B, 3), centers[2]])
        with pytest.raises(RuntimeError, match="centers holds 2 tensors for 3 views"):
            fn(rays, centers[:2])
        with pytest.raises(RuntimeError, match="rays must be a non-empty list"):
            fn(rays[0], centers)
        with pytest.raises(RuntimeError, match="conf holds 2 tensors for 3 views"):
            fn(rays, centers, conf[:2])
        with pytest.raises(RuntimeError, match="conf holds 4 tensors for 3 views"):
            fn(rays, centers, conf + conf[:1])
        with pytest.raises(RuntimeError, match=r"conf\[1\]: expected shape"):
            fn(rays, centers, [conf[0], torch.ones(B, J, 3), conf[2]])                      # one form for all views
        with pytest.raises(RuntimeError, match=r"conf\[0\]: expected shape"):
            fn(rays, centers, [torch.ones(B, J, 2) for _ in range(V)])
        with pytest.raises(RuntimeError, match=r"float32 tensors required \(conf\[2\]"):
            fn(rays, centers, conf[:2] + [conf[2].double()])
    with pytest.raises(RuntimeError, match="weight holds 2 tensors for 3 views"):
        consistency_weights(rays, centers, conf, weight[:2])
    with pytest.raises(RuntimeError, match=r"weight\[0\]: expected shape"):
        consistency_weights(rays, centers, conf, [w[:, :5] for w in weight])
    with pytest.raises(RuntimeError, match="weight must be"):
        consistency_weights(rays, centers, conf, None)


@pytest.mark.parametrize("tag", ["v2", "v3", "v4"])
def test_restatement_matches_the_reference_golden(tag):
    """float64 on the float32 rays against the reference's float64 on the detections: what is left is the fp32 rounding of the
    rays, ~3e-6, far inside the 1e-4 parity rule the kernels are held to"""
    c = gc.golden_case(gc.golden(), tag)
    n = len(c["rays"])
    assert n == int(tag[1:]) and c["rays"][0].shape == (5, 17, 3) and c["rays"][0].dtype == np.float32
    conf = [c["conf"][v] for v in range(n)]
    cen, d = gc.lines(c["rays"], c["centers"])
    p = 0
    for i in range(n):
        for k in range(i + 1, n):
            mx, nw = gc.rel_errors(gc.pair_distance(cen[i], d[i], cen[k], d[k]), c["pairs"][p])
            assert mx <= 1e-5 and nw <= 1e-5, (tag, i, k, mx, nw)
            np.testing.assert_array_equal(gc.pair_distance(cen[k], d[k], cen[i], d[i]), gc.pair_distance(cen[i], d[i], cen[k], d[k]))
            p += 1
    err = gc.epipolar(c["rays"], c["centers"], conf)
    mx, nw = gc.rel_errors(err, c["err"])
    assert mx <= 1e-5 and nw <= 1e-5, (tag, mx, nw)
    poses = [np.stack([np.zeros_like(f), np.ones_like(f), f], axis=-1) for f in conf]         # channel 2 of a pose tensor
    np.testing.assert_array_equal(gc.epipolar(c["rays"], c["centers"], poses), err)
    assert np.abs(c["err"] / c["threshold"] - 1).min() > 1e-3                                # the weights are decided
    w = gc.thresholded(err, [c["weight"][v] for v in range(n)], c["threshold"])
    for v in range(n):
        np.testing.assert_array_equal(w[v], c["weights_out"][v])
    assert (c["weights_out"] == 0).any() and (c["weights_out"] != 0).any()


def test_restatement_triangulates_exact_lines_and_flags_degenerate_joints():
    case = gc.ring_case(3, 5, 17, seed=6, exact=True)
    x, r = gc.triangulate(case["rays"], case["centers"])
    assert np.abs(x - case["points"]).max() < 1e-5 and r.max() < 1e-5
    noisy = gc.ring_case(3, 3, 17, seed=7)
    conf = [noisy["conf"][v].copy() for v in range(3)]
    conf[1][1, 5] = conf[2][1, 5] = 0.0
    conf[1][0, 16] = np.nan
    x, r = gc.triangulate(noisy["rays"], noisy["centers"], conf)
    assert np.isnan(x[1, 5]).all() and np.isnan(r[1, 5]) and np.isnan(r).sum() == 1 and np.isnan(x).sum() == 3
    conf[1][0, 16] = 0.0
    x0, r0 = gc.triangulate(noisy["rays"], noisy["centers"], conf)
    np.testing.assert_array_equal(x, x0)
    np.testing.assert_array_equal(r, r0)
    # two views: det(A / sum w) = sin^2(angle) / 4
    c, d = gc.lines(noisy["rays"][:2], noisy["centers"][:2])
    A = sum(np.eye(3) - d[v][..., :, None] * d[v][..., None, :] for v in range(2)) / 2
    sin2 = np.sum(np.cross(d[0], d[1]) ** 2, axis=-1)
    np.testing.assert_allclose(np.linalg.det(A), sin2 / 4, rtol=1e-9)
