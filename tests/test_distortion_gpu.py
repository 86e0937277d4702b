"""The lens on the device (csrc/views.hpp, distortion.hip, inputs.hip, synth.hip): every call that takes distortion= against the
float64 restatement of tests/distortion_cases.py and the reference-generated golden, and the closed loop that says what the
feature buys.  Tolerances: each output is one fp64 value rounded once to fp32 on both sides (tests/synth_cases.assert_matches)."""
import numpy as np
import pytest
import torch

from tests import distortion_cases as dc
from tests import geometry_cases as gc
from tests import synth_cases as sc

pytestmark = pytest.mark.gpu

G = dc.golden()
WH = (1000.0, 1000.0)
SHAPES = [(1, 1, 1), (3, 4, 17), (2, 32, 3), (5, 2, 64)]                   # one item; the usual rig; the view limit; 640 items: three
#                                                                            workgroups, the last one ragged
# (set, every n-th item of a view whose lens folds is made invalid); at (1,1,1) the one item is either valid or not
LENS = [("zeros", 0), ("h36m", 0), ("cmu", 5), ("strong", 5), ("per_view", 5)]
OWN = dict(rotate=True, room=(-0.4, 0.4, -0.3, 0.3), noise_level=6.0, penalize="exp_error", penalize_a=0.95, penalize_b=0.04,
           missing_level=0.2, target_scale=(2.0, 2.5, 1.25), target_offset=(0.1, -0.2, 1.0))


@pytest.fixture(autouse=True)
def _device_error_is_clear():
    yield
    from openmpl_amd import cabi
    torch.cuda.synchronize()
    assert not cabi.device_error()


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _np(lst):
    return np.stack([t.cpu().numpy() for t in lst])


def _case(B, V, J, name, every):
    if (B, V, J) == (1, 1, 1):
        every = 1 if every and name != "per_view" else 0         # view 0 of per_view has no fold
    return dc.case(B, V, J, name, invalid_every=every)


def _within_one_ulp(got, ref64, what):
    ref = ref64.astype(np.float32)
    assert got.dtype == np.float32 and got.shape == ref.shape
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    keep = ~np.isnan(ref)
    assert (np.abs(got[keep].astype(np.float64) - ref[keep]) <= np.spacing(np.abs(ref[keep]))).all(), what


# ------------------------------------------------------------------------------------------------------------------ 1. projection
def test_project_points_matches_golden_and_restatement():
    from openmpl_amd import project_points
    P, Cm = _dev(G["points"]), _dev(G["cams"])
    for name in ("zeros", "h36m", "strong"):
        px, depth = project_points(P, Cm, distortion=_dev(G[name + "_dist"]))
        got = dict(pixels_clean=px.cpu().numpy(), depth=depth.cpu().numpy())
        sc.assert_matches(got, dict(pixels_clean=G[name + "_pixels"]))
        ref_px, ref_depth = dc.project(G["points"], G["cams"], G[name + "_dist"])
        sc.assert_matches(got, dict(pixels_clean=ref_px, depth=ref_depth))
    # without the argument: the launch and the bits of before; zeros agree with them to rounding
    plain, _ = project_points(P, Cm)
    zeros, _ = project_points(P, Cm, distortion=_dev(G["zeros_dist"]))
    np.testing.assert_allclose(zeros.cpu().numpy(), plain.cpu().numpy(), rtol=2e-7, atol=2e-7)


@pytest.mark.parametrize("B,V,J", SHAPES)
@pytest.mark.parametrize("name", ["h36m", "strong", "per_view"])
def test_project_points_at_every_shape(B, V, J, name):
    from openmpl_amd import project_points
    c = dc.case(B, V, J, name)
    px, depth = project_points(_dev(c["points"]), _dev(c["cams"]), distortion=_dev(c["dist"]))
    ref_px, ref_depth = dc.project(c["points"], c["cams"], c["dist"])
    sc.assert_matches(dict(pixels_clean=px.cpu().numpy(), depth=depth.cpu().numpy()), dict(pixels_clean=ref_px, depth=ref_depth))
    # behind the camera: pixel (0,0), as without a lens
    pts = c["points"].copy()
    pts[0, 0] = c["cams"][0, 13:16] - 2.0 * c["cams"][0, 10:13]
    px, depth = project_points(_dev(pts), _dev(c["cams"]), distortion=_dev(c["dist"]))
    assert float(depth[0, 0, 0]) < 0 and not px[0, 0, 0].any()


# ------------------------------------------------------------------------------------------------- 2. the lens and its inverse
@pytest.mark.parametrize("B,V,J", SHAPES)
@pytest.mark.parametrize("name,every", LENS)
def test_undistort_and_distort_match_the_restatement(B, V, J, name, every):
    from openmpl_amd import distort_points, undistort_points
    c = _case(B, V, J, name, every)
    X, Cm, D = _dev(c["pixels"]), _dev(c["cams"]), _dev(c["dist"])
    out, valid = undistort_points(X, Cm, D)
    assert out.shape == (B, V, J, 2) and out.dtype == torch.float32 and valid.shape == (B, V, J) and valid.dtype == torch.bool
    got, ok = out.cpu().numpy(), valid.cpu().numpy()
    assert np.array_equal(ok, c["valid"])
    assert np.array_equal(np.isnan(got), np.broadcast_to(~c["valid"][..., None], got.shape))       # NaN exactly at the invalid items
    _within_one_ulp(got, c["restated"]["pixels"], "undistort_points")
    again, valid2 = undistort_points(X, Cm, D)
    assert np.array_equal(again.cpu().numpy(), got, equal_nan=True) and torch.equal(valid, valid2)
    if name == "zeros":
        assert torch.equal(out, X)
    # forward, on the pinhole pixels of the same points
    pin = dc.project(c["points"], c["cams"], dc.table("zeros", V))[0].astype(np.float32)
    fwd = distort_points(_dev(pin), Cm, D)
    _within_one_ulp(fwd.cpu().numpy(), dc.distort_pixels(pin, c["cams"], c["dist"]), "distort_points")
    assert torch.equal(fwd, distort_points(_dev(pin), Cm, D))
    if name == "zeros":
        assert torch.equal(fwd, _dev(pin))


# ------------------------------------------------------------------------------------------------------------- 3. there and back
@pytest.mark.parametrize("B,V,J", SHAPES)
@pytest.mark.parametrize("name", ["h36m", "cmu", "strong", "per_view"])
def test_distort_of_undistort_is_the_input(B, V, J, name):
    """The floor is the restatement's same chain on the same fp32 values, the undistorted pixel rounded to fp32 between the two
    calls; the device is allowed 4 x that, as the closed loops of test_synth_gpu.py are.  The correction is a few pixels and varies
    slowly, so the half ulp lost in between does not survive the second rounding: in numpy the floor is 0 in every case but
    (2,32,3) per_view (6.1e-5 px, one fp32 ulp at 1000 px), and where it is 0 the device has to return the input bits too.  It does
    unless its fp64 correction and numpy's fall on two sides of an fp32 rounding boundary, 1e-13 px apart in a spacing of 6e-5."""
    from openmpl_amd import distort_points, undistort_points
    c = dc.case(B, V, J, name)
    x = c["pixels"]
    mid = dc.undistort_pixels(x, c["cams"], c["dist"])["pixels"].astype(np.float32)
    floor = float(np.abs(dc.distort_pixels(mid, c["cams"], c["dist"]).astype(np.float32).astype(np.float64) - x).max())
    X, Cm, D = _dev(x), _dev(c["cams"]), _dev(c["dist"])
    u, valid = undistort_points(X, Cm, D)
    back = distort_points(u, Cm, D)
    err = float((back.double() - X.double()).abs().max())
    print("distort(undistort(x)) - x, %s at %s: restatement %.3e px, device %.3e px" % (name, (B, V, J), floor, err))
    assert bool(valid.all()) and floor < 1e-3
    assert err <= 4 * floor


# -------------------------------------------------------------------------------------------------------------- 4. prepare_inputs
@pytest.mark.parametrize("B,V,J", SHAPES)
@pytest.mark.parametrize("name,every", LENS)
def test_prepare_inputs_sends_the_ray_through_the_undistorted_pixel(B, V, J, name, every):
    from openmpl_amd import triangulate_rays
    from openmpl_amd.inputs import prepare_inputs
    c = _case(B, V, J, name, every)
    conf = (0.5 + 0.5 * sc.draw(5, "test.conf", 0, np.arange(B * V * J)).reshape(B, V, J)).astype(np.float32)
    X, Cf, Cm, D = _dev(c["pixels"]), _dev(conf), _dev(c["cams"]), _dev(c["dist"])
    bad_v = np.transpose(~c["valid"], (1, 0, 2))
    for norm_in, norm_cam in ((True, True), (True, False), (False, False)):
        p0, r0, c0 = prepare_inputs(X, Cf, Cm, WH, norm_in, norm_cam)
        p, r, ce = prepare_inputs(X, Cf, Cm, WH, norm_in, norm_cam, distortion=D)
        pz, rz, cz = prepare_inputs(X, Cf, Cm, WH, norm_in, norm_cam, distortion=_dev(dc.table("zeros", V)))
        for v in range(V):                                                    # zeros: bitwise the call without distortion
            assert torch.equal(pz[v], p0[v]) and torch.equal(rz[v], r0[v]) and torch.equal(cz[v], c0[v])
            assert torch.equal(ce[v], c0[v])
        P, R, P0, R0 = _np(p), _np(r), _np(p0), _np(r0)
        assert np.array_equal(P[..., :2], P0[..., :2])                        # poses: the observed pixel, under any set
        assert np.array_equal(P[..., 2][~bad_v], P0[..., 2][~bad_v])
        assert (P[..., 2][bad_v] == 0).all() and np.array_equal(R[bad_v], R0[bad_v])     # invalid: confidence 0, the pinhole ray
        ref = dc.prepare(c["pixels"], conf, c["cams"], c["dist"], WH, norm_in, norm_cam)
        sc.assert_matches(dict(poses=P, rays=R, centers=_np(ce)), ref)
    if V >= 2 and bad_v.any():
        # left out by the triangulation: what the ray of an invalid joint says does not matter
        p, r, ce = prepare_inputs(X, Cf, Cm, WH, False, False, distortion=D)
        pts, res = triangulate_rays(r, ce, p)
        moved = [torch.where(_dev(bad_v[v])[..., None], r[v] + 100.0, r[v]) for v in range(V)]
        pts2, res2 = triangulate_rays(moved, ce, p)
        assert np.array_equal(pts.cpu().numpy(), pts2.cpu().numpy(), equal_nan=True)
        assert np.array_equal(res.cpu().numpy(), res2.cpu().numpy(), equal_nan=True)


# ------------------------------------------------------------------------------------------------------------ 5. synthesize_views
def _synth(points, cams, dist, **kw):
    from openmpl_amd import synthesize_views
    if kw.get("conf") is not None:
        kw["conf"] = _dev(np.asarray(kw["conf"], np.float32))
    r = synthesize_views(_dev(points), _dev(cams), WH, return_pixels=True, distortion=_dev(dist), **kw)
    return dict(poses=_np(r.poses), rays=_np(r.rays), centers=_np(r.centers), target=r.target.cpu().numpy(), pixels=r.pixels.cpu().numpy(),
                pixels_clean=r.pixels_clean.cpu().numpy())


@pytest.mark.parametrize("B,V,J", SHAPES)
@pytest.mark.parametrize("name", ["h36m", "per_view"])
@pytest.mark.parametrize("clip", [True, False])
def test_synthesize_views_matches_the_restatement(B, V, J, name, clip):
    """Everything on.  The margin rule of test_own_streams_match_the_restatement: an item within 1e-6 px of a decision could decide
    differently; with these seeds there is none, and none comes near a fold either."""
    points, cams = sc.scene(B, V, J, seed=5, focal=dc.FOCAL)
    dist = dc.table(name, V)
    conf = None if clip else (0.5 + 0.5 * sc.draw(5, "test.conf", 0, np.arange(B * V * J)).reshape(B, V, J)).astype(np.float32)
    kw = dict(OWN, seed=17, first_index=1000003, clip=clip, conf=conf, normalize_cameras=clip)
    ref = dc.synthesize(points, cams, dist, WH, **kw)
    skip = ref["margin"] < 1e-6
    assert skip.sum() == 0
    assert ref["valid"].all() and ref["min_det"].min() >= dc.DET_MIN
    got = _synth(points, cams, dist, **kw)
    sc.assert_matches(got, ref, skip=skip)
    if B * V * J > 100:            # the case does what it is there for
        assert (ref["conf"] == 0).any() and (ref["conf"] > 0).any() and (ref["conf"] < 1).any()
        assert np.abs(ref["pixels_clean"] - sc.synthesize(points, cams, WH, **kw)["pixels_clean"]).max() > 0.5


def test_synthesize_views_batching_is_bitwise():
    points, cams = sc.scene(12, 4, 17, seed=2, focal=dc.FOCAL)
    dist = dc.table("per_view", 4)
    kw = dict(OWN, seed=3)
    whole = _synth(points, cams, dist, **kw)
    parts = [_synth(points[s:s + 4], cams, dist, first_index=s, **kw) for s in (0, 4, 8)]
    for k, axis in (("poses", 1), ("rays", 1), ("centers", 1), ("target", 0), ("pixels", 0), ("pixels_clean", 0)):
        assert np.array_equal(whole[k], np.concatenate([p[k] for p in parts], axis=axis), equal_nan=True), k
    # without the argument the launch is the one of before: the pinhole bits, which the lens moves
    from openmpl_amd import synthesize_views
    plain = synthesize_views(_dev(points), _dev(cams), WH, return_pixels=True, **kw)
    assert not np.array_equal(plain.pixels_clean.cpu().numpy(), whole["pixels_clean"])
    np.testing.assert_array_equal(plain.target.cpu().numpy(), whole["target"])


# ------------------------------------------------------------------------------------------------------------- 6. decode_heatmaps
@pytest.mark.parametrize("layout", ["list", "tensor"])
def test_decode_heatmaps_with_distortion_is_decode_then_prepare(layout):
    from openmpl_amd import decode_heatmaps
    from openmpl_amd.inputs import prepare_inputs
    B, V, J, H, W = 3, 4, 5, 24, 20
    _, cams = sc.scene(B, V, J, seed=7, focal=dc.FOCAL)
    hm = _dev(sc.draw(9, "test.hm", 0, np.arange(B * V * J * H * W)).reshape(B, V, J, H, W).astype(np.float32))
    center = _dev(np.tile(np.array([[480.0, 510.0]], np.float32), (B, V, 1)))
    scale = _dev(np.tile(np.array([[2.0, 2.0]], np.float32), (B, V, 1)))
    arg = [hm[:, v].contiguous() for v in range(V)] if layout == "list" else hm
    Cm, D = _dev(cams), _dev(dc.table("per_view", V))
    for norm in (True, False):
        d = decode_heatmaps(arg, center, scale, cams=Cm, image_size=WH, normalize_inputs=norm, normalize_cameras=norm, distortion=D,
                            subpixel="gaussian")
        plain = decode_heatmaps(arg, center, scale, subpixel="gaussian")
        p, r, c = prepare_inputs(plain.pixels, plain.conf, Cm, WH, norm, norm, distortion=D)
        assert torch.equal(d.pixels, plain.pixels) and torch.equal(d.conf, plain.conf)
        for v in range(V):
            assert torch.equal(d.poses[v], p[v]) and torch.equal(d.rays[v], r[v]) and torch.equal(d.centers[v], c[v])
        fused = decode_heatmaps(arg, center, scale, cams=Cm, image_size=WH, normalize_inputs=norm, normalize_cameras=norm, subpixel="gaussian")
        assert not torch.equal(fused.rays[1], d.rays[1]) and torch.equal(fused.poses[1], d.poses[1])     # the lens moves the rays only
    with pytest.raises(RuntimeError, match="distortion needs cams"):
        decode_heatmaps(arg, center, scale, distortion=D)


# ------------------------------------------------------------------------------------------------------------- 7. the closed loop
def test_closed_loop_the_lens_is_undone():
    """project_points(distortion=D) -> prepare_inputs(distortion=D) -> triangulate_rays recovers the points within 4 x the error of
    the float64 chain on the same fp32 rays; the same pixels through prepare_inputs without distortion -- what the chain did
    before -- land at least 100 x further away (in numpy: 1.6e-3 against below 1e-6 scene units)."""
    from openmpl_amd import project_points, triangulate_pixels, triangulate_rays
    from openmpl_amd.inputs import prepare_inputs
    B, V, J = 6, 4, 17
    points, cams = sc.scene(B, V, J, seed=3, focal=dc.FOCAL)
    dist = dc.table("h36m", V)
    P, Cm, D = _dev(points), _dev(cams), _dev(dist)
    # the float64 chain, rounded to fp32 where the device rounds
    px64 = dc.project(points, cams, dist)[0].astype(np.float32)
    ref = dc.prepare(px64, None, cams, dist, WH, False, False)
    x64, _ = gc.triangulate([r.astype(np.float32) for r in ref["rays"]], [c.astype(np.float32) for c in ref["centers"]])
    dist_to = lambda x: np.linalg.norm(np.asarray(x, dtype=np.float64) - points.astype(np.float64), axis=-1)
    e_ref = float(dist_to(x64).max())
    px, depth = project_points(P, Cm, distortion=D)
    p, r, c = prepare_inputs(px, None, Cm, WH, False, False, distortion=D)
    pts, res = triangulate_rays(r, c)
    e_dev = dist_to(pts.cpu().numpy())
    p0, r0, c0 = prepare_inputs(px, None, Cm, WH, False, False)
    pts0, _ = triangulate_rays(r0, c0)
    e_pin = dist_to(pts0.cpu().numpy())
    print("closed loop under the H36M-like lens, distance to the points (scene units): float64 chain max %.3e; device max %.3e mean %.3e; "
          "the same pixels taken for pinhole: max %.3e mean %.3e" % (e_ref, e_dev.max(), e_dev.mean(), e_pin.max(), e_pin.mean()))
    assert 0 < e_ref < 1e-5
    assert e_dev.max() <= 4 * e_ref
    assert e_pin.mean() >= 100 * e_dev.mean() and e_pin.max() >= 100 * e_dev.max()
    # the wrapper is the composition
    tp, tr, ti = triangulate_pixels(px, None, Cm, distortion=D)
    pts_c, res_c = triangulate_rays(r, c, p)
    assert torch.equal(tp, pts_c) and torch.equal(tr, res_c) and bool((ti == 1).all())
    conf = _dev((0.5 + 0.5 * sc.draw(5, "test.conf", 0, np.arange(B * V * J)).reshape(B, V, J)).astype(np.float32))
    tp, tr, ti = triangulate_pixels(px, conf, Cm, WH, distortion=D)
    p, r, c = prepare_inputs(px, conf, Cm, WH, False, False, distortion=D)
    pts_c, res_c = triangulate_rays(r, c, p)
    assert torch.equal(tp, pts_c) and torch.equal(tr, res_c)


# -------------------------------------------------------------------------------------------------------------------- the refusals
def test_errors_are_loud_and_launch_nothing():
    from openmpl_amd import cabi, decode_heatmaps, distort_points, project_points, synthesize_views, triangulate_pixels, undistort_points
    from openmpl_amd.inputs import prepare_inputs
    c = dc.case(2, 3, 17, "h36m")
    P, X, Cm, D = _dev(c["points"]), _dev(c["pixels"]), _dev(c["cams"]), _dev(c["dist"])
    cabi.profile_start()
    for bad in (D[:2], D[:, :4], D.float(), D.cpu(), D.reshape(-1)):
        with pytest.raises(RuntimeError, match="distortion must"):
            prepare_inputs(X, None, Cm, WH, distortion=bad)
        with pytest.raises(RuntimeError, match="distortion must"):
            undistort_points(X, Cm, bad)
        with pytest.raises(RuntimeError, match="distortion must"):
            project_points(P, Cm, distortion=bad)
        with pytest.raises(RuntimeError, match="distortion must"):
            synthesize_views(P, Cm, WH, distortion=bad)
        with pytest.raises(RuntimeError, match="distortion must"):
            triangulate_pixels(X, None, Cm, distortion=bad)
    with pytest.raises(RuntimeError, match="needs distortion"):
        distort_points(X, Cm, None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        undistort_points(X.cpu(), Cm, D)
    with pytest.raises(RuntimeError, match="pixels must be float32"):
        undistort_points(X.double(), Cm, D)
    with pytest.raises(RuntimeError, match="pixels must be float32"):
        distort_points(X[..., :1], Cm, D)
    with pytest.raises(RuntimeError, match="cams must be float64"):
        undistort_points(X, Cm[:2], D)
    hm = torch.zeros(2, 3, 17, 8, 8, device="cuda")
    with pytest.raises(RuntimeError, match="distortion"):
        decode_heatmaps(hm, cams=Cm, image_size=WH, distortion=D[:2])
    assert sum(n for _, n in cabi.profile_stop().values()) == 0        # nothing was launched
