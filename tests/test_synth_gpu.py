"""synthesize_views / project_points (csrc/synth.hip) on the device: against the reference-generated golden with its explicit
streams, against the float64 restatement with the kernel's own streams, and closed loops through triangulate_rays, the model and
PoseEvaluator.  Tolerances: each output is one fp64 value rounded once to fp32 on both sides (tests/synth_cases.assert_matches)."""
import numpy as np
import pytest
import torch

from tests import geometry_cases as gc
from tests import synth_cases as sc

pytestmark = pytest.mark.gpu

G = sc.golden()
COMBOS = [(t, p, c) for t in sc.TAGS for p in sc.PENALTIES for c in (True, False)]
WH = (1000.0, 1000.0)
# everything switched on; the seeds are picked so that the restatement has no item within 1e-6 px of a decision
OWN = dict(rotate=True, room=(-0.4, 0.4, -0.3, 0.3), noise_level=6.0, penalize="exp_error", penalize_a=0.95, penalize_b=0.04,
           missing_level=0.2, target_scale=(2.0, 2.5, 1.25), target_offset=(0.1, -0.2, 1.0))
OWN_SHAPES = [(1, 1, 1), (7, 4, 17), (2, 32, 3), (3, 2, 64)]


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _run(poses3d, cams, wh, **kw):
    """synthesize_views on numpy inputs -> dict of numpy outputs in the layout of sc.synthesize"""
    from openmpl_amd import synthesize_views
    for k in ("conf", "rotation_deg", "translation", "noise", "missing_u"):
        if kw.get(k) is not None:
            kw[k] = _dev(np.asarray(kw[k], np.float32))
    r = synthesize_views(_dev(poses3d), _dev(cams), wh, return_pixels=True, **kw)
    return dict(poses=np.stack([t.cpu().numpy() for t in r.poses]), rays=np.stack([t.cpu().numpy() for t in r.rays]),
                centers=np.stack([t.cpu().numpy() for t in r.centers]), target=r.target.cpu().numpy(), pixels=r.pixels.cpu().numpy(),
                pixels_clean=r.pixels_clean.cpu().numpy())


def _no_device_error():
    from openmpl_amd import cabi
    torch.cuda.synchronize()
    assert not cabi.device_error()


@pytest.mark.parametrize("tag,penalize,clip", COMBOS)
def test_kernel_matches_reference_golden(tag, penalize, clip):
    poses3d, cams, wh, kw = sc.golden_case(G, tag, penalize)
    got = _run(poses3d, cams, wh, clip=clip, **kw)
    sc.assert_matches(got, {k: v.astype(np.float64) for k, v in sc.golden_outputs(G, tag, penalize, clip).items()})
    _no_device_error()


@pytest.mark.parametrize("B,V,J", OWN_SHAPES)
@pytest.mark.parametrize("clip", [True, False])
def test_own_streams_match_the_restatement(B, V, J, clip):
    """Box-Muller uses the device's log / cos here and libm in the restatement: an item within 1e-6 px of a decision could decide
    differently and is left out -- at most 1 % of a case, and with these seeds none."""
    poses3d, cams = sc.scene(B, V, J, seed=5, focal=2400.0)
    conf = None if clip else (0.5 + 0.5 * sc.draw(5, "test.conf", 0, np.arange(B * V * J)).reshape(B, V, J)).astype(np.float32)
    kw = dict(OWN, seed=17, first_index=1000003, clip=clip, conf=conf, normalize_cameras=clip)
    ref = sc.synthesize(poses3d, cams, WH, **kw)
    skip = ref["margin"] < 1e-6
    assert skip.sum() <= 0.01 * skip.size and skip.sum() == 0
    got = _run(poses3d, cams, WH, **kw)
    sc.assert_matches(got, ref, skip=skip)
    if B * V * J > 100:            # the case does what it is there for
        assert (ref["conf"] == 0).any() and (ref["conf"] > 0).any() and (ref["conf"] < 1).any()
    _no_device_error()


def test_batching_and_seeds_bitwise():
    poses3d, cams = sc.scene(12, 4, 17, seed=2, focal=2400.0)
    kw = dict(OWN, seed=3)
    whole = _run(poses3d, cams, WH, **kw)
    again = _run(poses3d, cams, WH, **kw)
    parts = [_run(poses3d[s:s + 4], cams, WH, first_index=s, **kw) for s in (0, 4, 8)]
    for k, axis in (("poses", 1), ("rays", 1), ("centers", 1), ("target", 0), ("pixels", 0), ("pixels_clean", 0)):
        assert np.array_equal(whole[k], again[k], equal_nan=True), k
        assert np.array_equal(whole[k], np.concatenate([p[k] for p in parts], axis=axis), equal_nan=True), k
    other = _run(poses3d, cams, WH, **dict(kw, seed=4))
    assert not np.array_equal(whole["pixels"], other["pixels"])
    _no_device_error()


def test_switches_off_is_project_points_then_prepare_inputs():
    from openmpl_amd import project_points, synthesize_views
    from openmpl_amd.inputs import prepare_inputs
    poses3d, cams = sc.scene(5, 3, 17, seed=9, focal=600.0)           # a short focal length: every joint is inside the image
    P, Cm = _dev(poses3d), _dev(cams)
    r = synthesize_views(P, Cm, WH, clip=False, return_pixels=True)
    px, depth = project_points(P, Cm)
    assert torch.equal(px, r.pixels_clean) and torch.equal(px, r.pixels) and float(depth.min()) > 1.0
    assert float(px.min()) > 0 and float(px.max()) < 999
    p, ry, c = prepare_inputs(px, None, Cm, WH)
    for v in range(3):
        np.testing.assert_allclose(r.poses[v].cpu().numpy(), p[v].cpu().numpy(), rtol=2e-7, atol=2e-7)
        np.testing.assert_allclose(r.rays[v].cpu().numpy(), ry[v].cpu().numpy(), rtol=3e-7, atol=5e-7)
        assert torch.equal(r.centers[v], c[v])
        assert bool((r.poses[v][..., 2] == 1).all())
    assert torch.equal(r.target, P) and r.target.data_ptr() != P.data_ptr()
    # without noise there is nothing to penalise
    q = synthesize_views(P, Cm, WH, clip=False, noise_level=0.0, penalize="exp_sqrt", penalize_a=0.5)
    for v in range(3):
        assert torch.equal(q.poses[v], r.poses[v]) and torch.equal(q.rays[v], r.rays[v])
    assert q.pixels is None and q.pixels_clean is None
    _no_device_error()


def test_closed_loop_triangulation_returns_the_placed_poses():
    """Noise-free views -> triangulate_rays -> the placed poses.  The bound is 4 x the error of the same chain in float64 (the
    restatements of synth_cases and geometry_cases) on fp32-rounded rays and centres: the factor covers another summation order
    over the views."""
    from openmpl_amd import synthesize_views, triangulate_rays
    B, V, J = 6, 4, 17
    poses3d, cams = sc.scene(B, V, J, seed=13, focal=600.0)
    kw = dict(seed=21, rotate=True, room=(-0.4, 0.4, -0.3, 0.3))
    ref = sc.synthesize(poses3d, cams, WH, **kw)
    assert (ref["conf"] == 1).all()
    x64, _ = gc.triangulate([r.astype(np.float32) for r in ref["rays"]], [c.astype(np.float32) for c in ref["centers"]])
    e_ref = float(np.linalg.norm(x64 - ref["placed"], axis=-1).max())
    r = synthesize_views(_dev(poses3d), _dev(cams), WH, **kw)
    pts, res = triangulate_rays(r.rays, r.centers)
    e_dev = float(np.linalg.norm(pts.cpu().numpy().astype(np.float64) - ref["placed"], axis=-1).max())
    print("closed loop: max distance to the placed poses: float64 chain %.3e, device %.3e (world units)" % (e_ref, e_dev))
    assert 0 < e_ref < 1e-4
    assert e_dev <= 4 * e_ref
    np.testing.assert_allclose(r.target.cpu().numpy(), ref["placed"].astype(np.float32), rtol=2e-7, atol=2e-7)
    _no_device_error()


def test_closed_loop_model_and_evaluator():
    from openmpl_amd import PoseEvaluator, detrng, synthesize_views
    from openmpl_amd.multiview_mpl import MultiView_MPL
    from oracle import mpl_oracle
    flags = dict(num_joints=17, embed_dim_ratio=32, num_heads=8, depth=2, num_views=3, pose_3d_emb_learnable=True,
                 confidence_input_as_third=True, input_rays_as_token=True, multiple_spatial_blocks=True,
                 add_3D_pos_encoding_to_rays=True)
    m = MultiView_MPL(**flags)
    detrng.fill_module_(m, seed=5)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m = m.cuda().eval()
    poses3d, cams = sc.scene(5, 3, 17, seed=5, focal=2400.0)
    kw = dict(OWN, seed=17)
    ref = sc.synthesize(poses3d, cams, WH, **kw)
    assert (ref["margin"] < 1e-6).sum() == 0 and (ref["conf"] == 0).any()
    r = synthesize_views(_dev(poses3d), _dev(cams), WH, **kw)
    with torch.no_grad():
        out = m(r.poses, rays=r.rays, centers=r.centers)
    f32 = lambda a: [torch.from_numpy(x.astype(np.float32)) for x in a]
    want = mpl_oracle.forward(sd, flags, f32(ref["poses"]), f32(ref["rays"]), f32(ref["centers"]))
    mx, nw = mpl_oracle.rel_errors(out.cpu(), want)
    print("model on synthesized views against the oracle on the restatement: max %.2e norm %.2e" % (mx, nw))
    assert mx < 1e-4 and nw < 1e-4
    ev = PoseEvaluator(17)
    ev.update(out, r.target, scale=kw["target_scale"], offset=kw["target_offset"])
    rep = ev.compute()
    assert rep["n_samples"] == 5 and np.isfinite(rep["loss"]) and np.isfinite(rep["absolute"]["mpjpe"])
    assert np.isfinite(rep["absolute"]["pjpe"]).all() and np.isfinite(rep["relative"]["pjpe"]).all()
    _no_device_error()


def test_project_points_matches_golden_and_restatement():
    from openmpl_amd import project_points
    for tag in sc.TAGS:
        points, cams = G[tag + "_points"], G[tag + "_cams"]            # the placed poses of the case, float32
        px, depth = project_points(_dev(points), _dev(cams))
        assert px.shape == (5, 3, 17, 2) and depth.shape == (5, 3, 17)
        got = dict(pixels_clean=px.cpu().numpy(), depth=depth.cpu().numpy())
        sc.assert_matches(got, dict(pixels_clean=G[tag + "_points_pixels"], depth=G[tag + "_points_depth"]))
        sc.assert_matches(got, sc.synthesize(points, cams, (1.0, 1.0)))
    # behind the camera: pixel (0,0), the depth says why
    poses3d, cams = sc.scene(2, 2, 5, seed=1)
    poses3d[0, 0] = cams[0, 13:16] - 2.0 * cams[0, 10:13]
    px, depth = project_points(_dev(poses3d), _dev(cams))
    assert float(depth[0, 0, 0]) < 0 and not px[0, 0, 0].any() and bool((depth[0, 0, 1:] > 0).all())
    _no_device_error()


def test_errors_are_loud_and_launch_nothing():
    from openmpl_amd import cabi, project_points, synthesize_views
    poses3d, cams = sc.scene(2, 3, 17, seed=1)
    P, Cm = _dev(poses3d), _dev(cams)
    cabi.profile_start()
    with pytest.raises(RuntimeError, match="no CPU path"):
        synthesize_views(torch.from_numpy(poses3d), Cm, WH)
    with pytest.raises(RuntimeError, match="no CPU path"):
        project_points(torch.from_numpy(poses3d), Cm)
    for bad in (Cm[:, :15], Cm.float(), Cm.cpu(), Cm.reshape(-1)):
        with pytest.raises(RuntimeError, match="cams must be float64"):
            synthesize_views(P, bad, WH)
    with pytest.raises(RuntimeError, match="at most 32 views"):
        synthesize_views(P, _dev(sc.scene(2, 33, 17, seed=1)[1]), WH)
    with pytest.raises(RuntimeError, match="noise must be float32"):
        synthesize_views(P, Cm, WH, noise_level=1.0, noise=torch.zeros(2, 3, 17, 3, device="cuda"))
    with pytest.raises(RuntimeError, match="penalize must be one of"):
        synthesize_views(P, Cm, WH, penalize="sqrt")
    with pytest.raises(RuntimeError, match="target_scale"):
        synthesize_views(P, Cm, WH, target_scale=(1.0, 0.0, 1.0))
    with pytest.raises(RuntimeError, match="room takes"):
        synthesize_views(P, Cm, WH, room=(0.5, -0.5, 0.0, 1.0))
    with pytest.raises(RuntimeError, match="poses3d must be float32"):
        synthesize_views(P.double(), Cm, WH)
    with pytest.raises(RuntimeError, match="image_size"):
        synthesize_views(P, Cm, (0.0, 1000.0))
    assert sum(n for _, n in cabi.profile_stop().values()) == 0        # nothing was launched
    _no_device_error()
