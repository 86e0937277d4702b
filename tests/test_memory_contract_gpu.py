"""The memory contract of every entry point: where a call writes, and what it reads that it was never given.

Every case runs through tests/guarded.py `run_contract`: the call is made with every output, workspace and input between guards
the harness owns, under the NaN pattern, under zero bytes and with 1e30 instead of NaN around the inputs.  Asserted per case:
every guard intact; every element of every returned tensor written (EXEMPT is the closed list of outputs the documentation
leaves alone); the same bits under both prefills and both surroundings, and the bits of the plain call -- which the entry point's
own test file ties to its float64 restatement --; the inputs keep their bits; the tensors handed in and out are the ones the
launches saw; the device-error word is clear.  tests/test_guarded_cpu.py shows without a GPU that this procedure rejects a write
one element before or behind an output, at the far end of a guard, an element left unwritten, an int32 left unwritten, a
workspace read before it is written, a read behind an input and an input that was copied.

The cases are those of each entry point's own case module and shape list, which hold the tile edges, plus the corners they lack:
V = 32 with J = 64, and work-item counts one below, at and one above the workgroup of the kernel (read from its launch line):

  entry point                              workgroup               the case that visits its tail thread
  prepare_inputs, undistort / distort,     256 over B V J          n255 / n257 (5,3,17) / (257,1,1): removing `idx >= total`
  synthesize_views, project_points                                 writes behind the last view's tensors
  triangulate_rays_robust, refine_points,  64 over B J             n63 / n65 (9,V,7) / (5,V,13)
  reprojection_errors, triangulate_pixels
  refine_cameras (bundle_adjust)           512 striding over B J   n511 / n513 (73,V,7) / (27,V,19)
  refine_poses                             one wave per pose       (2,4,64): every lane a joint; (1,1,1): 63 idle lanes
  locate_cameras, relative_pose            64 hypotheses, tiles    small_h63 / small_h65 (a lane beyond H), n63 / n65 (a slot beyond N)
                                           of 64 slots
  refine_relative_pose                     256 striding over B J   n255 / n257 (15,2,17) / (257,2,1)
  decode_heatmaps, render_heatmaps         4 maps per workgroup    (1,3,17,64,64): 51 maps, (1,2,3,5,7): 6 maps; a map beyond N
  rpsm                                     256 over the bins       n5 (125 bins), n11 (1331 bins): cubes, so never 255 or 257
  pose_metrics                             one workgroup           J 16 / 33: joints below the 17 / 64 lanes of a slice

Removing the bounds check of the tail thread of any of these kernels turns the named case red: its write lands in a guard.
On passing, every test prints how many allocations and bytes it guarded.
"""
import functools

import numpy as np
import pytest
import torch

from tests import guarded as G

pytestmark = pytest.mark.gpu

# The closed list of outputs that need not be written everywhere: (entry point, field) -> the docstring sentence that grants it.
# It is empty: every entry point documents a value for every element of everything it returns.
EXEMPT = {}

_STATS = {}


def _report(entry, stats, capsys):
    n = sum(s[0] for s in stats)
    b = sum(s[1] for s in stats)
    _STATS[entry] = (len(stats), n, b)
    with capsys.disabled():
        print("\n%s: %d cases, %d guarded allocations, %d bytes (each run three times between its guards)" % (entry, len(stats), n, b))
    assert n > 0 and b > 0, "%s reached no guarded allocation" % entry


def _lib():
    from openmpl_amd import cabi
    return cabi.load()


# ---------------------------------------------------------------------------------------------------------------- the lines of sight
ROBUST_EDGES = [((9, 2, 7), 0), ((4, 3, 16), 1), ((5, 2, 13), 0), ((1, 32, 64), 4)]       # 63, 64, 65 items; the envelope corner


def test_triangulate_rays_robust(capsys):
    from openmpl_amd import triangulate_rays_robust
    from tests import robust_tri_cases as rt
    from tests.test_triangulate_robust_gpu import SHAPES
    stats = []
    for (B, V, J), n_out in list(SHAPES) + ROBUST_EDGES:
        c = rt.outlier_case(B, V, J, n_out=n_out, seed=3, n_zero=max(1, B * V * J // 25), configs=())
        flat = [c["conf"][v] for v in range(V)]
        poses = [np.concatenate([np.zeros(f.shape + (2,), np.float32), f[..., None]], axis=-1) for f in flat]
        for conf, kw in ((None, dict(threshold=c["tau"])), (flat, dict(threshold=c["tau"], conf_threshold=0.5)),
                         (poses, dict(threshold=None, conf_threshold=0.5)), (flat, dict())):
            call = lambda rays, centers, conf, kw=kw: triangulate_rays_robust(rays, centers, conf, **kw)
            _, n, b = G.run_contract(call, dict(rays=list(c["rays"]), centers=list(c["centers"]), conf=conf), min_outputs=3)
            stats.append((n, b))
    _report("triangulate_rays_robust", stats, capsys)


# ------------------------------------------------------------------------------------------------- points against pixels, 64 over B J
POINT_EDGES = [(9, 2, 7), (4, 3, 16), (5, 2, 13), (1, 32, 64)]


def _point_shapes():
    from tests.test_refine_gpu import SHAPES
    return list(SHAPES) + POINT_EDGES


@functools.lru_cache(maxsize=None)
def _point_case(B, V, J, conf):
    from tests import refine_cases as rc
    return rc.case(B, V, J, "h36m", conf=conf)


def test_refine_points_and_reprojection_errors(capsys):
    from openmpl_amd import refine_points, reprojection_errors
    stats, errs = [], []
    for B, V, J in _point_shapes():
        for conf, lens, kw in (("none", True, dict()), ("mixed", True, dict(huber=2.5)), ("uniform", False, dict(max_iterations=3))):
            c = _point_case(B, V, J, conf)
            args = dict(points=c["points0"], pixels=c["pixels"], conf=c["conf"], cams=c["cams"], distortion=c["dist"] if lens else None)
            r, n, b = G.run_contract(lambda **a: refine_points(**a, **kw), args, min_outputs=5)
            assert r.iterations.dtype == torch.int32 and r.status.dtype == torch.uint8 and int(r.status.max()) <= 3
            stats.append((n, b))
            _, n, b = G.run_contract(lambda **a: reprojection_errors(**a), args, min_outputs=2)
            errs.append((n, b))
    _report("refine_points", stats, capsys)
    _report("reprojection_errors", errs, capsys)


def test_triangulate_pixels(capsys):
    from openmpl_amd import triangulate_pixels
    stats = []
    for B, V, J in _point_shapes():
        if V < 2:
            continue
        for conf, lens, kw in (("none", True, dict()), ("uniform", True, dict(threshold=0.3, refine=True, huber=2.5)),
                               ("mixed", False, dict(conf_threshold=0.5, refine=True))):
            c = _point_case(B, V, J, conf)
            args = dict(pixels=c["pixels"], conf=c["conf"], cams=c["cams"], distortion=c["dist"] if lens else None)
            _, n, b = G.run_contract(lambda **a: triangulate_pixels(image_size=(1000.0, 1000.0), **a, **kw), args, min_outputs=3)
            stats.append((n, b))
    _report("triangulate_pixels", stats, capsys)


# ------------------------------------------------------------------------------------------------- cameras: 512 threads stride over B J
CAMERA_EDGES = [(73, 2, 7), (32, 2, 16), (27, 2, 19), (1, 32, 64)]          # N = 511, 512, 513; the envelope corner


@functools.lru_cache(maxsize=None)
def _camera_case(B, V, J, conf="none"):
    from tests import refine_cameras_cases as cc
    return cc.case(B, V, J, "h36m", conf=conf)


def test_refine_cameras_and_bundle_adjust(capsys):
    from openmpl_amd import bundle_adjust, refine_cameras
    from tests.test_refine_cameras_gpu import SHAPES
    stats, ba = [], []
    for B, V, J in list(SHAPES) + CAMERA_EDGES:
        for conf, lens, kw in (("none", True, dict()), ("mixed", False, dict(huber=2.5, fixed=(0,), max_iterations=5))):
            c = _camera_case(B, V, J, conf)
            args = dict(points=c["points"], pixels=c["pixels"], conf=c["conf"], cams=c["cams0"], distortion=c["dist"] if lens else None)
            r, n, b = G.run_contract(lambda **a: refine_cameras(**a, **kw), args, min_outputs=7)
            assert r.used.dtype == torch.int32 and int(r.status.max()) <= 3
            stats.append((n, b))
        if (B, V, J) in ((1, 4, 17), (70, 3, 17), (27, 2, 19)):
            _, n, b = G.run_contract(lambda **a: bundle_adjust(**a, rounds=2, fixed=(0,), max_iterations=4), args, min_outputs=2 + 7 + 5)
            ba.append((n, b))
    _report("refine_cameras", stats, capsys)
    _report("bundle_adjust", ba, capsys)


def test_refine_poses(capsys):
    from openmpl_amd import refine_poses
    from tests import refine_poses_cases as pc
    from tests.test_refine_poses_gpu import SHAPES
    stats = []
    for B, V, J, kind in list(SHAPES) + [(2, 32, 64, "random")]:
        for conf, limb, lens, kw in (("none", "pose", True, dict()), ("mixed", "shared", False, dict(huber=2.5, max_iterations=6))):
            c = pc.case(B, V, J, kind, "h36m", conf=conf, limb=limb)
            args = dict(points=c["points0"], pixels=c["pixels"], conf=c["conf"], cams=c["cams"], limb_length=c["limb"],
                        distortion=c["dist"] if lens else None)
            r, n, b = G.run_contract(lambda **a: refine_poses(parents=c["parents"], **a, **kw), args, min_outputs=7)
            assert r.cost.dtype == torch.float64 and r.iterations.dtype == torch.int32 and int(r.status.max()) <= 3
            stats.append((n, b))
    _report("refine_poses", stats, capsys)


# -------------------------------------------------------------------------------------- hypothesise and score: the explicit workspaces
def test_locate_cameras(capsys):
    """every case of locate_cameras_cases.gpu_cases() (n63 / n64_j64 / n65, small_h1 / h63 / h64 / h65, v32), the corner V = 32 with
    J = 64, with the polish and with the hypotheses handed out; the added corner is checked through the checker of
    tests/test_locate_cameras_gpu.py, the restated steps on the device's own poses"""
    from openmpl_amd import locate_cameras
    from tests import locate_cameras_cases as lc
    cases = dict(lc.gpu_cases(), v32_j64=lc.case(1, 32, 64, name="per_view", hypotheses=16))
    stats = []
    for name in sorted(cases):
        c = cases[name]
        B, V, J = c["pixels"].shape[:3]
        ws = _lib().mpl_locate_cameras_workspace_bytes(B, V, J)
        args = dict(points=c["points"], pixels=c["pixels"], conf=c["conf"], cams=c["cams"], distortion=c["dist"])
        for kw in (dict(return_hypotheses=True), dict(refine=True, huber=2.5)):
            r, n, b = G.run_contract(lambda **a: locate_cameras(**a, **lc.call_args(c), **kw), args, workspace_bytes=(ws,),
                                     min_outputs=(8 if "return_hypotheses" in kw else 6 + 7))
            stats.append((n, b))
            assert int(r.best.min()) >= -1 and int(r.best.max()) < c["hypotheses"] and int(r.status.max()) <= 3
        if name == "v32_j64":
            from tests.test_locate_cameras_gpu import _check_against_own_poses, _locate
            _check_against_own_poses(c, _locate(c)[0])
    _report("locate_cameras", stats, capsys)


def test_relative_pose_and_its_polish(capsys):
    """every case of relative_pose_cases.gpu_cases(), the corner J = 64 under all 32 pair slots, 255 / 256 / 257 correspondences
    (the polish strides 256 threads over them), with the polish and with the hypotheses handed out; refine_relative_pose alone
    from the poses of the hypothesis stage"""
    from openmpl_amd import refine_relative_pose, relative_pose
    from tests import relative_pose_cases as rp
    v32 = tuple((0, v) for v in range(1, 17)) + tuple((v, 0) for v in range(17, 32)) + ((1, 0),)
    cases = dict(rp.gpu_cases(), v32_j64=rp.case(1, 32, 64, pairs=v32, name="per_view", hypotheses=16), n255=rp.case(15, 2, 17, hypotheses=16),
                 n256=rp.case(16, 2, 16, hypotheses=16), n257=rp.case(257, 2, 1, hypotheses=16))
    stats, polish = [], []
    for name in sorted(cases):
        c = cases[name]
        B, V, J = c["pixels"].shape[:3]
        P = len(c["pairs"])
        ws = _lib().mpl_relative_pose_workspace_bytes(B, P, J)
        args = dict(pixels=c["pixels"], conf=c["conf"], cams=c["cams"], distortion=c["dist"])
        for kw in (dict(return_hypotheses=True), dict(refine=True, huber=2.5, baseline=2.0)):
            r, n, b = G.run_contract(lambda **a: relative_pose(**a, **rp.call_args(c), **kw), args, workspace_bytes=(ws,),
                                     min_outputs=(11 if "return_hypotheses" in kw else 8 + 9))
            stats.append((n, b))
            assert int(r.best.min()) >= -1 and int(r.best.max()) < c["hypotheses"] and int(r.status.max()) <= 3
        start = relative_pose(**G.plain(args, "cuda"), **rp.call_args(c))
        # the poses of the hypothesis stage as they are: NaN where a pair is invalid, which the polish documents as its status 3
        args2 = dict(args, rotation=start.rotation.cpu().numpy(), direction=start.direction.cpu().numpy(), weight=start.inliers.cpu().numpy())
        _, n, b = G.run_contract(lambda **a: refine_relative_pose(pairs=c["pairs"], max_iterations=6, **a), args2, min_outputs=9)
        polish.append((n, b))
    _report("relative_pose", stats, capsys)
    _report("refine_relative_pose", polish, capsys)


def _rpsm_corner(rc):
    """the envelope corner the case table lacks, V = 32 with J = 64 at B = 2: the 17 maps of a 32-view case four times over, on a
    chain of 64 joints (the contract needs arguments the call accepts, no restatement)"""
    inp = rc.inputs(B=2, V=32, H=8, W=8, first_nbins=3, recur_depth=1, grid_size=900.0, tolerance=350.0, per_sample_limbs=True)
    inp["hm"] = np.ascontiguousarray(np.tile(inp["hm"], (1, 1, 4, 1, 1))[:, :, :64])
    inp["parents"] = [-1] + list(range(63))
    inp["limb"] = np.full((2, 64), 250.0, np.float32)
    return inp


def test_rpsm(capsys):
    """the cases of tests/test_rpsm_gpu.py that differ in what is launched and allocated: bin counts below a wave, ragged against a
    wave and against 256 threads, every tree, B = 3 with per-sample limbs, 8 x 8 and 64 x 48 maps, a lens, a NaN; 16-bit maps and
    a list of views"""
    import openmpl_amd
    from tests import rpsm_cases as rc
    stats = []
    for name, dtype, as_list in [(k, None, False) for k in ("n2", "n3", "n5", "n11", "single", "chain_r3", "depth0", "batch3", "small_maps",
                                                             "nonsquare", "distorted", "nan", "v32_j64")] + [("batch3", torch.float16, True), ("n5", torch.bfloat16, False)]:
        inp = rc.attempt_inputs(name, 0) if name != "v32_j64" else _rpsm_corner(rc)
        B, V, J = inp["hm"].shape[:3]
        hm = torch.from_numpy(inp["hm"].astype(np.float32))
        hm = hm if dtype is None else hm.to(dtype)
        args = dict(heatmaps=[hm[:, v].contiguous() for v in range(V)] if as_list else hm, center=inp["center"], scale=inp["scale"],
                    cams=inp["cams"], root_center=inp["root_center"], limb_length=inp["limb"], distortion=inp["dist"])
        ws = _lib().mpl_rpsm_workspace_bytes(B, J, inp["kw"]["first_nbins"])
        r, n, b = G.run_contract(lambda **a: openmpl_amd.rpsm(image_size=inp["image_size"], parents=inp["parents"], **a, **inp["kw"]), args,
                                 workspace_bytes=(ws,), min_outputs=3)
        nb = max(inp["kw"]["first_nbins"], inp["kw"]["recur_nbins"]) ** 3
        assert r.bins.dtype == torch.int32 and int(r.bins.min()) >= 0 and int(r.bins.max()) < nb
        stats.append((n, b))
    _report("rpsm", stats, capsys)


# ------------------------------------------------------------------------------------------------------------------- heatmaps
def test_decode_heatmaps(capsys):
    from openmpl_amd import decode_heatmaps
    from tests import heatmap_cases as hc
    from tests import synth_cases as sc
    from tests.test_heatmaps_gpu import SHAPES
    stats = []
    for shape in list(SHAPES) + [(1, 1, 1, 8, 8), (1, 1, 3, 64, 64), (1, 2, 2, 64, 64), (1, 1, 5, 64, 64), (1, 32, 64, 8, 8)]:
        B, V, J, H, W = shape
        hm, center, scale = hc.batch(*shape, seed=0)
        _, cams = sc.scene(B, V, J, seed=1)
        dist = np.tile(np.array([-0.1, 0.02, 0.0, 0.001, -0.001]), (V, 1))
        variants = [(torch.float32, False, dict(return_coords=True)), (torch.float32, True, dict(post_process=True, return_coords=True)),
                    (torch.float32, True, dict(cams=cams, image_size=(1000.0, 1000.0))),
                    (torch.float32, True, dict(cams=cams, image_size=(1000.0, 800.0), distortion=dist, normalize_cameras=False)),
                    (torch.float32, False, dict(subpixel="gaussian", return_coords=True)),
                    (torch.float32, True, dict(subpixel="centroid", radius=3, cams=cams, image_size=(1000.0, 1000.0))),
                    (torch.float16, True, dict(post_process=True)), (torch.bfloat16, False, dict(subpixel="gaussian"))]
        for dtype, boxes, kw in variants:
            kw = dict(kw)
            extra = {k: kw.pop(k) for k in ("cams", "distortion") if k in kw}
            args = dict(heatmaps=torch.from_numpy(np.array(hm)).to(dtype), center=center if boxes else None, scale=scale if boxes else None, **extra)
            outs = 2 + ("return_coords" in kw) + (3 * V if "cams" in extra else 0)
            _, n, b = G.run_contract(lambda **a: decode_heatmaps(**a, **kw), args, min_outputs=outs)
            stats.append((n, b))
    _report("decode_heatmaps", stats, capsys)


def test_render_heatmaps(capsys):
    from openmpl_amd import render_heatmaps
    from tests import render_cases as rc
    from tests.test_render_gpu import SHAPES
    stats = []
    for shape in list(SHAPES) + [(1, 1, 1, 8, 8), (1, 1, 3, 64, 64), (1, 2, 2, 64, 64), (1, 1, 5, 64, 64), (1, 32, 64, 8, 8)]:
        B, V, J, H, W = shape
        cells, conf = rc.joints(B, V, J, W, H)
        center, scale = rc.boxes(B, V)
        k = scale[..., 0].astype(np.float64) * 200.0 / W
        with np.errstate(invalid="ignore"):
            boxed = (center.astype(np.float64)[:, :, None] + (cells.astype(np.float64) - np.array([W * 0.5, H * 0.5])) * k[:, :, None, None]).astype(np.float32)
        for pixels, cf, boxes, kw in ((cells, conf, False, dict(mode="reference")), (boxed, conf, True, dict(mode="subpixel")),
                                      (cells, None, False, dict(mode="subpixel", stride=(1.0, 1.0), noise_level=0.01, seed=3)),
                                      (boxed, conf, True, dict(mode="reference", dtype=torch.float16)),
                                      (boxed, conf, True, dict(mode="subpixel", dtype=torch.bfloat16, noise_level=0.01))):
            args = dict(pixels=pixels, conf=cf, center=center if boxes else None, scale=scale if boxes else None)
            r, n, b = G.run_contract(lambda **a: render_heatmaps(heatmap_size=(W, H), **a, **kw), args, min_outputs=3)
            assert r.heatmaps.shape == shape
            stats.append((n, b))
    _report("render_heatmaps", stats, capsys)


# --------------------------------------------------------------------------------------------------------- 256 threads over B V J
POINTWISE_EDGES = [(5, 3, 17), (4, 4, 16), (257, 1, 1), (19, 3, 9), (1, 32, 64)]        # 255, 256, 257, 513; the envelope corner


def test_synthesize_views_and_project_points(capsys):
    from openmpl_amd import project_points, synthesize_views
    from tests import distortion_cases as dc
    from tests import synth_cases as sc
    from tests.test_synth_gpu import OWN, OWN_SHAPES
    stats, proj = [], []
    for B, V, J in list(OWN_SHAPES) + POINTWISE_EDGES:
        poses3d, cams = sc.scene(B, V, J, seed=5, focal=2400.0)
        dist = dc.table("h36m", V)
        conf = (0.5 + 0.5 * sc.draw(5, "test.conf", 0, np.arange(B * V * J)).reshape(B, V, J)).astype(np.float32)
        for kw, extra in ((dict(OWN, seed=17, first_index=1000003, return_pixels=True), dict()),
                          (dict(OWN, seed=17, clip=False, normalize_cameras=False), dict(conf=conf, distortion=dist)),
                          (dict(return_pixels=True, normalize_inputs=False), dict(distortion=dist))):
            args = dict(poses3d=poses3d, cams=cams, **extra)
            _, n, b = G.run_contract(lambda **a: synthesize_views(image_size=(1000.0, 1000.0), **a, **kw), args,
                                     min_outputs=3 * V + 1 + (2 if kw.get("return_pixels") else 0))
            stats.append((n, b))
        for lens in (None, dist):
            _, n, b = G.run_contract(lambda **a: project_points(**a), dict(points3d=poses3d, cams=cams, distortion=lens), min_outputs=2)
            proj.append((n, b))
    _report("synthesize_views", stats, capsys)
    _report("project_points", proj, capsys)


def test_undistort_and_distort_points(capsys):
    from openmpl_amd.inputs import distort_points, undistort_points
    from tests import distortion_cases as dc
    from tests.test_distortion_gpu import SHAPES
    stats = []
    for B, V, J in list(SHAPES) + POINTWISE_EDGES:
        for name, every in (("h36m", 0), ("strong", 5)):
            c = dc.case(B, V, J, name, invalid_every=every if B * V * J >= 5 else 0)
            args = dict(pixels=c["pixels"], cams=c["cams"], distortion=c["dist"])
            (px, valid), n, b = G.run_contract(lambda **a: undistort_points(**a), args, min_outputs=2)
            assert valid.dtype == torch.bool and np.array_equal(valid.cpu().numpy(), c["valid"])
            stats.append((n, b))
            _, n, b = G.run_contract(lambda **a: distort_points(**a), args, min_outputs=1)
            stats.append((n, b))
    _report("undistort_points / distort_points", stats, capsys)


def test_prepare_inputs(capsys):
    """the thread-count edges of tests/test_inputs.py (255 / 256 / 257 / 513 points, V = 32 with J = 64, one point), whose values
    that file holds against the float64 oracle; conf=None; with and without the lens"""
    from openmpl_amd.inputs import prepare_inputs
    from tests import distortion_cases as dc
    from tests.test_inputs import EDGE_SHAPES, EDGE_WH, edge_case
    stats = []
    for name in sorted(EDGE_SHAPES):
        px, conf, cams = edge_case(name)
        V = px.shape[1]
        for cf, lens, ni, nc in ((conf, None, True, True), (None, None, True, False), (conf, dc.table("h36m", V), False, False)):
            args = dict(joints_px=px, conf=cf, cams=cams, distortion=lens)
            _, n, b = G.run_contract(lambda **a: prepare_inputs(image_size=EDGE_WH, normalize_inputs=ni, normalize_cameras=nc, **a), args,
                                     min_outputs=3 * V)
            stats.append((n, b))
    _report("prepare_inputs", stats, capsys)


def test_pose_metrics(capsys):
    """both geometries of pose_metrics_kernel at the cases of tests/test_metrics.py, whose values that file holds against the
    float64 oracle: B below, at and above the slice counts, with weight, scale and offset, a skip mask, NaN joints"""
    from openmpl_amd.metrics import pose_metrics
    from tests.test_metrics import METRIC_J, metric_case
    stats = []
    for J in METRIC_J:
        for B, variant in ((1, "plain"), (14, "weight"), (15, "scaled"), (16, "skip"), (61, "nan_joint"), (3, "nan_root")):
            mc = metric_case(J, B, variant)
            if mc is None:
                continue
            out, tgt, kw = mc
            args = dict(output=out, target=tgt, weight=kw.get("w"))
            res, n, b = G.run_contract(lambda **a: pose_metrics(scale=kw.get("scale"), offset=kw.get("offset"),
                                                                not_consider_kp=kw.get("not_consider_kp"), **a), args, min_outputs=8)
            assert sum(t.numel() for t in res.values()) == _lib().mpl_pose_metrics_size(J)
            stats.append((n, b))
    _report("pose_metrics", stats, capsys)


# ======================================================================================================================= the forward
# The plain ctypes route (use_torch_op(False)) with a FRESH module per run, whose first forward happens between the guards: the
# struct blob and every packed operand of _marshal (mpl_spt_pack, mpl_d32_pack, mpl_pack_h2 / _scaled, mpl_pack_bf16 / _any) are
# guarded allocations like `out`, `ws`, `xs` and the staged intermediates, and the workspace is handed over as NaN bytes.  One
# model per path; the library is asked which path the launch took (mpl_block_stack_last_form, mpl_spt_form) and the test fails if
# the form it is there for was not reached.  Batches: the smallest the library's own rule sends to the form on this device.
# The table of models, one per path, is tests/forward_paths.py, which tests/test_nonfinite_gpu.py visits too.
from tests.forward_paths import DEV, FORWARD_MODELS, _fresh_model, _stack_shape  # noqa: E402

FORWARD_CALLS = ("mpl_forward", "mpl_spt_tokens", "mpl_block_stack_ex", "mpl_view_norm", "mpl_view_fuse", "mpl_layernorm", "mpl_linear")


@pytest.mark.parametrize("name", sorted(FORWARD_MODELS))
def test_forward(name, capsys):
    import ctypes as C
    from openmpl_amd import cabi, detrng
    flags, prec, small, want_stack, want_spt, B = FORWARD_MODELS[name]
    lib = cabi.load()
    V, J, L, H = flags["num_views"], flags["num_joints"], flags["depth"], flags["num_heads"]
    n_tok, D = _stack_shape(flags)
    parts = {"fp32": 2, "bf16": 1, "fp32_mfma": 0}[prec]
    sflags = 0 if small == "auto" else cabi.F_NO_SMALL_STACK
    if B is None:
        form = getattr(cabi, "FORM_" + want_stack)
        B = next((b for b in range(1, 4097) if lib.mpl_block_stack_form(b, n_tok, D, H, L + 1, parts, sflags) == form), None)
        assert B is not None, "%s: no batch up to 4096 is sent to %s on this device" % (name, want_stack)
    p, r, c = detrng.make_inputs(B, V, J, seed=5)
    seen = {}

    def call(poses, rays, centers):
        m = _fresh_model(flags, prec, small)
        with torch.no_grad():
            out = m(poses, rays=rays, centers=centers)
        torch.cuda.synchronize()
        ent = m._hip_cache[torch.device(DEV).index]
        spw = C.c_int(0)
        seen["stack"] = lib.mpl_block_stack_last_form()
        seen["spt"] = lib.mpl_spt_form(C.byref(ent["cfg"]), B, int(ent["weights"].spt_packed), 0, C.byref(spw))
        seen["cfg"] = ent["cfg"]
        return out

    def after(g, result):
        # the blobs of _marshal and the workspace of this route are among the guarded allocations
        sizes = [a.nbytes for a in g.allocations if a.dtype == torch.uint8]
        staged = bool(flags.get("linear_weighted_mean") or flags.get("deep_head") or flags.get("head_kadkhod"))
        ws = lib.mpl_block_stack_workspace_bytes(B, n_tok, D) if staged else lib.mpl_forward_workspace_bytes(C.byref(seen["cfg"]), B)
        assert ws in sizes, "%s: no guarded workspace of %d bytes among %s" % (name, ws, sizes)
        assert len(sizes) >= 2, "%s: the struct blob of _marshal is not guarded" % name
        if prec != "fp32_mfma" and (J, flags["embed_dim_ratio"], H) == (17, 32, 8):
            assert sizes.count(lib.mpl_spt_pack_bytes()) >= L, "%s: the packed SPT operands are not guarded" % name
        if staged:
            assert any(a.kind == "empty_like" for a in g.allocations), "%s: the staged route's empty_like is not guarded" % name

    _, n, b = G.run_contract(call, dict(poses=list(p), rays=list(r), centers=list(c)), min_outputs=1,
                             record=[(lib, f) for f in FORWARD_CALLS], after=after)
    if want_stack is not None:
        assert seen["stack"] == getattr(cabi, "FORM_" + want_stack), "%s: the stack took form %d" % (name, seen["stack"])
    assert seen["spt"] in {getattr(cabi, "SPT_" + s) for s in want_spt}, "%s: the SPT stage took form %d" % (name, seen["spt"])
    with capsys.disabled():
        print("\nforward %s: B = %d, stack form %s, SPT form %d, %d guarded allocations, %d bytes" % (name, B, seen["stack"], seen["spt"], n, b))


# ================================================================================= the added corners against the float64 restatements
# The contract ties a guarded call to the plain call bit for bit, and the plain call is what each entry point's own test file ties to
# its float64 restatement -- on that file's shapes.  The corners added above are therefore run through the same checkers here.
def _dev(x):
    return None if x is None else torch.from_numpy(np.array(x)).cuda()


def test_added_corners_of_the_lines_of_sight_and_the_points():
    from tests import refine_cases as rc
    from tests import robust_tri_cases as rt
    from tests import test_refine_gpu as tr
    from tests import test_triangulate_robust_gpu as tt
    for (B, V, J), n_out in ROBUST_EDGES:
        configs = ((True, None),) if V == 32 else ((False, None), (True, None), (True, 0.5))
        c = rt.outlier_case(B, V, J, n_out=n_out, seed=3, n_zero=max(1, B * V * J // 25), configs=configs)      # asserts its margins
        flat = [c["conf"][v] for v in range(V)]
        for with_conf, cth in configs:
            x, res, inl = tt._run(tt._dev(c["rays"]), tt._dev(c["centers"]), tt._dev(flat) if with_conf else None, threshold=c["tau"],
                                  conf_threshold=cth)
            x_ref, r_ref, i_ref = rt.robust(c["rays"], c["centers"], flat if with_conf else None, c["tau"], cth)
            what = "B%d V%d J%d conf %s sel %s" % (B, V, J, with_conf, cth)
            assert np.array_equal(inl, i_ref), what
            tt._assert_parity(x, x_ref, "points " + what)
            tt._assert_parity(res, r_ref, "residual " + what)
    for B, V, J in POINT_EDGES:
        c = _point_case(B, V, J, "mixed")
        ref = rc.refine(c["points0"], c["pixels"], c["conf"], c["cams"], c["dist"], tr.HUBER)
        got, n = tr._run(c, huber=tr.HUBER)
        what = "%s huber conf=mixed" % ((B, V, J),)
        assert n == 1, what
        tr._assert_parity(got, ref, what)
        assert np.array_equal(got["status"] == 2, ref["status"] == 2) and np.array_equal(got["status"] == 3, ref["status"] == 3), what
        tr._assert_cost_did_not_rise(got, c, c["conf"], tr.HUBER, what)


def test_added_corners_of_the_camera_and_pose_refinements():
    from tests import refine_poses_cases as pc
    from tests import test_refine_cameras_gpu as tc
    from tests import test_refine_poses_gpu as tp
    for B, V, J in CAMERA_EDGES:
        tc._parity(B, V, J, "h36m", True, ("none",), (None,))
    B, V, J, kind = 2, 32, 64, "random"
    c, ref, kw = pc.parity_case(B, V, J, kind, "h36m", "none", "pose", None)
    got, n = tp._run(c, **kw)
    what = "%s plain" % ((B, V, J, kind),)
    assert n == 1, what
    tp._assert_parity(got, ref, what)
    assert np.array_equal(got["status"], ref["status"]), what
    tp._assert_cost_did_not_rise(got, c, None, kw["bone_weight"], True, what)


def test_added_corners_of_relative_pose():
    from tests import relative_pose_cases as rp
    from tests import test_relative_pose_gpu as tr
    v32 = tuple((0, v) for v in range(1, 17)) + tuple((v, 0) for v in range(17, 32)) + ((1, 0),)
    for c in (rp.case(1, 32, 64, pairs=v32, name="per_view", hypotheses=16), rp.case(257, 2, 1, hypotheses=16)):
        tr._check_against_own_poses(c, tr._relative(c)[0])


def test_added_corners_of_the_heatmaps_and_the_lens():
    from openmpl_amd import decode_heatmaps, distort_points, project_points, render_heatmaps, undistort_points
    from tests import distortion_cases as dc
    from tests import heatmap_cases as hc
    from tests import render_cases as rc
    from tests import synth_cases as sc
    from tests import test_distortion_gpu as td
    from tests import test_heatmaps_gpu as th
    from tests import test_render_gpu as tr
    for shape in [(1, 1, 1, 8, 8), (1, 1, 3, 64, 64), (1, 2, 2, 64, 64), (1, 1, 5, 64, 64), (1, 32, 64, 8, 8)]:
        B, V, J, H, W = shape
        hm, center, scale = hc.batch(*shape, seed=0)
        for post in (False, True):
            r = decode_heatmaps(_dev(hm), _dev(center), _dev(scale), post_process=post, return_coords=True)
            th._check(r, hc.decode(hm, center, scale, post), "%s post=%s" % (shape, post))
        cells, conf = rc.joints(B, V, J, W, H)
        for mode in ("reference", "subpixel"):
            r = render_heatmaps(_dev(cells), _dev(conf), heatmap_size=(W, H), mode=mode)
            tr._check(r, rc.render(cells, conf, None, None, heatmap_size=(W, H), sigma=2.0, mode=mode, fmt="fp32"), "fp32", mode,
                      "%s %s" % (shape, mode))
    for B, V, J in POINTWISE_EDGES:
        c = dc.case(B, V, J, "strong", invalid_every=5)
        X, Cm, D = _dev(c["pixels"]), _dev(c["cams"]), _dev(c["dist"])
        out, valid = undistort_points(X, Cm, D)
        assert np.array_equal(valid.cpu().numpy(), c["valid"])
        td._within_one_ulp(out.cpu().numpy(), c["restated"]["pixels"], "undistort_points %s" % ((B, V, J),))
        pin = dc.project(c["points"], c["cams"], dc.table("zeros", V))[0].astype(np.float32)
        td._within_one_ulp(distort_points(_dev(pin), Cm, D).cpu().numpy(), dc.distort_pixels(pin, c["cams"], c["dist"]),
                           "distort_points %s" % ((B, V, J),))
        px, depth = project_points(_dev(c["points"]), Cm, distortion=D)
        ref_px, ref_depth = dc.project(c["points"], c["cams"], c["dist"])
        sc.assert_matches(dict(pixels_clean=px.cpu().numpy(), depth=depth.cpu().numpy()), dict(pixels_clean=ref_px, depth=ref_depth))
