"""decode_heatmaps(subpixel=...) (csrc/heatmaps.hip) on the device: against the float64 restatement of tests/render_cases.py
(confidences bit for bit, coordinates and pixels within 1 float32 ulp on well-conditioned cases), across layouts, forms and
dtypes bit for bit, against prepare_inputs for the fused outputs, and in a closed loop behind project_points and render_heatmaps."""
import functools

import numpy as np
import pytest
import torch

from tests import heatmap_cases as hc
from tests import render_cases as rc
from tests import synth_cases as sc

pytestmark = pytest.mark.gpu

# B, V, J, H, W: the shapes of tests/test_heatmaps_gpu.py
SHAPES = [(2, 2, 3, 8, 8), (1, 3, 17, 64, 64), (2, 2, 2, 64, 48), (1, 2, 3, 5, 7), (1, 1, 2, 128, 128), (1, 2, 2, 96, 72)]
ESTIMATORS = [("gaussian", 2), ("centroid", 1), ("centroid", 2), ("centroid", 8)]
WH = (1000.0, 1000.0)
IDS = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)


def _dev(x):
    return None if x is None else torch.from_numpy(np.array(x)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


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


@functools.lru_cache(maxsize=None)
def _maps(shape, seed=0):
    hm, center, scale = hc.batch(*shape, seed=seed)
    for a in (hm, center, scale):
        a.setflags(write=False)
    return hm, center, scale


@functools.lru_cache(maxsize=None)
def _ref(shape, subpixel, radius, boxes, seed=0):
    """the restatement, computed once; the case must be well conditioned (render_cases.well_conditioned): then the float64 offset
    of either side is good to far below a float32 ulp of the coordinate, and 1 ulp is the rounding alone"""
    hm, center, scale = _maps(shape, seed)
    r = rc.decode(hm, center if boxes else None, scale if boxes else None, subpixel, radius)
    assert rc.well_conditioned(r, subpixel), (shape, subpixel, radius, r["cond"])
    return r


def _check(r, ref, what):
    coords, conf, pixels = r.coords.cpu().numpy(), r.conf.cpu().numpy(), r.pixels.cpu().numpy()
    assert np.array_equal(conf, ref["maxval"], equal_nan=True), what
    plain = ~ref["refined"]
    assert np.array_equal(coords[plain], ref["coords"][plain]), what            # where no refinement applies: the integer peak or (0, 0)
    uc, up = hc.ulps(coords, ref["coords"]), hc.ulps(pixels, ref["pixels"])
    print("%s: %d of %d coords and %d pixel entries differ from the restatement, at most %.1f / %.1f ulp"
          % (what, int((uc > 0).sum()), uc.size, int((up > 0).sum()), uc.max(), up.max()))
    assert uc.max() <= 1.0 and up.max() <= 1.0, what


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("subpixel,radius", ESTIMATORS)
@pytest.mark.parametrize("boxes", [False, True])
def test_matches_the_restatement_in_one_launch(shape, subpixel, radius, boxes):
    from openmpl_amd import decode_heatmaps
    hm, center, scale = _maps(shape)
    ref = _ref(shape, subpixel, radius, boxes)
    c, s = (_dev(center), _dev(scale)) if boxes else (None, None)
    r, n = _launches(lambda: decode_heatmaps(_dev(hm), c, s, subpixel=subpixel, radius=radius, return_coords=True))
    assert n == 1 and r.poses is None
    _check(r, ref, "%s %s r=%d boxes=%s" % (shape, subpixel, radius, boxes))
    if not boxes:
        assert _same_bits(r.pixels, r.coords)
    assert ref["refined"].any() and (ref["coords"][ref["refined"]] != np.round(ref["coords"][ref["refined"]])).any()


def test_subpixel_none_is_the_plain_decode():
    from openmpl_amd import decode_heatmaps
    hm, center, scale = _maps((1, 3, 17, 64, 64))
    for post in (False, True):
        a = decode_heatmaps(_dev(hm), _dev(center), _dev(scale), post_process=post, return_coords=True)
        b = decode_heatmaps(_dev(hm), _dev(center), _dev(scale), post_process=post, return_coords=True, subpixel=None, radius=5, threshold=0.5)
        for k in ("pixels", "conf", "coords"):
            assert _same_bits(getattr(a, k), getattr(b, k)), k


@pytest.mark.parametrize("subpixel,radius", ESTIMATORS)
def test_every_special_and_edge_map(subpixel, radius):
    """NaN, -inf, all-zero and non-positive maps keep the plain decode's (0, 0); a +inf peak keeps its integer peak; peaks on every
    border and one cell inside it get what the rule gives them"""
    from openmpl_amd import decode_heatmaps
    for H, W in ((64, 64), (5, 7), (16, 12)):
        special = hc.special_maps(H, W)
        inf = special[0].copy()
        inf[H // 2, W // 2] = np.inf
        hm = np.concatenate([special, inf[None], hc.edge_maps(H, W)])[None, None]          # (1,1,33,H,W)
        ref = rc.decode(hm, None, None, subpixel, radius)
        assert rc.well_conditioned(ref, subpixel)
        assert not ref["refined"][0, 0, 1:8].any() and ref["refined"][0, 0, 0] and ref["refined"][0, 0, 8:].all()
        assert np.array_equal(ref["coords"][0, 0, 7], np.float32([W // 2, H // 2])) and not ref["coords"][0, 0, 1:7].any()
        _check(decode_heatmaps(_dev(hm), subpixel=subpixel, radius=radius, return_coords=True), ref, "%dx%d %s r=%d" % (H, W, subpixel, radius))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("shape", [(1, 3, 17, 64, 64), (1, 2, 3, 5, 7), (2, 2, 2, 64, 48), (1, 1, 2, 256, 128)], ids=IDS)
@pytest.mark.parametrize("subpixel,radius", [("gaussian", 2), ("centroid", 2)])
def test_16_bit_maps_equal_their_fp32_upcast(dtype, shape, subpixel, radius):
    """(1,1,2,256,128): 64 KiB of 16-bit values, the four-wave form; 64x64: one wave, eight chunks per lane; 5x7: element-wise.  The
    two forms are set against each other in test_one_wave_and_four_wave_forms_agree_bitwise."""
    from openmpl_amd import decode_heatmaps
    hm, center, scale = _maps(shape)
    low = _dev(hm).to(dtype)
    up = low.float()
    kw = dict(subpixel=subpixel, radius=radius, return_coords=True)
    a = decode_heatmaps(low, _dev(center), _dev(scale), **kw)
    b = decode_heatmaps(up, _dev(center), _dev(scale), **kw)
    for k in ("pixels", "conf", "coords"):
        assert _same_bits(getattr(a, k), getattr(b, k)), k
    ref = rc.decode(up.cpu().numpy(), center, scale, subpixel, radius)
    assert rc.well_conditioned(ref, subpixel)
    _check(a, ref, "%s %s %s" % (dtype, shape, subpixel))


@pytest.mark.parametrize("subpixel,radius", ESTIMATORS)
def test_one_wave_and_four_wave_forms_agree_bitwise(subpixel, radius):
    """128 x 128 maps of bfloat16-representable values: as float32 they are 64 KiB and take the four-wave form, as bfloat16 32 KiB
    and the one-wave form; both widen to the same values, so every output must be the same bits"""
    from openmpl_amd import decode_heatmaps
    from openmpl_amd import cabi
    hm, center, scale = _maps((2, 2, 3, 128, 128))
    low = _dev(hm).to(torch.bfloat16)
    up = low.float()
    assert up[0, 0, 0].numel() * 4 >= 65536 > low[0, 0, 0].numel() * 2
    cams = _dev(sc.scene(2, 2, 3, seed=4)[1])
    kw = dict(subpixel=subpixel, radius=radius, return_coords=True, cams=cams, image_size=WH)
    a = decode_heatmaps(low, _dev(center), _dev(scale), **kw)
    b = decode_heatmaps(up, _dev(center), _dev(scale), **kw)
    for k in ("pixels", "conf", "coords"):
        assert _same_bits(getattr(a, k), getattr(b, k)), k
    for k in ("poses", "rays", "centers"):
        for v in range(2):
            assert _same_bits(getattr(a, k)[v], getattr(b, k)[v]), k
    ref = rc.decode(up.cpu().numpy(), center, scale, subpixel, radius)
    assert rc.well_conditioned(ref, subpixel)
    _check(b, ref, "four-wave form %s r=%d" % (subpixel, radius))


@pytest.mark.parametrize("subpixel,radius", [("gaussian", 2), ("centroid", 2), ("centroid", 8)])
def test_sub_batches_layouts_and_reruns_bitwise(subpixel, radius):
    from openmpl_amd import decode_heatmaps
    shape = (3, 2, 5, 64, 48)
    hm, center, scale = _maps(shape)
    t, c, s = _dev(hm), _dev(center), _dev(scale)
    cams = _dev(sc.scene(3, 2, 5, seed=4)[1])
    kw = dict(subpixel=subpixel, radius=radius, return_coords=True, cams=cams, image_size=WH)
    whole, again = decode_heatmaps(t, c, s, **kw), decode_heatmaps(t, c, s, **kw)
    part = decode_heatmaps(t[1:], c[1:], s[1:], **kw)
    views = decode_heatmaps(list(t.unbind(1)), c, s, **kw)
    swapped = decode_heatmaps(t.transpose(0, 1).contiguous().transpose(0, 1), c, s, **kw)
    odd = torch.empty(t.numel() + 1, device="cuda")[1:].view(t.shape).copy_(t)                # unaligned bases: element-wise loads
    assert odd.data_ptr() % 16 != 0
    unaligned = decode_heatmaps(odd, c, s, **kw)
    for k in ("pixels", "conf", "coords"):
        assert _same_bits(getattr(whole, k), getattr(again, k)), k
        assert _same_bits(getattr(whole, k)[1:], getattr(part, k)), k
        assert _same_bits(getattr(whole, k), getattr(views, k)), k
        assert _same_bits(getattr(whole, k), getattr(swapped, k)), k
        assert _same_bits(getattr(whole, k), getattr(unaligned, k)), k
    for k in ("poses", "rays", "centers"):
        for v in range(2):
            assert _same_bits(getattr(whole, k)[v], getattr(again, k)[v]) and _same_bits(getattr(whole, k)[v][1:], getattr(part, k)[v]), k
            assert _same_bits(getattr(whole, k)[v], getattr(views, k)[v]) and _same_bits(getattr(whole, k)[v], getattr(swapped, k)[v]), k


@pytest.mark.parametrize("subpixel,radius", [("gaussian", 2), ("centroid", 3)])
@pytest.mark.parametrize("normalize_inputs,normalize_cameras", [(True, True), (False, False)])
def test_fused_outputs_are_prepare_inputs_bitwise(subpixel, radius, normalize_inputs, normalize_cameras):
    from openmpl_amd import decode_heatmaps
    from openmpl_amd.inputs import prepare_inputs
    shape = (2, 3, 5, 64, 64)
    hm, center, scale = _maps(shape)
    cams = _dev(sc.scene(2, 3, 5, seed=4)[1])
    kw = dict(normalize_inputs=normalize_inputs, normalize_cameras=normalize_cameras)
    r, n = _launches(lambda: decode_heatmaps(_dev(hm), _dev(center), _dev(scale), subpixel=subpixel, radius=radius, cams=cams, image_size=WH, **kw))
    assert n == 1 and r.coords is None
    plain = decode_heatmaps(_dev(hm), _dev(center), _dev(scale), subpixel=subpixel, radius=radius)
    assert _same_bits(plain.pixels, r.pixels) and _same_bits(plain.conf, r.conf)
    assert bool(torch.isnan(r.conf).any()) and bool((r.conf > 0).any())
    poses, rays, centers = prepare_inputs(r.pixels, r.conf, cams, WH, **kw)
    for v in range(3):
        assert _same_bits(r.poses[v], poses[v]) and _same_bits(r.rays[v], rays[v]) and _same_bits(r.centers[v], centers[v])


def test_closed_loop_on_the_device():
    """poses -> project_points -> render_heatmaps(mode="subpixel") -> decode_heatmaps -> the pixels again, then on through cams= and
    triangulate_rays to the poses; nothing leaves the device in between.  With the log-quadratic fit every interior joint must land
    within 0.01 cell: a cap, 25 times under the quarter shift's bound (the restatement's worst on clean float32 maps is about
    1e-6 cell); the plain decode exceeds 0.25 cell somewhere.  The 3D error follows: printed, and recorded in DESIGN.md section 7."""
    from openmpl_amd import decode_heatmaps, detrng, project_points, render_heatmaps, triangulate_rays
    B, V, J, H, W = 2, 3, 17, 64, 64
    poses3d, cams = sc.scene(B, V, J, seed=9, focal=600.0)
    center = (500.0 + detrng.uniform(1, "loop.center", (B, V, 2), -20.0, 20.0)).astype(np.float32)
    scale = detrng.uniform(1, "loop.scale", (B, V, 2), 5.0, 5.5)                  # k = 15.6 .. 17.2 px per cell
    P, Cm, c, s = _dev(poses3d), _dev(cams), _dev(center), _dev(scale)
    true, depth = project_points(P, Cm)
    assert bool((depth > 0).all())
    k = torch.from_numpy((scale[..., 0].astype(np.float64) * 200.0 / W)[:, :, None, None]).cuda()
    target = P.double()

    def run(noise, **kw):
        maps, n = _launches(lambda: render_heatmaps(true, None, c, s, heatmap_size=(W, H), mode="subpixel", noise_level=noise, seed=3))
        assert n == 1
        cells = maps.cells.double()
        interior = ((cells >= 3.0) & (cells <= torch.tensor([W - 4.0, H - 4.0], device="cuda"))).all(-1)
        assert int(interior.sum()) > 0.7 * interior.numel()
        r = decode_heatmaps(maps.heatmaps, c, s, cams=Cm, image_size=WH, **kw)
        err = ((r.pixels.double() - true.double()).abs() / k)[interior]                       # per axis, in cells
        pts, _ = triangulate_rays(r.rays, r.centers)
        seen = interior.all(1)                                                                # joints interior in every view
        e3d = (pts.double() - target).norm(dim=-1)[seen]
        assert int(seen.sum()) > 0.5 * seen.numel() and bool(torch.isfinite(e3d).all())
        return float(err.max()), float(err.mean()), float(e3d.mean())

    clean = {name: run(0.0, **kw) for name, kw in (("gaussian", dict(subpixel="gaussian")), ("quarter shift", dict(post_process=True)),
                                                  ("centroid r=4", dict(subpixel="centroid", radius=4)), ("plain", dict()))}
    noisy = {name: run(0.004, **kw) for name, kw in (("gaussian", dict(subpixel="gaussian")), ("quarter shift", dict(post_process=True)),
                                                    ("centroid r=4", dict(subpixel="centroid", radius=4, threshold=0.004)))}
    for title, rows in (("clean maps", clean), ("maps + U(0, 0.004)", noisy)):
        for name, (worst, mean, e3d) in rows.items():
            print("%s, %-13s: per-axis error worst %.6f / mean %.6f cells; mean 3D error %.3e world units" % (title, name, worst, mean, e3d))
    assert clean["gaussian"][0] <= 0.01
    assert clean["plain"][0] > 0.25
    assert clean["gaussian"][2] < clean["quarter shift"][2]
    assert noisy["gaussian"][2] < noisy["quarter shift"][2]
