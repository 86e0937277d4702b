"""decode_heatmaps (csrc/heatmaps.hip) on the device: against the numpy restatement of tests/heatmap_cases.py (peak, shift and
confidence bit for bit; pixels within 1 float32 ulp, the margin for a contracted multiply-add), against the reference-generated
golden, against prepare_inputs for the fused outputs, and in a closed loop behind synthesize_views."""
import functools

import numpy as np
import pytest
import torch

from tests import heatmap_cases as hc
from tests import synth_cases as sc

pytestmark = pytest.mark.gpu

# B, V, J, H, W
SHAPES = [(2, 2, 3, 8, 8),        # a map smaller than a wave's one vector load
          (1, 3, 17, 64, 64),     # the standard map; 51 maps, a ragged last workgroup
          (2, 2, 2, 64, 48),      # non-square
          (1, 2, 3, 5, 7),        # element-wise path, unaligned bases
          (1, 1, 2, 128, 128),    # fp32, the four-wave form
          (1, 2, 2, 96, 72)]      # a second non-square size: 27 chunks per lane, every unroll step and the guarded tail
WH = (1000.0, 1000.0)


def _dev(x):
    return None if x is None else torch.from_numpy(np.array(x)).cuda()                  # a copy: the cached cases are read-only


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
def _case(shape, seed=0):
    """the maps, their boxes and the restatement under all four switch settings, computed once and not written to"""
    hm, center, scale = hc.batch(*shape, seed=seed)
    ref = {(post, boxes): hc.decode(hm, center if boxes else None, scale if boxes else None, post)
           for post in (False, True) for boxes in (False, True)}
    for a in (hm, center, scale):
        a.setflags(write=False)
    return hm, center, scale, ref


def _check(r, ref, what):
    coords, conf, pixels = r.coords.cpu().numpy(), r.conf.cpu().numpy(), r.pixels.cpu().numpy()
    assert np.array_equal(coords, ref["coords"], equal_nan=True), what
    assert np.array_equal(conf, ref["maxval"], equal_nan=True), what
    u = hc.ulps(pixels, ref["pixels"])
    print("%s: %d of %d pixel entries differ from the restatement, at most %.1f ulp" % (what, int((u > 0).sum()), u.size, u.max() if u.size else 0))
    assert u.size == 0 or u.max() <= 1.0, what


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("post", [False, True])
@pytest.mark.parametrize("boxes", [False, True])
@pytest.mark.parametrize("as_list", [True, False])
def test_matches_the_restatement_in_one_launch(shape, post, boxes, as_list):
    from openmpl_amd import decode_heatmaps
    hm, center, scale, ref = _case(shape)
    t = _dev(hm)
    arg = [t[:, v].contiguous() for v in range(shape[1])] if as_list else t
    c, s = (_dev(center), _dev(scale)) if boxes else (None, None)
    r, n = _launches(lambda: decode_heatmaps(arg, c, s, post_process=post, return_coords=True))
    assert n == 1
    assert r.poses is None and r.rays is None and r.centers is None
    _check(r, ref[post, boxes], "%s post=%s boxes=%s list=%s" % (shape, post, boxes, as_list))
    if not boxes:
        assert _same_bits(r.pixels, r.coords)
    q = decode_heatmaps(arg, c, s, post_process=post)
    assert q.coords is None and _same_bits(q.pixels, r.pixels) and _same_bits(q.conf, r.conf)


def test_every_special_and_edge_map():
    from openmpl_amd import decode_heatmaps
    for H, W in ((64, 64), (5, 7), (16, 12)):
        hm = np.concatenate([hc.special_maps(H, W), hc.edge_maps(H, W)])[None, None]          # (1,1,32,H,W)
        for post in (False, True):
            _check(decode_heatmaps(_dev(hm), post_process=post, return_coords=True), hc.decode(hm, post_process=post), "%dx%d post=%s" % (H, W, post))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("shape", [(1, 3, 17, 64, 64), (1, 2, 3, 5, 7), (2, 2, 2, 64, 48), (1, 1, 2, 256, 128)], ids=lambda s: "x".join(map(str, s)))
def test_16_bit_maps_equal_their_fp32_upcast(dtype, shape):
    """(1,1,2,256,128): 64 KiB of 16-bit values, the four-wave form; 64x64: eight chunks per lane; 5x7: element-wise"""
    from openmpl_amd import decode_heatmaps
    hm, center, scale, _ = _case(shape)
    low = _dev(hm).to(dtype)
    up = low.float()
    assert not torch.equal(up, _dev(hm))                       # the rounding did something, so this is not the fp32 test again
    a = decode_heatmaps(low, _dev(center), _dev(scale), post_process=True, return_coords=True)
    b = decode_heatmaps(up, _dev(center), _dev(scale), post_process=True, return_coords=True)
    for k in ("pixels", "conf", "coords"):
        assert _same_bits(getattr(a, k), getattr(b, k)), k
    _check(a, hc.decode(up.cpu().numpy(), center, scale, True), "%s %s" % (dtype, shape))


@pytest.mark.parametrize("normalize_inputs,normalize_cameras", [(True, True), (True, False), (False, True), (False, False)])
def test_fused_outputs_are_prepare_inputs_bitwise(normalize_inputs, normalize_cameras):
    from openmpl_amd import decode_heatmaps
    from openmpl_amd.inputs import prepare_inputs
    shape = (2, 3, 5, 64, 64)
    hm, center, scale, _ = _case(shape)
    cams = _dev(sc.scene(2, 3, 5, seed=4)[1])
    kw = dict(normalize_inputs=normalize_inputs, normalize_cameras=normalize_cameras)
    r, n = _launches(lambda: decode_heatmaps(_dev(hm), _dev(center), _dev(scale), post_process=True, cams=cams, image_size=WH, **kw))
    assert n == 1 and r.coords is None
    plain = decode_heatmaps(_dev(hm), _dev(center), _dev(scale), post_process=True)
    assert _same_bits(plain.pixels, r.pixels) and _same_bits(plain.conf, r.conf)
    assert bool(torch.isnan(r.conf).any()) and bool((r.conf > 0).any())              # the NaN maps are part of it
    poses, rays, centers = prepare_inputs(r.pixels, r.conf, cams, WH, **kw)
    assert len(r.poses) == len(r.rays) == len(r.centers) == 3
    for v in range(3):
        assert _same_bits(r.poses[v], poses[v]) and _same_bits(r.rays[v], rays[v]) and _same_bits(r.centers[v], centers[v])
        assert r.poses[v].shape == (2, 5, 3) and r.centers[v].shape == (2, 1, 3)


def test_sub_batches_layouts_and_reruns_bitwise():
    from openmpl_amd import decode_heatmaps
    shape = (3, 2, 5, 64, 48)
    hm, center, scale, _ = _case(shape)
    t, c, s = _dev(hm), _dev(center), _dev(scale)
    cams = _dev(sc.scene(3, 2, 5, seed=4)[1])
    kw = dict(post_process=True, return_coords=True, cams=cams, image_size=WH)
    whole, again = decode_heatmaps(t, c, s, **kw), decode_heatmaps(t, c, s, **kw)
    part = decode_heatmaps(t[1:], c[1:], s[1:], **kw)                              # a view at an offset, read in place
    views = decode_heatmaps(list(t.unbind(1)), c, s, **kw)                        # views with the batch stride of the 5-D tensor
    swapped = decode_heatmaps(t.transpose(0, 1).contiguous().transpose(0, 1), c, s, **kw)     # (V,B,...) memory: view stride > batch stride
    for k in ("pixels", "conf", "coords"):
        assert _same_bits(getattr(whole, k), getattr(again, k)), k
        assert _same_bits(getattr(whole, k)[1:], getattr(part, k)), k
        assert _same_bits(getattr(whole, k), getattr(views, k)), k
        assert _same_bits(getattr(whole, k), getattr(swapped, k)), k
    for k in ("poses", "rays", "centers"):
        for v in range(2):
            assert _same_bits(getattr(whole, k)[v], getattr(again, k)[v]) and _same_bits(getattr(whole, k)[v][1:], getattr(part, k)[v]), k
            assert _same_bits(getattr(whole, k)[v], getattr(views, k)[v]) and _same_bits(getattr(whole, k)[v], getattr(swapped, k)[v]), k


@pytest.mark.parametrize("tag", ["64x64", "64x48"])
@pytest.mark.parametrize("post", [False, True])
def test_reference_golden_straight_through_the_kernel(tag, post):
    """coords and confidences are the reference's own bit for bit; pixels are within the golden's measured 20 ulps of the
    reference (tests/test_heatmaps_cpu.py) plus the kernel's 1"""
    from openmpl_amd import decode_heatmaps
    g = hc.golden()
    hm, center, scale = g[tag + "_hm"], g[tag + "_center"], g[tag + "_scale"]                 # (N,J,H,W), (N,2): one view
    r = decode_heatmaps([_dev(hm)], _dev(center[:, None]), _dev(scale[:, None]), post_process=post, return_coords=True)
    assert np.array_equal(r.coords.cpu().numpy()[:, 0], g[tag + ("_coords_post" if post else "_coords")], equal_nan=True)
    assert np.array_equal(r.conf.cpu().numpy()[:, 0], g[tag + "_maxvals"], equal_nan=True)
    u = hc.ulps(r.pixels.cpu().numpy()[:, 0], g[tag + ("_preds_post" if post else "_preds")])
    print("%s post=%s: at most %.1f ulps from the reference" % (tag, post, u.max()))
    assert u.max() <= 21


def test_closed_loop_behind_synthesize_views():
    """poses -> synthesize_views pixels -> Gaussians rendered at stride k -> decode_heatmaps -> the pixels again.  The bound is
    the estimator's own: the peak is round(m), and the shift moves a quarter cell towards m, so every axis is within 0.25 k of the
    true pixel with post_process and 0.5 k without; 1e-3 px covers the float32 roundings (an ulp of 1000 px is 6e-5)."""
    from openmpl_amd import decode_heatmaps, synthesize_views
    from openmpl_amd import detrng
    B, V, J, H, W = 2, 3, 17, 64, 64
    poses3d, cams = sc.scene(B, V, J, seed=9, focal=600.0)
    true = synthesize_views(_dev(poses3d), _dev(cams), WH, clip=False, return_pixels=True).pixels.cpu().numpy()
    center = (500.0 + detrng.uniform(1, "loop.center", (B, V, 2), -20.0, 20.0)).astype(np.float32)
    scale = detrng.uniform(1, "loop.scale", (B, V, 2), 5.0, 5.5)                  # k = 15.6 .. 17.2 px per cell
    k = (scale[..., 0].astype(np.float64) * 200.0 / W)[:, :, None, None]
    hm, m = hc.render(true, center, scale, H, W)
    interior = ((m >= 3.0) & (m <= np.array([W - 4.0, H - 4.0]))).all(-1)
    assert interior.sum() > 0.7 * interior.size
    for post, bound in ((True, 0.25), (False, 0.5)):
        r = decode_heatmaps(_dev(hm), _dev(center), _dev(scale), post_process=post)
        err = np.abs(r.pixels.cpu().numpy().astype(np.float64) - true)
        print("post_process=%s: worst axis error %.4f cells of %.2f allowed" % (post, (err / k)[interior].max(), bound))
        assert (err <= bound * k + 1e-3)[interior].all()
        assert bool((r.conf.cpu().numpy()[interior] > 0.9).all())
    assert (err > 0.25 * k + 1e-3)[interior].any()                                # without the shift the tighter bound does not hold
