"""render_heatmaps (csrc/heatmap_render.hip) on the device: against the float64 restatement of tests/render_cases.py (weights, cells
and zero cells bit for bit, values within 1 ulp of the dtype: both sides round a float64 value that is good to a few float64 ulps),
against the reference-generated golden, across output layouts and store paths, with its noise stream, and back through
decode_heatmaps."""
import functools

import numpy as np
import pytest
import torch

from tests import render_cases as rc

pytestmark = pytest.mark.gpu

# B, V, J, H, W
SHAPES = [(2, 2, 3, 8, 8),        # a map smaller than one wave's vector stores
          (1, 3, 17, 64, 64),     # the standard map: every lane keeps its columns; 51 maps, a ragged last workgroup
          (2, 2, 2, 64, 48),      # non-square: a round of chunks is not a whole number of rows
          (1, 2, 3, 5, 7),        # element-wise path, unaligned bases
          (1, 1, 2, 128, 128),    # larger than 64 x 64: the factors are evaluated per cell
          (1, 2, 2, 96, 72)]      # the same, non-square
FMT = {torch.float32: "fp32", torch.float16: "fp16", torch.bfloat16: "bf16"}
IDS = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)


def _dev(x):
    return None if x is None else torch.from_numpy(np.array(x)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


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
def _inputs(shape, boxes):
    """joints in and around the map, as cells or (boxes) as the image pixels of those cells; computed once, read-only"""
    B, V, J, H, W = shape
    cells, conf = rc.joints(B, V, J, W, H)
    center = scale = None
    pixels = cells
    if boxes:
        center, scale = rc.boxes(B, V)
        k = scale[..., 0].astype(np.float64) * 200.0 / W
        with np.errstate(invalid="ignore"):
            pixels = (center.astype(np.float64)[:, :, None] + (cells.astype(np.float64) - np.array([W * 0.5, H * 0.5])) * k[:, :, None, None]).astype(np.float32)
    for a in (pixels, conf, center, scale):
        if a is not None:
            a.setflags(write=False)
    return pixels, conf, center, scale


@functools.lru_cache(maxsize=None)
def _ref(shape, mode, boxes, fmt="fp32", sigma=2.0):
    pixels, conf, center, scale = _inputs(shape, boxes)
    return rc.render(pixels, conf, center, scale, heatmap_size=(shape[4], shape[3]), sigma=sigma, mode=mode, fmt=fmt)


def _check(r, ref, fmt, mode, what):
    got = r.heatmaps.float().cpu().numpy().astype(np.float64)
    assert np.array_equal(r.weight.cpu().numpy(), ref["weight"], equal_nan=True), what
    assert np.array_equal(r.cells.cpu().numpy(), ref["cells"], equal_nan=True), what
    off = ~(ref["weight"] > (0.5 if mode == "reference" else 0.0))
    assert not got[off].any(), what                                                 # a map that is off is exactly zero
    if mode == "reference":
        assert np.array_equal(got == 0, ref["heatmaps"] == 0), what                 # and so is every cell outside the patch
    u = rc.ulps(got, ref["heatmaps"], fmt)
    print("%s: %d of %d values differ from the restatement, at most %.1f ulp" % (what, int((u > 0).sum()), u.size, u.max()))
    assert u.max() <= 1.0, what


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("mode", ["reference", "subpixel"])
@pytest.mark.parametrize("boxes", [False, True])
def test_matches_the_restatement_in_one_launch(shape, mode, boxes):
    from openmpl_amd import render_heatmaps
    pixels, conf, center, scale = _inputs(shape, boxes)
    r, n = _launches(lambda: render_heatmaps(_dev(pixels), _dev(conf), _dev(center), _dev(scale), heatmap_size=(shape[4], shape[3]), mode=mode))
    assert n == 1
    assert r.heatmaps.shape == shape and r.heatmaps.dtype == torch.float32 and r.weight.shape == shape[:3] and r.cells.shape == shape[:3] + (2,)
    ref = _ref(shape, mode, boxes)
    assert (ref["weight"] > 0.5).any() and (ref["weight"].size < 12 or (ref["weight"] == 0).any())
    _check(r, ref, "fp32", mode, "%s %s boxes=%s" % (shape, mode, boxes))


@pytest.mark.parametrize("shape", [(1, 3, 17, 64, 64), (1, 2, 3, 5, 7), (2, 2, 2, 64, 48), (1, 2, 2, 96, 72)], ids=IDS)
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("mode", ["reference", "subpixel"])
def test_16_bit_maps_are_rounded_once(shape, dtype, mode):
    """against the restatement in that format, and against the float32 output: rounding that a second time is within 1 ulp of the
    16-bit type of rounding the float64 value once"""
    from openmpl_amd import render_heatmaps
    pixels, conf, center, scale = _inputs(shape, True)
    args = (_dev(pixels), _dev(conf), _dev(center), _dev(scale))
    kw = dict(heatmap_size=(shape[4], shape[3]), mode=mode)
    r, n = _launches(lambda: render_heatmaps(*args, dtype=dtype, **kw))
    assert n == 1 and r.heatmaps.dtype == dtype
    _check(r, _ref(shape, mode, True, FMT[dtype]), FMT[dtype], mode, "%s %s %s" % (shape, mode, FMT[dtype]))
    full = render_heatmaps(*args, **kw)
    assert _same_bits(full.weight, r.weight) and _same_bits(full.cells, r.cells)
    twice = full.heatmaps.to(dtype).float().cpu().numpy()
    u = rc.ulps(r.heatmaps.float().cpu().numpy(), twice, FMT[dtype])
    print("%d of %d values differ from the twice-rounded float32 output" % (int((u > 0).sum()), u.size))
    assert u.max() <= 1.0


# maps narrower than one 16-byte chunk (W < 4 at fp32, W < 8 at 16 bits) whose byte size is still a multiple of 16: they take the
# vector stores, and a chunk spans several rows; and widths that are no multiple of the chunk, where it straddles two
NARROW = [((1, 2, 3, 8, 2), torch.float32), ((1, 2, 3, 64, 2), torch.float32), ((1, 2, 3, 16, 1), torch.float32), ((1, 2, 3, 8, 6), torch.float32),
          ((1, 2, 3, 8, 4), torch.bfloat16), ((1, 2, 3, 64, 4), torch.bfloat16), ((1, 2, 3, 16, 1), torch.float16), ((1, 2, 3, 8, 2), torch.float16),
          ((1, 2, 3, 4, 12), torch.bfloat16), ((1, 2, 3, 2, 128), torch.float32)]


@pytest.mark.parametrize("shape,dtype", NARROW, ids=lambda v: IDS(v) if isinstance(v, tuple) else FMT[v])
@pytest.mark.parametrize("mode", ["reference", "subpixel"])
def test_narrow_maps_on_the_vector_store_path(shape, dtype, mode):
    """against the restatement, and bitwise against the same call into an unaligned buffer, which takes the element-wise stores"""
    from openmpl_amd import render_heatmaps
    B, V, J, H, W = shape
    assert (H * W * (4 if dtype == torch.float32 else 2)) % 16 == 0
    cells = np.stack([rc.detrng.uniform(4, "narrow.x.%d.%d" % (H, W), (B, V, J), -0.4, W - 0.6),
                      rc.detrng.uniform(4, "narrow.y.%d.%d" % (H, W), (B, V, J), 0.0, H - 1.0)], -1)
    conf = rc.detrng.uniform(4, "narrow.c.%d.%d" % (H, W), (B, V, J), 0.6, 1.2)
    kw = dict(heatmap_size=(W, H), sigma=1.0, mode=mode)
    ref = rc.render(cells, conf, fmt=FMT[dtype], **kw)
    assert (ref["weight"] > 0.5).all()
    r, n = _launches(lambda: render_heatmaps(_dev(cells), _dev(conf), dtype=dtype, **kw))
    assert n == 1 and r.heatmaps.data_ptr() % 16 == 0
    _check(r, ref, FMT[dtype], mode, "%s %s %s" % (shape, FMT[dtype], mode))
    odd = torch.empty(B * V * J * H * W + 1, dtype=dtype, device="cuda")[1:].view(shape)
    assert odd.data_ptr() % 16 != 0
    render_heatmaps(_dev(cells), _dev(conf), out=odd, **kw)
    assert _same_bits(odd.contiguous(), r.heatmaps)


@pytest.mark.parametrize("sigma", [1.0, 3.0, 1.0 / 3.0])
def test_other_sigmas(sigma):
    from openmpl_amd import render_heatmaps
    shape = (2, 2, 2, 64, 48)
    pixels, conf, _, _ = _inputs(shape, False)
    for mode in ("reference", "subpixel"):
        r = render_heatmaps(_dev(pixels), _dev(conf), heatmap_size=(48, 64), sigma=sigma, mode=mode)
        _check(r, _ref(shape, mode, False, "fp32", sigma), "fp32", mode, "sigma %g %s" % (sigma, mode))


@pytest.mark.parametrize("tag,W,H", rc.GOLDEN_SIZES, ids=lambda v: str(v))
@pytest.mark.parametrize("sigma", rc.GOLDEN_SIGMAS)
def test_reference_golden_straight_through_the_kernel(tag, W, H, sigma):
    """the joints of generate_heatmap's golden at its feat_stride: weights and zero cells are the reference's own; values within the
    golden's measured ulps of the reference (tests/test_render_cpu.py) plus the kernel's 1"""
    from openmpl_amd import render_heatmaps
    from tests.test_render_cpu import GOLDEN_ULPS
    g = rc.golden()
    k = "%s_s%d" % (tag, sigma)
    r = render_heatmaps(_dev(g[k + "_joints"][None, None]), _dev(g[k + "_vis"][None, None]), heatmap_size=(W, H), stride=tuple(g["stride"]),
                        sigma=float(sigma))
    got = r.heatmaps.cpu().numpy()[0, 0]
    assert np.array_equal(r.weight.cpu().numpy()[0, 0], g[k + "_weight"])
    assert np.array_equal(got == 0, g[k + "_target"] == 0)
    u = rc.ulps(got, g[k + "_target"])
    print("%s: at most %.0f ulps from the reference" % (k, u.max()))
    assert u.max() <= GOLDEN_ULPS[sigma] + 1


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("noise", [0.0, 0.01])
def test_out_layouts_store_paths_and_reruns_bitwise(dtype, noise):
    from openmpl_amd import render_heatmaps
    shape = B, V, J, H, W = (3, 2, 5, 64, 48)
    pixels, conf, center, scale = _inputs(shape, True)
    args = (_dev(pixels), _dev(conf), _dev(center), _dev(scale))
    kw = dict(mode="subpixel", noise_level=noise, seed=5)
    whole = render_heatmaps(*args, heatmap_size=(W, H), dtype=dtype, **kw)
    again = render_heatmaps(*args, heatmap_size=(W, H), dtype=dtype, **kw)
    assert whole.heatmaps.is_contiguous() and _same_bits(whole.heatmaps, again.heatmaps)
    new = lambda *s: torch.full(s, 7.0, dtype=dtype, device="cuda")
    outs = {"list": [new(B, J, H, W) for _ in range(V)],
            "5-D": new(B, V, J, H, W),
            "offset view": new(B + 1, V, J, H, W)[1:],
            "(V,B,...) memory": new(V, B, J, H, W).transpose(0, 1),
            "unaligned base: element-wise stores": new(B * V * J * H * W + 1)[1:].view(B, V, J, H, W)}
    assert outs["unaligned base: element-wise stores"].data_ptr() % 16 != 0 and whole.heatmaps.data_ptr() % 16 == 0
    for what, out in outs.items():
        r, n = _launches(lambda: render_heatmaps(*args, out=out, **kw))
        assert n == 1 and r.heatmaps is out, what
        got = torch.stack(list(out), 1) if isinstance(out, list) else out
        assert _same_bits(got.contiguous(), whole.heatmaps), what
        assert _same_bits(r.weight, whole.weight) and _same_bits(r.cells, whole.cells), what
    big = new(B + 1, V, J, H, W)
    render_heatmaps(*args, out=big[1:], **kw)
    assert bool((big[0] == 7.0).all())                                  # nothing is written in front of the view
    with pytest.raises(RuntimeError, match="written where it lies"):
        render_heatmaps(*args, out=new(B, V, J, H, W + 1)[..., :W], **kw)


def test_noise_is_the_detrng_stream_and_a_cut_batch_is_the_whole():
    from openmpl_amd import detrng, render_heatmaps
    shape = B, V, J, H, W = (4, 2, 3, 8, 12)
    pixels, conf, _, _ = _inputs(shape, False)
    p, c = _dev(pixels), _dev(conf)
    for mode in ("reference", "subpixel"):
        kw = dict(heatmap_size=(W, H), mode=mode, noise_level=0.004, seed=9, sigma=1.0)
        whole = render_heatmaps(p, c, **kw)
        head, tail = render_heatmaps(p[:1], c[:1], **kw), render_heatmaps(p[1:], c[1:], first_index=1, **kw)
        assert _same_bits(torch.cat([head.heatmaps, tail.heatmaps]), whole.heatmaps)
        assert not _same_bits(render_heatmaps(p[1:], c[1:], **kw).heatmaps, whole.heatmaps[1:])
        ref = rc.render(pixels, conf, heatmap_size=(W, H), mode=mode, noise_level=0.004, seed=9, sigma=1.0)
        u = rc.ulps(whole.heatmaps.cpu().numpy(), ref["heatmaps"])
        assert u.max() <= 1.0
        shifted = rc.render(pixels, conf, heatmap_size=(W, H), mode=mode, noise_level=0.004, seed=9, sigma=1.0, first_index=3)
        r3 = render_heatmaps(p, c, first_index=3, **kw)
        assert rc.ulps(r3.heatmaps.cpu().numpy(), shifted["heatmaps"]).max() <= 1.0
    # on zero maps the values are the host's detrng.uniform bit for bit, and at 16 bits the one rounding of the same float64
    # product 0.02 * u: a single correctly rounded multiply on both sides, so equality and no tolerance
    zero = render_heatmaps(p, torch.zeros_like(c), heatmap_size=(W, H), mode="subpixel", noise_level=0.02, seed=9)
    host = detrng.uniform(9, "render.noise", (B, V, J, H, W), 0.0, 0.02)
    assert not zero.weight.any() and np.array_equal(zero.heatmaps.cpu().numpy(), host)
    exact = 0.02 * rc.noise_draws(9, 0, B * V * J, H * W).reshape(B, V, J, H, W)
    assert np.array_equal(exact.astype(np.float32), host)
    for dtype in (torch.float16, torch.bfloat16):
        low = render_heatmaps(p, torch.zeros_like(c), heatmap_size=(W, H), mode="subpixel", noise_level=0.02, seed=9, dtype=dtype)
        assert np.array_equal(low.heatmaps.float().cpu().numpy().astype(np.float64), rc.round_once(exact, FMT[dtype])), dtype
    assert not np.array_equal(render_heatmaps(p, torch.zeros_like(c), heatmap_size=(W, H), mode="subpixel", noise_level=0.02, seed=10).heatmaps.cpu().numpy(), host)
    none = render_heatmaps(p, torch.zeros_like(c), heatmap_size=(W, H), mode="subpixel", seed=9)
    assert not none.heatmaps.any()                                      # noise_level == 0 draws nothing


@pytest.mark.parametrize("shape", [(1, 3, 17, 64, 64), (3, 2, 5, 64, 48), (2, 2, 3, 128, 128)], ids=IDS)
def test_reference_mode_closes_the_loop_the_coarse_way(shape):
    """decode_heatmaps without the shift returns mu exactly wherever the patch was written and holds its centre; a map that was
    not written decodes to (0, 0) with confidence 0"""
    from openmpl_amd import decode_heatmaps, render_heatmaps
    pixels, conf, center, scale = _inputs(shape, True)
    r = render_heatmaps(_dev(pixels), _dev(conf), _dev(center), _dev(scale), heatmap_size=(shape[4], shape[3]))
    d = decode_heatmaps(r.heatmaps, return_coords=True)
    ref = _ref(shape, "reference", True)
    mu, on = ref["mu"], ref["weight"] > 0.5
    held = on & (mu >= 0).all(-1) & (mu[..., 0] < shape[4]) & (mu[..., 1] < shape[3])
    assert held.sum() >= 3 and (~on).sum() >= 3                         # the case has both kinds
    coords, peak = d.coords.cpu().numpy(), d.conf.cpu().numpy()
    assert np.array_equal(coords[held], mu[held].astype(np.float32)) and (peak[held] == 1.0).all()
    assert not coords[~on].any() and not peak[~on].any()
