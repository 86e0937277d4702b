"""Heatmap rendering (openmpl_amd.render_heatmaps): the numpy restatement against the reference-generated golden, the rounding and
the noise stream it is made of, the C prototypes of both new entry points against their bindings with every refusal of the C ABI,
and every argument complaint of the Python wrapper.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import openmpl_amd
from openmpl_amd import cabi, detrng
from tests import render_cases as rc

G = rc.golden()
KEYS = [(tag, W, H, s) for tag, W, H in rc.GOLDEN_SIZES for s in rc.GOLDEN_SIGMAS]
GOLDEN_ULPS = {1: 1, 2: 1, 3: 3}        # per sigma, measured on the committed golden, see test_golden_measures_what_it_claims


def _restate(tag, W, H, s, **kw):
    k = "%s_s%d" % (tag, s)
    return k, rc.render(G[k + "_joints"][None, None], G[k + "_vis"][None, None], heatmap_size=(W, H), stride=G["stride"], sigma=float(s), **kw)


@pytest.mark.parametrize("tag,W,H,s", KEYS, ids=lambda v: str(v))
def test_restatement_matches_reference_golden(tag, W, H, s):
    """weights and zero cells are the reference's exactly.  The values are not bitwise: the reference evaluates numpy's float32
    exp, which is not correctly rounded; against float64-then-one-rounding it is off by at most 1 ulp at sigma 1 and 2 and by 3
    ulps at sigma 3 on the committed golden, and that is asserted."""
    k, r = _restate(tag, W, H, s)
    assert np.array_equal(r["weight"][0, 0], G[k + "_weight"])
    assert np.array_equal(r["heatmaps"][0, 0] == 0, G[k + "_target"] == 0)
    u = rc.ulps(r["heatmaps"][0, 0], G[k + "_target"])
    print("%s: %d of %d non-zero values differ from the reference, at most %.0f ulps" % (k, int((u > 0).sum()), int((G[k + "_target"] != 0).sum()), u.max()))
    assert u.max() <= GOLDEN_ULPS[s]


def test_golden_measures_what_it_claims():
    worst = {s: 0 for s in rc.GOLDEN_SIGMAS}
    for tag, W, H, s in KEYS:
        k, r = _restate(tag, W, H, s)
        worst[s] = max(worst[s], rc.ulps(r["heatmaps"][0, 0], G[k + "_target"]).max())
        target, weight, vis, t = G[k + "_target"], G[k + "_weight"], G[k + "_vis"], 3 * s
        full = (2 * t + 1) ** 2
        count = (target != 0).reshape(len(vis), -1).sum(1)
        mu = r["mu"][0, 0]
        assert count[0] == full and (0 < count[1:5]).all() and (count[1:5] < full).all()           # inside; cut by each border
        assert mu[1, 0] - t < 0 and mu[2, 0] + t >= W and mu[3, 1] - t < 0 and mu[4, 1] + t >= H
        assert not weight[5:9].any() and not count[5:9].any()                                        # wholly outside, each side
        assert mu[5, 0] + t + 1 < 0 and mu[6, 0] - t >= W and mu[7, 1] + t + 1 < 0 and mu[8, 1] - t >= H
        assert mu[9, 0] == 0 and mu[10, 1] == -1 and count[9] and count[10]                          # int() truncates towards zero
        assert weight[11] == 1 and count[11] == 0 and mu[11, 0] + t + 1 == 0                         # an empty patch keeps its weight
        assert count[12] == 1 and target[12, H - 1, W - 1] != 0                                      # the patch's corner
        assert vis[13:].tolist() == [0.0, np.float32(0.4), 1.0] and np.array_equal(weight[13:], vis[13:])
        assert count[13] == 0 and count[14] == 0 and count[15] == full                               # written only above one half
    assert worst == GOLDEN_ULPS                                                # the asserted bounds are the measured values, no more
    assert os.path.getsize(os.path.join(rc.GOLD, "render.npz")) < 32 * 1024


def test_the_separable_product_rounds_to_the_joint_form():
    """gx(x) * gy(y) in float64 and exp(-(dx^2 + dy^2) / (2 sigma^2)) in float64 round to the same float32 values on the golden's
    joints: the kernel's separable form loses nothing against the formula of the reference."""
    differ = total = 0
    for tag, W, H, s in KEYS:
        k, r = _restate(tag, W, H, s)
        mu, on = r["mu"][0, 0], r["weight"][0, 0] > 0.5
        x, y = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)[:, None]
        for i in np.nonzero(on)[0]:
            dx, dy = x - mu[i, 0], y - mu[i, 1]
            joint = np.where((np.abs(dx) <= 3 * s) & (np.abs(dy) <= 3 * s), np.exp(-(dx ** 2 + dy ** 2) / (2.0 * s * s)), 0.0)
            differ += int((joint.astype(np.float32) != r["heatmaps"][0, 0, i].astype(np.float32)).sum())
            total += int((joint != 0).sum())
    print("%d of %d values differ between the separable and the joint form" % (differ, total))
    assert differ == 0 and total > 1000


def test_round_once_is_the_formats_rounding():
    x = np.concatenate([detrng.uniform01(1, "round", 4000) * 2.0 ** -detrng.uniform(1, "round.e", (4000,), 0.0, 150.0).astype(np.float64),
                        [0.0, 1.0, 2.0 ** -149, 2.0 ** -150, 3 * 2.0 ** -150, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8]])
    x = np.concatenate([x, -x])
    assert np.array_equal(rc.round_once(x, "fp32"), x.astype(np.float32).astype(np.float64))
    assert np.array_equal(rc.round_once(x, "fp16"), x.astype(np.float16).astype(np.float64))
    f = x.astype(np.float32)                        # float32 -> bfloat16 is one rounding in torch
    assert np.array_equal(rc.round_once(f.astype(np.float64), "bf16"), torch.from_numpy(f).to(torch.bfloat16).double().numpy())
    # a float64 just above a bfloat16 tie that float32 would round onto the tie: one rounding goes up, two would go to even
    tie = 1.0 + 2.0 ** -8 + 2.0 ** -40
    assert rc.round_once(tie, "bf16") == 1.0 + 2.0 ** -7 and float(torch.tensor(np.float32(tie)).to(torch.bfloat16)) == 1.0
    assert rc.ulp_of(1.0, "bf16") == 2.0 ** -7 and rc.ulp_of(0.75, "fp16") == 2.0 ** -11 and rc.ulp_of(0.0, "fp32") == 2.0 ** -149


def test_noise_is_the_detrng_stream_and_survives_batching():
    HW = 35
    whole = rc.noise_draws(3, 0, 12, HW)
    assert np.array_equal(whole.reshape(-1), detrng.uniform01(3, "render.noise", 12 * HW))
    assert np.array_equal(rc.noise_draws(3, 5, 7, HW), whole[5:])
    p, conf = rc.joints(4, 2, 3, 7, 5)
    kw = dict(heatmap_size=(7, 5), mode="subpixel", noise_level=0.01, seed=3)
    a = rc.render(p, conf, **kw)["heatmaps"]
    b = rc.render(p[1:], conf[1:], first_index=1, **kw)["heatmaps"]
    assert np.array_equal(a[1:], b)
    zero = rc.render(p, np.zeros_like(conf), **kw)["heatmaps"]
    assert np.array_equal(zero.reshape(-1).astype(np.float32), detrng.uniform(3, "render.noise", (4 * 2 * 3 * 35,), 0.0, 0.01))


def test_restated_special_joints():
    p, conf = rc.joints(2, 2, 3, 8, 8)
    p.reshape(-1, 2)[:4] = (3.0, 4.0)                                  # the four joints with conf 0, 0.4, 0.5, 1 are inside
    for mode in ("reference", "subpixel"):
        r = rc.render(p, conf, heatmap_size=(8, 8), sigma=1.0, mode=mode)
        w, hm = r["weight"].reshape(-1), r["heatmaps"].reshape(-1, 64)
        assert not w[-3:].any() and not hm[-3:].any()                  # NaN, infinite, beyond 2^30
        assert np.isnan(r["cells"].reshape(-1, 2)[-1, 0]) and np.isinf(r["cells"].reshape(-1, 2)[-2, 1])
        assert w[0] == 0 and not hm[0].any()                           # conf 0
        if mode == "reference":
            assert w[1] == np.float32(0.4) and not hm[1].any() and w[2] == 0.5 and not hm[2].any()
        else:
            assert w[1] == np.float32(0.4) and (hm[1] > 0).all()
    with pytest.raises(AssertionError):
        rc.render(p, conf, heatmap_size=(8, 8), sigma=0.5)


# ------------------------------------------------------------------------------------------------- the C ABI, both symbols
def _declared(name):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mpl_hip.h")).read()
    m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
    assert m, "%s is not declared in include/mpl_hip.h" % name
    return header, [p.strip() for p in m.group(1).replace("\n", " ").split(",")]


def test_symbols_header_and_bindings_agree():
    assert "mpl_render_heatmaps" in cabi.EXPORTS and "mpl_decode_heatmaps_ex" in cabi.EXPORTS and cabi.ABI_VERSION == 14
    lib = cabi.load()
    header, params = _declared("mpl_render_heatmaps")
    assert re.search(r"#define MPL_HIP_ABI_VERSION 14\b", header)
    assert len(params) == 22 and params[0] == "void *const *heatmaps" and params[-1] == "void *stream"
    assert len(lib.mpl_render_heatmaps.argtypes) == len(params) and lib.mpl_render_heatmaps.restype is C.c_int
    _, old = _declared("mpl_decode_heatmaps")
    _, ex = _declared("mpl_decode_heatmaps_ex")
    assert len(old) == 23 and ex == old[:-1] + ["int refine", "int radius", "double threshold", "void *stream"]
    assert len(lib.mpl_decode_heatmaps_ex.argtypes) == 26 and lib.mpl_decode_heatmaps_ex.restype is C.c_int
    assert len(lib.mpl_decode_heatmaps.argtypes) == 23
    codes = dict((n, int(v)) for n, v in re.findall(r"#define MPL_RENDER_([A-Z]+) (\d+)", header))
    assert codes == dict(REFERENCE=cabi.RENDER_MODES["reference"], SUBPIXEL=cabi.RENDER_MODES["subpixel"])
    codes = dict((n, int(v)) for n, v in re.findall(r"#define MPL_REFINE_([A-Z]+) (\d+)", header))
    assert codes == dict(NONE=cabi.REFINE[None], GAUSSIAN=cabi.REFINE["gaussian"], CENTROID=cabi.REFINE["centroid"])
    assert openmpl_amd.render_heatmaps is __import__("openmpl_amd.heatmaps", fromlist=["x"]).render_heatmaps


INVALID, UNSUPPORTED = -1, -2
_tab = lambda *a: (cabi._fp * len(a))(*a)
_p = lambda a: None if a is None else C.c_void_p(a)                     # never dereferenced by a refused call


def test_render_refusals_come_before_any_launch():
    lib = cabi.load()

    def call(hm=_tab(8, 8), dtype=0, stride=3 * 64 * 64, B=2, V=2, J=3, H=64, W=64, pixels=8, conf=None, center=None, scale=None, sx=0.0, sy=0.0,
             mode=0, sigma=2.0, noise=0.0, first=0, weight=8, cells=8):
        return lib.mpl_render_heatmaps(hm, dtype, stride, B, V, J, H, W, _p(pixels), _p(conf), _p(center), _p(scale), sx, sy, mode, sigma, noise,
                                       0, first, _p(weight), _p(cells), None)
    assert call(hm=None) == INVALID and call(hm=_tab(8, None)) == INVALID
    assert call(pixels=None) == INVALID and call(weight=None) == INVALID and call(cells=None) == INVALID
    for k in ("B", "V", "J", "H", "W"):
        assert call(**{k: 0}) == INVALID and call(**{k: -1}) == INVALID
    assert call(center=8) == INVALID and call(scale=8) == INVALID
    assert call(sx=4.0) == INVALID and call(sy=4.0) == INVALID and call(sx=-4.0, sy=4.0) == INVALID and call(sx=float("nan"), sy=4.0) == INVALID
    assert call(center=8, scale=8, sx=4.0, sy=4.0) == INVALID
    assert call(dtype=3) == INVALID and call(dtype=-1) == INVALID
    assert call(mode=2) == INVALID and call(mode=-1) == INVALID
    assert call(sigma=0.0) == INVALID and call(sigma=-1.0) == INVALID and call(sigma=float("nan")) == INVALID
    assert call(sigma=0.5) == INVALID and call(sigma=2.1) == INVALID          # reference mode: 3 sigma is not an integer
    assert call(noise=-0.1) == INVALID and call(noise=float("nan")) == INVALID and call(first=-1) == INVALID
    assert call(stride=3 * 64 * 64 - 1) == INVALID
    assert call(hm=_tab(*([8] * 33)), V=33) == UNSUPPORTED
    assert call(H=1024, W=1025, stride=3 * 1024 * 1025) == UNSUPPORTED
    assert call(B=1 << 20, V=2, J=1 << 9 | 1, stride=(1 << 9 | 1) * 64 * 64) == UNSUPPORTED


def test_decode_ex_refusals_come_before_any_launch():
    lib = cabi.load()

    def call(hm=_tab(8, 8), dtype=0, stride=3 * 64 * 64, B=2, V=2, J=3, H=64, W=64, post=0, pixels=8, conf=8, refine=1, radius=2, threshold=1e-6):
        return lib.mpl_decode_heatmaps_ex(hm, dtype, stride, B, V, J, H, W, post, None, None, _p(pixels), _p(conf), None, None, 1000.0, 1000.0, 1, 1,
                                          None, None, None, refine, radius, threshold, None)
    for refine in (0, 1, 2):
        assert call(hm=None, refine=refine) == INVALID and call(pixels=None, refine=refine) == INVALID and call(conf=None, refine=refine) == INVALID
        assert call(dtype=3, refine=refine) == INVALID and call(B=0, refine=refine) == INVALID and call(W=-1, refine=refine) == INVALID
        assert call(stride=3 * 64 * 64 - 1, refine=refine) == INVALID
        assert call(hm=_tab(*([8] * 33)), V=33, refine=refine) == UNSUPPORTED
        assert call(H=1024, W=1025, stride=3 * 1024 * 1025, refine=refine) == UNSUPPORTED
        assert call(B=1 << 20, V=2, J=1 << 9 | 1, stride=(1 << 9 | 1) * 64 * 64, refine=refine) == UNSUPPORTED
    assert call(refine=3) == INVALID and call(refine=-1) == INVALID
    assert call(refine=1, post=1) == INVALID and call(refine=2, post=1) == INVALID
    for radius in (0, -1, 9, 100):
        assert call(refine=2, radius=radius) == INVALID
    assert call(refine=2, threshold=float("nan")) == INVALID


# ------------------------------------------------------------------------------------------------------------ the wrapper
def test_wrapper_complaints_need_no_gpu():
    """shapes, then values, then dtypes, then devices: on CPU tensors a well-formed call gets as far as the device complaint"""
    r = openmpl_amd.render_heatmaps
    px = lambda: torch.zeros((2, 2, 3, 2))
    box = lambda: torch.zeros((2, 2, 2))
    size = dict(heatmap_size=(8, 8))

    def complains(text, *a, exc=RuntimeError, **kw):
        with pytest.raises(exc, match=text):
            r(*a, **kw)
    complains("pixels: expected a tensor of shape \\(B,V,J,2\\)", torch.zeros((2, 3, 2)), **size)
    complains("pixels: expected a tensor of shape \\(B,V,J,2\\)", torch.zeros((2, 2, 3, 3)), **size)
    complains("pixels: expected a tensor of shape \\(B,V,J,2\\), got ndarray", np.zeros((2, 2, 3, 2)), **size)
    complains("center and scale go together \\(got only center\\)", px(), None, box(), **size)
    complains("center and scale go together \\(got only scale\\)", px(), None, None, box(), **size)
    complains("stride and center / scale exclude each other", px(), None, box(), box(), stride=(4, 4), **size)
    complains("stride takes two values", px(), stride=4.0, **size)
    complains("stride must be positive", px(), stride=(4.0, 0.0), **size)
    complains("heatmap_size \\(W, H\\) is needed without out", px())
    complains("heatmap_size must be positive", px(), heatmap_size=(8, 0))
    complains("heatmap_size takes two values", px(), heatmap_size=8)
    complains("expected one \\(B,V,J,H,W\\) tensor", px(), out=torch.zeros((2, 3, 8, 8)))
    complains("out holds \\(B,V,J\\) = \\(2, 2, 4\\), pixels \\(2, 2, 3\\)", px(), out=torch.zeros((2, 2, 4, 8, 8)))
    complains("heatmaps\\[1\\]: expected shape \\(2, 3, 8, 8\\)", px(), out=[torch.zeros((2, 3, 8, 8)), torch.zeros((2, 3, 8, 7))])
    complains("but out holds maps of 8 rows and 6 columns", px(), out=torch.zeros((2, 2, 3, 8, 6)), heatmap_size=(8, 6))
    complains("conf: expected a tensor of shape \\(2, 2, 3\\)", px(), torch.zeros((2, 2)), **size)
    complains("center: expected a tensor of shape \\(2, 2, 2\\)", px(), None, torch.zeros((2, 2)), box(), **size)
    complains("scale: expected a tensor of shape \\(2, 2, 2\\)", px(), None, box(), torch.zeros((2, 2, 3)), **size)
    complains("mode must be one of reference, subpixel", px(), mode="gaussian", **size)
    complains("sigma must be positive", px(), sigma=0.0, **size)
    complains("needs an integer 3 \\* sigma", px(), sigma=0.5, **size)
    complains("needs an integer 3 \\* sigma", px(), sigma=2.1, mode="reference", **size)
    complains("noise_level must not be negative", px(), noise_level=-1.0, **size)
    complains("noise_level must not be negative", px(), noise_level=float("nan"), **size)
    complains("first_index must not be negative", px(), first_index=-1, **size)
    complains("at most 32 views", torch.zeros((1, 33, 1, 2)), exc=NotImplementedError, **size)
    complains("2\\^20 values per map", torch.zeros((1, 1, 1, 2)), heatmap_size=(1025, 1024), exc=NotImplementedError)
    # dtypes
    complains("out must be float32, float16 or bfloat16, all alike", px(), out=torch.zeros((2, 2, 3, 8, 8), dtype=torch.float64))
    complains("all alike", px(), out=[torch.zeros((2, 3, 8, 8)), torch.zeros((2, 3, 8, 8), dtype=torch.float16)])
    complains("dtype is torch.float16, out is torch.float32", px(), out=torch.zeros((2, 2, 3, 8, 8)), dtype=torch.float16)
    complains("dtype must be float32, float16 or bfloat16", px(), dtype=torch.float64, **size)
    complains("pixels must be torch.float32", px().double(), **size)
    complains("conf must be torch.float32", px(), torch.zeros((2, 2, 3), dtype=torch.float64), **size)
    complains("scale must be torch.float32", px(), None, box(), box().half(), **size)
    # devices: the last complaint left
    for dtype in (None, torch.float32, torch.float16, torch.bfloat16):
        complains("no CPU path: pixels must live on a GPU", px(), torch.ones((2, 2, 3)), box(), box(), dtype=dtype, sigma=1.0, mode="subpixel", **size)
    complains("no CPU path: pixels must live on a GPU", px(), out=[torch.zeros((2, 3, 8, 8))] * 2, sigma=0.5, mode="subpixel", noise_level=0.1)
    with pytest.raises(TypeError):
        r(px(), None, None, None, (8, 8))                              # heatmap_size and what follows are keyword-only


def test_decode_wrapper_complaints_about_subpixel_need_no_gpu():
    d = openmpl_amd.decode_heatmaps
    maps = [torch.zeros((2, 3, 8, 8)) for _ in range(2)]

    def complains(text, **kw):
        with pytest.raises(RuntimeError, match=text):
            d(maps, **kw)
    complains("subpixel must be None, 'gaussian' or 'centroid'", subpixel="soft")
    complains("subpixel must be None", subpixel=True)
    complains("post_process and subpixel exclude each other", subpixel="gaussian", post_process=True)
    complains("post_process and subpixel exclude each other", subpixel="centroid", post_process=True)
    for radius in (0, 9, 2.0, True, None):
        complains("radius must be an integer from 1 to 8", subpixel="centroid", radius=radius)
    complains("threshold must be a number", subpixel="centroid", threshold=float("nan"))
    for kw in (dict(subpixel="gaussian"), dict(subpixel="centroid", radius=8, threshold=0.0), dict(subpixel=None, radius=0)):
        complains("no CPU path: heatmaps\\[0\\] must live on a GPU", **kw)       # well formed: only the device is left
