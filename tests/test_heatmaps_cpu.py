"""Heatmap decoding (openmpl_amd/heatmaps.py): the numpy restatement against the reference-generated golden, the C prototype against
its binding with every refusal of the C ABI, and every argument complaint of the Python wrapper.  No GPU."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import openmpl_amd
from openmpl_amd import cabi
from tests import heatmap_cases as hc

G = hc.golden()
TAGS = ("64x64", "64x48")
GOLDEN_ULPS = 20        # measured on the committed golden, see test_restatement_matches_reference_golden


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("post", [False, True])
def test_restatement_matches_reference_golden(tag, post):
    """coords and maxval are the reference's bit for bit.  pixels: the largest difference measured on the committed golden is
    20 float32 ulps (64x48, both POST_PROCESS values; 3 ulps on 64x64), and that is asserted.  It is the reference's error, not the
    closed form's: the value is x = -25.1876 px, the difference of 201.8 and 227.0, and the reference's float32-rounded anchor
    points (one of them near 774) are off by 3.8e-5 px there -- 2.5 ulps of the operands, 20 of the cancelled result.  The closed
    form is within half an ulp of exact rational arithmetic everywhere (test_closed_form_is_correctly_rounded)."""
    r = hc.decode(G[tag + "_hm"], G[tag + "_center"], G[tag + "_scale"], post)
    assert np.array_equal(r["coords"], G[tag + ("_coords_post" if post else "_coords")], equal_nan=True)
    assert np.array_equal(r["maxval"], G[tag + "_maxvals"], equal_nan=True)
    assert np.array_equal(np.isnan(r["maxval"]), np.isnan(G[tag + "_maxvals"]))
    u = hc.ulps(r["pixels"], G[tag + ("_preds_post" if post else "_preds")])
    print("%s post=%s: pixels differ in %d of %d entries, at most %.1f ulps" % (tag, post, int((u > 0).sum()), u.size, u.max()))
    assert u.max() <= GOLDEN_ULPS


def test_golden_measures_what_it_claims():
    worst = max(hc.ulps(hc.decode(G[t + "_hm"], G[t + "_center"], G[t + "_scale"], p)["pixels"], G[t + ("_preds_post" if p else "_preds")]).max()
                for t in TAGS for p in (False, True))
    assert worst == GOLDEN_ULPS                                        # the asserted bound is the measured value, no more
    for t in TAGS:
        shifted = (G[t + "_coords_post"] != G[t + "_coords"]).any(-1)
        assert shifted.sum() >= 8 and (~shifted).sum() >= 8            # both sides of the shift condition
        assert np.isnan(G[t + "_maxvals"]).sum() == 2 and (G[t + "_maxvals"] <= 0).sum() >= 3
    assert os.path.getsize(os.path.join(hc.GOLD, "heatmaps.npz")) < 603 * 1000


@pytest.mark.parametrize("tag", TAGS)
def test_closed_form_is_correctly_rounded(tag):
    """center + (coord - half) * scale_x * 200 / W in rational arithmetic on the float32 inputs; float64 then one rounding to float32
    is within half an ulp of it (plus the 2^-29 of the double rounding)."""
    hm, center, scale = G[tag + "_hm"], G[tag + "_center"], G[tag + "_scale"]
    H, W = hm.shape[-2:]
    r = hc.decode(hm, center, scale, True)
    worst = 0.0
    for n, j, a in np.ndindex(r["pixels"].shape):
        if np.isnan(r["coords"][n, j, a]):
            continue
        exact = Fraction(float(center[n, a])) + (Fraction(float(r["coords"][n, j, a])) - Fraction((W, H)[a], 2)) * Fraction(float(scale[n, 0])) * 200 / W
        got = r["pixels"][n, j, a]
        worst = max(worst, float(abs(Fraction(float(got)) - exact) / Fraction(float(np.spacing(np.abs(got))))))
    assert worst <= 0.5 + 2.0 ** -20


def test_special_and_edge_maps_are_what_they_say():
    for H, W in ((64, 64), (5, 7)):
        s = dict(zip(hc.SPECIAL, hc.special_maps(H, W)))
        r = {k: hc.decode(v[None], post_process=True) for k, v in s.items()}
        assert r["two_maxima"]["idx"][0] == (H // 2) * W + W // 2 and r["two_maxima"]["maxval"][0] == 2.0
        for k in ("all_zero", "all_negative", "signed_zeros", "nan", "nan_neighbour", "all_neg_inf"):
            assert not r[k]["coords"].any(), k
        assert r["all_zero"]["idx"][0] == 0 and r["signed_zeros"]["idx"][0] == 0 and r["all_neg_inf"]["idx"][0] == 0
        assert r["all_negative"]["maxval"][0] < 0 and r["all_neg_inf"]["maxval"][0] == -np.inf
        assert r["nan"]["idx"][0] == (H // 2 - 1) * W + 1 and np.isnan(r["nan"]["maxval"][0]) and np.isnan(r["nan_neighbour"]["maxval"][0])
        e = hc.decode(hc.edge_maps(H, W), post_process=True)
        plain = hc.decode(hc.edge_maps(H, W))["coords"]
        xs, ys = np.meshgrid(hc.EDGE(W), hc.EDGE(H))
        assert np.array_equal(plain, np.stack([xs.reshape(-1), ys.reshape(-1)], -1).astype(np.float32))
        inside = (1 < plain[:, 0]) & (plain[:, 0] < W - 1) & (1 < plain[:, 1]) & (plain[:, 1] < H - 1)
        assert inside.any() and not inside.all()
        assert np.array_equal(e["coords"][inside] - plain[inside], np.tile(np.float32([0.25, -0.25]), (inside.sum(), 1)))
        assert np.array_equal(e["coords"][~inside], plain[~inside])


def test_symbol_header_and_binding_agree():
    assert "mpl_decode_heatmaps" in cabi.EXPORTS and cabi.ABI_VERSION == 14
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mpl_hip.h")).read()
    assert re.search(r"#define MPL_HIP_ABI_VERSION 14\b", header)
    m = re.search(r"\bint mpl_decode_heatmaps\(([^;]*)\);", header)
    assert m, "mpl_decode_heatmaps is not declared in include/mpl_hip.h"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert len(params) == 23 and params[0] == "const void *const *heatmaps" and params[-1] == "void *stream"
    lib = cabi.load()
    assert len(lib.mpl_decode_heatmaps.argtypes) == len(params) and lib.mpl_decode_heatmaps.restype is C.c_int
    codes = dict((n, int(v)) for n, v in re.findall(r"#define MPL_HM_([A-Z0-9]+) (\d+)", header))
    assert codes == dict(F32=cabi.HM_F32, F16=cabi.HM_F16, BF16=cabi.HM_BF16)
    assert openmpl_amd.decode_heatmaps is __import__("openmpl_amd.heatmaps", fromlist=["x"]).decode_heatmaps


def test_c_abi_refusals_come_before_any_launch():
    lib = cabi.load()
    tab = lambda *a: (cabi._fp * len(a))(*a)
    p = lambda a: None if a is None else C.c_void_p(a)                  # never dereferenced by a refused call

    def call(hm=tab(8, 8), dtype=0, stride=3 * 64 * 64, B=2, V=2, J=3, H=64, W=64, center=None, scale=None, pixels=8, conf=8, cams=None,
             w=1000.0, h=1000.0, views=(None, None, None)):
        return lib.mpl_decode_heatmaps(hm, dtype, stride, B, V, J, H, W, 1, p(center), p(scale), p(pixels), p(conf), None, p(cams), w, h, 1, 1,
                                       views[0], views[1], views[2], None)
    INVALID, UNSUPPORTED = -1, -2
    assert call(hm=None) == INVALID and call(hm=tab(8, None)) == INVALID
    assert call(pixels=None) == INVALID and call(conf=None) == INVALID
    for k in ("B", "V", "J", "H", "W"):
        assert call(**{k: 0}) == INVALID and call(**{k: -1}) == INVALID
    assert call(center=8) == INVALID and call(scale=8) == INVALID
    t = tab(8, 8)
    assert call(cams=8) == INVALID and call(cams=8, views=(t, t, None)) == INVALID and call(cams=8, views=(None, t, t)) == INVALID
    assert call(cams=8, views=(t, tab(8, None), t)) == INVALID and call(cams=8, views=(t, t, t), w=0.0) == INVALID
    assert call(dtype=3) == INVALID and call(dtype=-1) == INVALID
    assert call(stride=3 * 64 * 64 - 1) == INVALID
    assert call(hm=tab(*([8] * 33)), V=33) == UNSUPPORTED
    assert call(H=1024, W=1025, stride=3 * 1024 * 1025) == UNSUPPORTED
    assert call(B=1 << 20, V=2, J=1 << 9 | 1, stride=(1 << 9 | 1) * 64 * 64) == UNSUPPORTED


def _maps(B=2, V=2, J=3, H=8, W=8, dtype=torch.float32):
    return [torch.zeros((B, J, H, W), dtype=dtype) for _ in range(V)]


def test_wrapper_complaints_need_no_gpu():
    """shapes, then dtypes, then devices: on CPU tensors a well-formed call gets as far as the device complaint.  The complaints
    about the heatmaps' structure and dtype are one rule for both entry points: openmpl_amd.rpsm, given the same heatmaps and
    otherwise valid CPU arguments, raises the same text as a ValueError."""
    d = openmpl_amd.decode_heatmaps
    box = lambda: torch.zeros((2, 2, 2))
    cams = torch.zeros((2, 16), dtype=torch.float64)

    def rpsm_too(text, heatmaps, B, V, J):
        with pytest.raises(ValueError, match=text):
            openmpl_amd.rpsm(heatmaps, torch.zeros((B, V, 2)), torch.ones((B, V, 2)), torch.zeros((V, 16), dtype=torch.float64), (256.0, 256.0),
                             torch.zeros((B, 3)), torch.ones(J), parents=[-1] + [0] * (J - 1))

    def complains(text, *a, exc=RuntimeError, both=None, **kw):
        with pytest.raises(exc, match=text):
            d(*a, **kw)
        if both:
            rpsm_too(text, *a, *both)
    # shapes
    complains("one \\(B,V,J,H,W\\) tensor or a non-empty list", [], both=(2, 2, 3))
    complains("one \\(B,V,J,H,W\\) tensor or a non-empty list", [np.zeros((2, 3, 8, 8))], both=(2, 2, 3))
    complains("one \\(B,V,J,H,W\\) tensor or a non-empty list", None, both=(2, 2, 3))
    complains("expected one \\(B,V,J,H,W\\) tensor", torch.zeros((2, 3, 8, 8)), both=(2, 2, 3))
    complains("expected one \\(B,V,J,H,W\\) tensor", torch.zeros((2, 2, 3, 0, 8)), both=(2, 2, 3))
    complains("heatmaps\\[0\\]: expected shape \\(B,J,H,W\\)", [torch.zeros((2, 2, 3, 8, 8))], both=(2, 2, 3))
    complains("heatmaps\\[1\\]: expected shape \\(2, 3, 8, 8\\), got \\(2, 3, 8, 7\\)", [_maps()[0], torch.zeros((2, 3, 8, 7))], both=(2, 2, 3))
    complains("center and scale go together \\(got only center\\)", _maps(), box())
    complains("center and scale go together \\(got only scale\\)", _maps(), None, box())
    complains("center: expected a tensor of shape \\(2, 2, 2\\)", _maps(), torch.zeros((2, 2)), box())
    complains("scale: expected a tensor of shape \\(2, 2, 2\\)", _maps(), box(), torch.zeros((2, 2, 3)))
    complains("cams: expected a tensor of shape \\(2, 16\\)", _maps(), cams=torch.zeros((3, 16), dtype=torch.float64), image_size=(1000, 1000))
    complains("cams needs image_size", _maps(), cams=cams)
    complains("image_size must be positive", _maps(), cams=cams, image_size=(1000, 0))
    complains("at most 32 views", [torch.zeros((1, 1, 2, 2))] * 33, exc=NotImplementedError)
    complains("2\\^20 values per map", torch.zeros((1, 1, 1, 1024, 1025), dtype=torch.bfloat16), exc=NotImplementedError)
    # dtypes: a shape complaint comes first
    complains("heatmaps\\[1\\]: expected shape", [_maps()[0], torch.zeros((2, 3, 8, 7), dtype=torch.float64)], both=(2, 2, 3))
    complains("float32, float16 or bfloat16, all alike \\(heatmaps\\[0\\] is torch.float64\\)", _maps(dtype=torch.float64), both=(2, 2, 3))
    complains("all alike \\(heatmaps\\[1\\] is torch.float16\\)", [_maps()[0], _maps(dtype=torch.float16)[0]], both=(2, 2, 3))
    complains("all alike \\(heatmaps is torch.int32\\)", torch.zeros((1, 1, 1, 2, 2), dtype=torch.int32), both=(1, 1, 1))
    complains("center must be torch.float32", _maps(), box().double(), box())
    complains("scale must be torch.float32", _maps(), box(), box().half())
    complains("cams must be torch.float64 .*pack_cameras", _maps(), cams=cams.float(), image_size=(1000, 1000))
    # devices: every dtype is in order, so this is the last complaint left
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        complains("no CPU path: heatmaps\\[0\\] must live on a GPU", _maps(dtype=dtype), box(), box(), cams=cams, image_size=(1000, 1000))
    complains("no CPU path: heatmaps must live on a GPU", torch.zeros((2, 2, 3, 8, 8)), post_process=True, return_coords=True)
    with pytest.raises(TypeError):
        d(_maps(), box(), box(), True)                                 # post_process and what follows are keyword-only
