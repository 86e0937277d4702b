"""Restatement of openmpl_amd.render_heatmaps (csrc/heatmap_render.hip) and of the sub-pixel refinements of decode_heatmaps
(csrc/heatmaps.hip) in numpy, with the cases of their tests (TEST INFRASTRUCTURE ONLY).

render() forms every value in float64 and rounds it once; its reference mode is pinned by tests/golden/render.npz, which the
reference's own generate_heatmap produced (tests/golden/make_golden_render.py).  refine() / decode() sit next to
heatmap_cases.decode, which they call for the integer peak; the reference has no usable oracle for them (its
find_tensor_peak_batch misses its own intent, see tests/golden/make_golden_subpixel.py), so they are pinned by their properties
(tests/test_subpixel_cpu.py).
"""
import os

import numpy as np

from openmpl_amd import detrng
from tests import heatmap_cases as hc

GOLD = hc.GOLD
CELL_MAX = 2.0 ** 30
FORMATS = {"fp32": (23, -126), "fp16": (10, -14), "bf16": (7, -126)}        # explicit mantissa bits, exponent of the smallest normal


# ------------------------------------------------------------------------------------------------------------- rounding
def round_once(x, fmt):
    """float64 -> the nearest value of the format (ties to even, denormals kept), returned as float64 (exact).  Written from
    the definition: scale by the ulp at the value's exponent, np.rint, scale back.  Values stay far below the formats' maxima."""
    mant, emin = FORMATS[fmt]
    x = np.asarray(x, np.float64)
    _, e = np.frexp(x)                                     # |x| = f * 2^e, 0.5 <= f < 1: the exponent of the leading bit is e - 1
    q = np.maximum(e - 1, emin) - mant
    return np.ldexp(np.rint(np.ldexp(x, -q)), q)


def ulp_of(x, fmt):
    """the spacing of the format at |x| (float64 array)"""
    mant, emin = FORMATS[fmt]
    x = np.asarray(x, np.float64)
    _, e = np.frexp(x)
    return np.ldexp(1.0, np.maximum(np.where(x == 0, emin, e - 1), emin) - mant)


def ulps(a, b, fmt="fp32"):
    """distance of two arrays of format values in units of the last place of the larger magnitude"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.isfinite(a).all() and np.isfinite(b).all()
    return np.abs(a - b) / ulp_of(np.maximum(np.abs(a), np.abs(b)), fmt)


# ------------------------------------------------------------------------------------------------------------ rendering
def to_cells(pixels, center=None, scale=None, stride=None, heatmap_size=None):
    """the joints in heatmap cells, float64 on the float32 inputs: (pixel - center) / k + (W/2, H/2) with k = scale_x * 200 / W;
    pixel / stride; or the pixels themselves"""
    p = np.asarray(pixels, np.float32).astype(np.float64)
    if center is not None:
        W, H = heatmap_size
        k = np.asarray(scale, np.float32)[..., 0].astype(np.float64) * 200.0 / float(W)
        return (p - np.asarray(center, np.float32).astype(np.float64)[:, :, None, :]) / k[:, :, None, None] + np.array([W * 0.5, H * 0.5])
    if stride is not None:
        return p / np.array([float(stride[0]), float(stride[1])])
    return p


def noise_draws(seed, first_map, n_maps, HW):
    """draws first_map * HW ... of the stream "render.noise", (n_maps, HW) float64 in [0,1)"""
    key = detrng._stream_key(seed, "render.noise")
    idx = np.uint64(first_map) * np.uint64(HW) + np.arange(n_maps * HW, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = detrng._mix(key + (idx + np.uint64(1)) * detrng._GOLD)
    return ((z >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)).reshape(n_maps, HW)


def render(pixels, conf=None, center=None, scale=None, *, heatmap_size, stride=None, sigma=2.0, mode="reference", fmt="fp32",
           noise_level=0.0, seed=0, first_index=0):
    """pixels (B,V,J,2) -> dict(heatmaps (B,V,J,H,W) float64 holding values of `fmt`, weight (B,V,J) f32, cells (B,V,J,2) f32,
    mu (B,V,J,2) float64: the patch centre of reference mode)"""
    W, H = heatmap_size
    m = to_cells(pixels, center, scale, stride, heatmap_size)
    B, V, J, _ = m.shape
    cf = np.ones((B, V, J), np.float32) if conf is None else np.asarray(conf, np.float32)
    with np.errstate(invalid="ignore"):
        finite = (np.abs(m) <= CELL_MAX).all(-1)                                   # False for NaN
        mu = np.trunc(m + 0.5)
    x, y = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    two_s2 = 2.0 * sigma * sigma
    if mode == "reference":
        t = 3.0 * sigma
        assert t == int(t)
        with np.errstate(invalid="ignore"):
            outside = (mu[..., 0] - t >= W) | (mu[..., 1] - t >= H) | (mu[..., 0] + t + 1 < 0) | (mu[..., 1] + t + 1 < 0)
            weight = np.where(finite & ~outside, cf, np.float32(0.0)).astype(np.float32)
            on = weight > 0.5
        c, amp, reach = mu, np.ones((B, V, J)), t
    else:
        with np.errstate(invalid="ignore"):
            on = finite & (cf > 0)
        weight = np.where(on, cf, np.float32(0.0)).astype(np.float32)
        c, amp, reach = m, cf.astype(np.float64), np.inf
    c = np.where(on[..., None], c, 0.0)                                            # a map that is off never looks at its centre
    dx, dy = x - c[..., 0, None], y - c[..., 1, None]
    gx = np.where(np.abs(dx) > reach, 0.0, np.exp(-(dx * dx) / two_s2))
    gy = np.where(np.abs(dy) > reach, 0.0, np.exp(-(dy * dy) / two_s2)) * np.where(on, amp, 0.0)[..., None]
    val = gx[..., None, :] * gy[..., :, None] * on[..., None, None]
    if noise_level > 0.0:
        val = val + noise_level * noise_draws(seed, first_index * V * J, B * V * J, H * W).reshape(B, V, J, H, W)
    return dict(heatmaps=round_once(val, fmt), weight=weight, cells=m.astype(np.float32), mu=mu, exact=val)


def joints(B, V, J, W, H, seed=0):
    """pixels = cells (B,V,J,2) float32 that cover the map and its surroundings: three in four inside, the others up to 8 cells
    outside on every side; conf (B,V,J) 0.3 .. 1.3.  From 12 joints on the first four have conf 0, 0.4, 0.5, 1 and the last three
    are special (NaN, infinite, beyond 2^30); with fewer the first has conf 0.4."""
    tag = "render.%d.%d.%d.%d.%d" % (B, V, J, W, H)
    p = np.stack([detrng.uniform(seed, tag + ".x", (B, V, J), -8.0, W + 7.0), detrng.uniform(seed, tag + ".y", (B, V, J), -8.0, H + 7.0)], -1)
    inside = detrng.uniform(seed, tag + ".in", (B, V, J), 0.0, 1.0) < 0.75
    q = np.stack([detrng.uniform(seed, tag + ".xi", (B, V, J), 0.0, W - 1.0), detrng.uniform(seed, tag + ".yi", (B, V, J), 0.0, H - 1.0)], -1)
    p = np.where(inside[..., None], q, p).astype(np.float32)
    conf = detrng.uniform(seed, tag + ".conf", (B, V, J), 0.3, 1.3).astype(np.float32)
    flat, cflat = p.reshape(-1, 2), conf.reshape(-1)
    n = flat.shape[0]
    cflat[0] = 0.4
    if n >= 12:
        cflat[:4] = (0.0, 0.4, 0.5, 1.0)
        flat[n - 1] = (np.nan, 3.0)
        flat[n - 2] = (5.0, np.inf)
        flat[n - 3] = (-2.0 ** 31, 4.0)
        cflat[n - 1] = cflat[n - 2] = cflat[n - 3] = 1.0
    return p, conf


def boxes(B, V, seed=0):
    center = detrng.uniform(seed, "render.center.%d.%d" % (B, V), (B, V, 2), 400.0, 600.0)
    scale = detrng.uniform(seed, "render.scale.%d.%d" % (B, V), (B, V, 2), 0.8, 2.5)
    return center, scale


def golden():
    g = np.load(os.path.join(GOLD, "render.npz"))
    return {k: g[k] for k in g.files}


GOLDEN_SIZES = (("64x64", 64, 64), ("64x48", 48, 64))            # tag, W, H
GOLDEN_SIGMAS = (1, 2, 3)


# ------------------------------------------------------------------------------------------------- sub-pixel refinement
def _windows(hm, px, py, r):
    """hm (N,H,W) float64, peaks (N,) -> (N, 2r+1 (j), 2r+1 (i)) windows about the peaks, zero outside the map"""
    N, H, W = hm.shape
    pad = np.zeros((N, H + 2 * r, W + 2 * r))
    pad[:, r:r + H, r:r + W] = hm
    o = np.arange(2 * r + 1)
    return pad[np.arange(N)[:, None, None], (py[:, None] + o)[:, :, None], (px[:, None] + o)[:, None, :]]


def refine(hm, subpixel, radius=2, threshold=1e-6):
    """hm (..., H, W) float32 (16-bit maps: their upcast) -> dict(coords (...,2) f32, maxval, refined (...) bool, cond: the
    smallest a + b over the axes that got a log-quadratic offset, or the smallest S, over the refined maps)."""
    hm = np.asarray(hm, np.float32)
    lead, (H, W) = hm.shape[:-2], hm.shape[-2:]
    plain = hc.decode(hm)
    maxval = plain["maxval"].reshape(-1)
    with np.errstate(invalid="ignore"):
        apply = (maxval > 0) & (maxval < np.inf)
    px, py = (plain["coords"].reshape(-1, 2)[:, a].astype(np.int64) for a in (0, 1))
    flat = np.where(apply[:, None, None], hm.reshape(-1, H, W), np.float32(0.0)).astype(np.float64)      # the others are not looked at
    d = np.zeros((flat.shape[0], 2))
    cond = np.inf
    if subpixel == "gaussian":
        win = _windows(flat, px, py, 1)
        with np.errstate(divide="ignore", invalid="ignore"):
            l0 = np.log(maxval.astype(np.float64))
            for a, (fm, fp, c, n) in enumerate(((win[:, 1, 0], win[:, 1, 2], px, W), (win[:, 0, 1], win[:, 2, 1], py, H))):
                ok = apply & (c > 0) & (c < n - 1) & (fm > 0) & np.isfinite(fm) & (fp > 0) & np.isfinite(fp)
                A, Bb = l0 - np.log(fp), l0 - np.log(fm)
                ok &= (A + Bb) != 0
                d[:, a] = np.where(ok, (Bb - A) / (2.0 * (A + Bb)), 0.0)
                if ok.any():
                    cond = min(cond, float((A + Bb)[ok].min()))
    elif subpixel == "centroid":
        assert isinstance(radius, int) and 1 <= radius <= 8
        win = _windows(flat, px, py, radius)
        w = np.where(win > threshold, win, 0.0)
        S = w.sum((1, 2)) + 2.22e-16
        o = np.arange(-radius, radius + 1, dtype=np.float64)
        d[:, 0] = (w * o[None, None, :]).sum((1, 2)) / S
        d[:, 1] = (w * o[None, :, None]).sum((1, 2)) / S
        if apply.any():
            cond = float(S[apply].min())
    else:
        raise ValueError(subpixel)
    refined = np.stack([px, py], -1).astype(np.float64) + d
    coords = np.where(apply[:, None], refined.astype(np.float32), plain["coords"].reshape(-1, 2)).astype(np.float32)
    return dict(coords=coords.reshape(lead + (2,)), maxval=plain["maxval"], refined=apply.reshape(lead), cond=cond, idx=plain["idx"])


def decode(hm, center=None, scale=None, subpixel="gaussian", radius=2, threshold=1e-6):
    """heatmap_cases.decode with step 2 replaced by the refinement: dict(coords, maxval, pixels, refined, cond)"""
    r = refine(hm, subpixel, radius, threshold)
    W, H = np.asarray(hm).shape[-1], np.asarray(hm).shape[-2]
    pixels = r["coords"]
    if center is not None:
        k = np.asarray(scale, np.float32)[..., 0].astype(np.float64) * 200.0 / float(W)
        half = np.array([W * 0.5, H * 0.5])
        pixels = np.asarray(center, np.float32).astype(np.float64)[..., None, :] + (r["coords"].astype(np.float64) - half) * k[..., None, None]
        pixels = pixels.astype(np.float32)
    r["pixels"] = pixels
    return r


A_PLUS_B_MIN, S_MIN = 1e-6, 1e-3          # what makes the float64 offset well conditioned (tests/test_subpixel_gpu.py)


def well_conditioned(r, subpixel):
    """the condition on a case, not a tolerance: every refined axis has a + b >= 1e-6, every refined map S >= 1e-3"""
    return r["cond"] >= (A_PLUS_B_MIN if subpixel == "gaussian" else S_MIN)


def probe_maps(n=4000, H=64, W=64, seed=11):
    """the maps of the accuracy table: n Gaussians, sigma 2, amplitude 0.2 .. 1, means at least 3 cells from the border ->
    (means (n,2) float64, clean float64 maps (n,H,W), noise draws (n,H,W) in [0,1))"""
    mx = detrng.uniform01(seed, "probe.mx", n) * (W - 7.0) + 3.0
    my = detrng.uniform01(seed, "probe.my", n) * (H - 7.0) + 3.0
    amp = detrng.uniform01(seed, "probe.amp", n) * 0.8 + 0.2
    x, y = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)[:, None]
    clean = amp[:, None, None] * np.exp(-((x - mx[:, None, None]) ** 2 + (y - my[:, None, None]) ** 2) / 8.0)
    u = detrng.uniform01(seed, "probe.noise", n * H * W).reshape(n, H, W)
    return np.stack([mx, my], -1), clean, u


def golden_subpixel():
    g = np.load(os.path.join(GOLD, "subpixel.npz"))
    return {k: g[k] for k in g.files}
