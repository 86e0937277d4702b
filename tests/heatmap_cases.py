"""Restatement of openmpl_amd/heatmaps.py (csrc/heatmaps.hip) in numpy and the maps of its tests (TEST INFRASTRUCTURE ONLY).

decode() restates steps a-c of mpl_decode_heatmaps: np.argmax for the peak (first maximum, NaN as the maximum), float32 coordinates
as get_max_preds keeps them, the sign of the quarter-pixel shift by comparison, and the closed form of transform_preds in float64
on the float32 inputs, rounded once.  It is pinned by tests/golden/heatmaps.npz, which the reference's own get_max_preds,
get_final_preds and generate_heatmap produced (tests/golden/make_golden_heatmaps.py).  Every map comes from openmpl_amd.detrng.
"""
import os

import numpy as np

from openmpl_amd import detrng

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SPECIAL = ("two_maxima", "all_zero", "all_negative", "signed_zeros", "nan", "nan_neighbour", "all_neg_inf")
EDGE = lambda n: (0, 1, 2, n - 2, n - 1)       # both sides of the shift condition 1 < p < n - 1


# ---------------------------------------------------------------------------------------------------------- restatement
def decode(hm, center=None, scale=None, post_process=False):
    """hm (..., H, W) float array (16-bit maps: pass their float32 upcast); center, scale (..., 2) float32 over the leading axes
    but the last (the joints share their view's box) -> dict(coords (...,2) f32, maxval (...) f32, pixels (...,2) f32, idx)."""
    hm = np.asarray(hm, np.float32)
    lead, (H, W) = hm.shape[:-2], hm.shape[-2:]
    flat = hm.reshape(lead + (H * W,))
    idx = np.argmax(flat, axis=-1)
    maxval = np.take_along_axis(flat, idx[..., None], axis=-1)[..., 0]
    positive = maxval > 0.0
    px, py = np.where(positive, idx % W, 0), np.where(positive, idx // W, 0)
    coords = np.stack([px, py], axis=-1).astype(np.float32)
    if post_process:
        inside = (1 < px) & (px < W - 1) & (1 < py) & (py < H - 1)
        at = np.where(inside, py * W + px, W + 1)[..., None]           # any interior cell where the shift does not apply
        pick = lambda off: np.take_along_axis(flat, at + off, axis=-1)[..., 0]

        def quarter(hi, lo):
            s = (hi > lo).astype(np.float32) - (hi < lo).astype(np.float32)
            return np.float32(0.25) * np.where(np.isnan(hi) | np.isnan(lo), np.float32(np.nan), s)
        if H > 2 and W > 2:
            shift = np.stack([quarter(pick(1), pick(-1)), quarter(pick(W), pick(-W))], axis=-1)
            coords = np.where(inside[..., None], coords + shift, coords).astype(np.float32)
    pixels = coords
    if center is not None:
        k = np.asarray(scale, np.float32)[..., 0].astype(np.float64) * 200.0 / float(W)
        half = np.array([W * 0.5, H * 0.5])
        pixels = np.asarray(center, np.float32).astype(np.float64)[..., None, :] + (coords.astype(np.float64) - half) * k[..., None, None]
        pixels = pixels.astype(np.float32)
    return dict(coords=coords, maxval=maxval, pixels=pixels, idx=idx)


def ulps(a, b):
    """distance of two float32 arrays in units of the last place of the larger magnitude; NaN must sit in the same places"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(a)
    d = np.abs(a[ok].astype(np.float64) - b[ok].astype(np.float64))
    return d / np.spacing(np.maximum(np.abs(a[ok]), np.abs(b[ok])).astype(np.float32)).astype(np.float64)


# ----------------------------------------------------------------------------------------------------------------- maps
def gaussian(H, W, mx, my, amp=1.0, sigma=2.0):
    """amp * exp(-((x - mx)^2 + (y - my)^2) / (2 sigma^2)) over the H x W cells, float32; mx, my, amp broadcast over leading axes"""
    mx, my, amp = (np.asarray(a, np.float64)[..., None, None] for a in (mx, my, amp))
    x, y = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)[:, None]
    return (amp * np.exp(-((x - mx) ** 2 + (y - my) ** 2) / (2.0 * sigma * sigma))).astype(np.float32)


def subpixel_maps(n, H, W, seed):
    """n sub-pixel Gaussians, sigma 2, real-valued means anywhere in the map, amplitude 0.2 .. 1, with a little uniform noise"""
    tag = "hm.%d.%d.%d" % (n, H, W)
    mx = detrng.uniform(seed, tag + ".mx", (n,), 0.0, W - 1.0)
    my = detrng.uniform(seed, tag + ".my", (n,), 0.0, H - 1.0)
    amp = detrng.uniform(seed, tag + ".amp", (n,), 0.2, 1.0)
    return gaussian(H, W, mx, my, amp) + detrng.uniform(seed, tag + ".noise", (n, H, W), 0.0, 0.004)


def edge_maps(H, W):
    """25 maps whose peak is at x in EDGE(W), y in EDGE(H); the mean is a fifth of a cell off the peak, so that both shifts have
    a sign where the condition lets them happen"""
    xs, ys = np.meshgrid(EDGE(W), EDGE(H))
    return gaussian(H, W, xs.reshape(-1) + 0.2, ys.reshape(-1) - 0.2, 0.9)


def special_maps(H, W, seed=0):
    """the maps of SPECIAL, in that order"""
    base = subpixel_maps(len(SPECIAL), H, W, seed + 77)
    cx, cy = W // 2, H // 2
    out = []
    for name, m in zip(SPECIAL, base):
        m = m.copy()
        if name == "two_maxima":                       # the first index wins
            m[cy, cx] = m[H - 1, 1] = 2.0
        elif name == "all_zero":
            m[:] = 0.0
        elif name == "all_negative":
            m = -m - 0.01
        elif name == "signed_zeros":                   # -0.0 first: 0.0 is not greater
            m[:] = 0.0
            m.reshape(-1)[::2] = -0.0
        elif name == "nan":                            # two NaNs: the first one is the peak, whatever else the map holds
            m[cy, cx] = 3.0
            m[H - 1, W - 1] = m[cy - 1, 1] = np.nan
        elif name == "nan_neighbour":                  # right of what would be the peak: NaN is the maximum, so the map decodes to
            m[cy, cx] = 3.0                            # (0, 0) with a NaN confidence and the shift never reads the NaN
            m[cy, cx + 1] = np.nan
        elif name == "all_neg_inf":
            m[:] = -np.inf
        out.append(m)
    return np.stack(out).astype(np.float32)


def maps(n, H, W, seed=0):
    """n maps: in turn a sub-pixel Gaussian, a special map, an edge map (each kind cycling through its own list)"""
    g, s, e = subpixel_maps((n + 2) // 3, H, W, seed), special_maps(H, W, seed), edge_maps(H, W)
    return np.stack([(g[i // 3], s[(i // 3) % len(s)], e[(i // 3) % len(e)])[i % 3] for i in range(n)])


def batch(B, V, J, H, W, seed=0):
    """(B,V,J,H,W) float32 of maps(), and the crop boxes: center (B,V,2) inside a 1000 px image, scale (B,V,2) of 160 .. 500 px"""
    hm = maps(B * V * J, H, W, seed).reshape(B, V, J, H, W)
    center = detrng.uniform(seed, "hm.center.%d.%d" % (B, V), (B, V, 2), 100.0, 900.0)
    scale = detrng.uniform(seed, "hm.scale.%d.%d" % (B, V), (B, V, 2), 0.8, 2.5)
    return hm, center, scale


def render(pixels, center, scale, H, W):
    """the detector of the closed loop: pixels (B,V,J,2) -> (B,V,J,H,W) noise-free unit Gaussians, sigma 2, at the sub-pixel cell
    m = (pixel - center) / k + (W/2, H/2), k = scale_x * 200 / W, and m itself"""
    k = np.asarray(scale, np.float64)[..., 0] * 200.0 / W
    m = (np.asarray(pixels, np.float64) - np.asarray(center, np.float64)[:, :, None, :]) / k[:, :, None, None] + np.array([W * 0.5, H * 0.5])
    return gaussian(H, W, m[..., 0], m[..., 1]), m


def golden():
    g = np.load(os.path.join(GOLD, "heatmaps.npz"))
    return {k: g[k] for k in g.files}
