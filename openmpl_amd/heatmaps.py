"""Detector heatmaps decoded into pixel detections, and with cameras into the model's inputs, on the device; and the way there:
heatmaps rendered from 2D joints (render_heatmaps, csrc/heatmap_render.hip; reference: generate_heatmap,
lib/dataset/joints_dataset_mpl.py:828-870).

Reference: lib/core/inference.py:22-81 (get_max_preds on an np.ndarray; get_final_preds, a Python double loop over (sample, joint)
for the quarter-pixel shift of TEST.POST_PROCESS, config.py:292, then one cv2.getAffineTransform per sample through
lib/utils/transforms.py:51-94 transform_preds).  One HIP kernel through the C ABI (mpl_decode_heatmaps, csrc/heatmaps.hip) on the
current stream: no synchronisation, no CPU path, and the heatmaps are read where they lie.
"""
from __future__ import annotations

import functools
from typing import List, NamedTuple, Optional, Sequence, Tuple, Union

import torch

from . import cabi, detrng
from ._marshal import HM_DTYPES, dtypes_and_devices, heatmap_shapes, heatmap_table, named_shapes, ptr, table, view_lists
from .inputs import prepare_inputs


class DecodedHeatmaps(NamedTuple):
    pixels: torch.Tensor                      # (B,V,J,2) image pixels (heatmap cells without center / scale)
    conf: torch.Tensor                        # (B,V,J) the peak values
    coords: Optional[torch.Tensor]            # (B,V,J,2) heatmap cells, with return_coords
    poses: Optional[List[torch.Tensor]]       # with cams: V x (B,J,3), what prepare_inputs(pixels, conf, ...) returns
    rays: Optional[List[torch.Tensor]]        # V x (B,J,3)
    centers: Optional[List[torch.Tensor]]     # V x (B,1,3)


def _check(heatmaps, center, scale, cams, image_size, distortion=None):
    """Shapes first, then dtypes, then devices, as geometry._lines does -> (views, B, V, J, H, W), the views being one (B,J,H,W)
    tensor each or None for the (B,V,J,H,W) tensor."""
    views, maps, B, V, J, H, W = heatmap_shapes(heatmaps, RuntimeError)
    if (center is None) != (scale is None):
        raise RuntimeError("center and scale go together (got only %s)" % ("center" if scale is None else "scale"))
    named = [(n, t, s, d) for n, t, s, d in (("center", center, (B, V, 2), torch.float32), ("scale", scale, (B, V, 2), torch.float32),
                                             ("cams", cams, (V, 16), torch.float64), ("distortion", distortion, (V, 5), torch.float64))
             if t is not None]
    named_shapes(named, RuntimeError)
    if cams is not None:
        if image_size is None:
            raise RuntimeError("cams needs image_size (w, h)")
        if not (float(image_size[0]) > 0 and float(image_size[1]) > 0):
            raise RuntimeError("image_size must be positive, got %r" % (tuple(image_size),))
    if V > cabi.MPL_MAX_VIEWS or H * W > 1 << 20 or B * V * J > 1 << 30:
        raise NotImplementedError("at most %d views, 2^20 values per map and 2^30 maps (got %d views, %dx%d maps, %d maps)"
                                  % (cabi.MPL_MAX_VIEWS, V, H, W, B * V * J))
    dtypes_and_devices(views, maps, named, "decode_heatmaps", RuntimeError)
    return views, B, V, J, H, W


def decode_heatmaps(heatmaps: Union[torch.Tensor, Sequence[torch.Tensor]], center: Optional[torch.Tensor] = None,
                    scale: Optional[torch.Tensor] = None, *, post_process: bool = False, cams: Optional[torch.Tensor] = None,
                    image_size: Optional[Tuple[float, float]] = None, normalize_inputs: bool = True, normalize_cameras: bool = True,
                    return_coords: bool = False, subpixel: Optional[str] = None, radius: int = 2,
                    threshold: float = 1e-6, distortion: Optional[torch.Tensor] = None) -> DecodedHeatmaps:
    """heatmaps: a list of V (B,J,H,W) tensors (what a 2D backbone returns per view) or one (B,V,J,H,W) tensor; float32, float16 or
    bfloat16 on a GPU.  A tensor whose (J,H,W) block is dense is read in place, whatever its batch stride; nothing is copied to
    change a layout.  Per heatmap, as get_final_preds does:

    1. peak: the first index of the maximum (NaN counts as the maximum, -0.0 and 0.0 tie), conf = its value; x = idx % W,
       y = idx // W, or (0, 0) when the value is not positive.
    2. post_process (TEST.POST_PROCESS): where 1 < x < W-1 and 1 < y < H-1, a quarter cell towards the higher neighbour on each
       axis; a NaN neighbour gives a NaN coordinate.  These are `coords` (return_coords).
    3. center, scale (B,V,2) float32, the crop boxes of the detector: pixel = center + (coord - (W/2, H/2)) * scale[...,0] * 200 / W
       (scale[...,1] is not read, as in the reference).  Without them pixels = coords.  The reference fits this affine map through
       three float32-rounded points; the closed form differs from it by a few float32 ulps.
    4. cams (V,16) float64 (pack_cameras) with image_size (w, h): poses, rays, centers, bitwise those of
       prepare_inputs(pixels, conf, cams, image_size, normalize_inputs, normalize_cameras), for model(poses, rays=, centers=).

    subpixel replaces step 2 (and excludes post_process) by a refinement of the integer peak (x0, y0), which locates a clean
    Gaussian to a thousandth of a cell where the quarter shift is good to a quarter.  It applies only where 0 < conf < inf;
    elsewhere the coordinates are those of step 1.  The offset is float64, x0 + d is rounded once, steps 3 and 4 follow on it.
    "gaussian": per axis, with f-, f0, f+ the peak and its neighbours, a = ln f0 - ln f+, b = ln f0 - ln f-,
       d = (b - a) / (2 (a + b)): exact for a Gaussian of any sigma, the best on clean maps; d = 0 at the border, beside a neighbour
       that is not positive and finite, or where a + b == 0.
    "centroid": the intent of the reference's find_tensor_peak_batch (lib/core/inference.py:84-134): the centroid, relative to the
       peak, of the values above `threshold` in the window of `radius` (1..8) cells about it, cells outside the map counting 0; the
       sum of the weights gets 2.22e-16 added.  More robust under noise, biased towards the peak on clean maps.

    distortion (V,5) float64 (pack_distortion), with cams: the decoded pixels are what the lens showed the detector, so the rays
    must go through the undistorted pixels.  The plain decode is then followed by prepare_inputs(pixels, conf, cams, image_size,
    normalize_inputs, normalize_cameras, distortion=) -- TWO launches, and bitwise that composition; the Newton inverse is kept
    out of the decode kernel, whose finishing lane is already its longest path.

    Returns DecodedHeatmaps(pixels, conf, coords, poses, rays, centers); what was not asked for is None.  One launch, two with
    distortion."""
    if distortion is not None and cams is None:
        raise RuntimeError("distortion needs cams: it only changes the rays")
    if subpixel not in cabi.REFINE:
        raise RuntimeError("subpixel must be None, 'gaussian' or 'centroid', got %r" % (subpixel,))
    if subpixel is not None and post_process:
        raise RuntimeError("post_process and subpixel exclude each other: both replace the integer peak")
    if subpixel == "centroid":
        if isinstance(radius, bool) or not isinstance(radius, int) or not 1 <= radius <= 8:
            raise RuntimeError("radius must be an integer from 1 to 8, got %r" % (radius,))
        if not float(threshold) == float(threshold):
            raise RuntimeError("threshold must be a number, got %r" % (threshold,))
    views, B, V, J, H, W = _check(heatmaps, center, scale, cams, image_size, distortion)
    keep, hm, stride, dtype = heatmap_table(heatmaps, views, B, V, J, H, W)
    dev = keep[0].device
    if center is not None:
        center, scale = center.contiguous(), scale.contiguous()
    pixels = torch.empty((B, V, J, 2), dtype=torch.float32, device=dev)
    conf = torch.empty((B, V, J), dtype=torch.float32, device=dev)
    coords = torch.empty((B, V, J, 2), dtype=torch.float32, device=dev) if return_coords else None
    poses = rays = centers = None
    w = h = 0.0
    fused = cams if distortion is None else None          # the decode kernel writes the model inputs itself
    if fused is not None:
        fused = fused.contiguous()
        w, h = float(image_size[0]), float(image_size[1])
        poses, rays, centers = view_lists(B, V, J, dev)
    args = (hm, dtype, stride, B, V, J, H, W, int(bool(post_process)), ptr(center), ptr(scale), pixels.data_ptr(), conf.data_ptr(),
            ptr(coords), ptr(fused), w, h, int(bool(normalize_inputs)), int(bool(normalize_cameras)), table(poses), table(rays), table(centers))
    if subpixel is None:
        cabi.launch("decode_heatmaps", dev, *args)
    else:
        cabi.launch("decode_heatmaps_ex", dev, *args, cabi.REFINE[subpixel], int(radius), float(threshold))
    if distortion is not None:
        poses, rays, centers = prepare_inputs(pixels, conf, cams, image_size, normalize_inputs, normalize_cameras, distortion=distortion)
    return DecodedHeatmaps(pixels, conf, coords, poses, rays, centers)


class RenderedHeatmaps(NamedTuple):
    heatmaps: Union[torch.Tensor, Sequence[torch.Tensor]]     # (B,V,J,H,W), or `out` as it was given
    weight: torch.Tensor                                      # (B,V,J) float32: generate_heatmap's target_weight
    cells: torch.Tensor                                       # (B,V,J,2) float32: the joints in heatmap cells


@functools.lru_cache(maxsize=64)
def _noise_key(seed):
    return int(detrng._stream_key(seed, "render.noise", 0))


def _pair(v, what):
    try:
        a, b = v
        return a, b
    except (TypeError, ValueError):
        raise RuntimeError("%s takes two values, got %r" % (what, v))


def render_heatmaps(pixels: torch.Tensor, conf: Optional[torch.Tensor] = None, center: Optional[torch.Tensor] = None,
                    scale: Optional[torch.Tensor] = None, *, heatmap_size: Optional[Tuple[int, int]] = None,
                    stride: Optional[Tuple[float, float]] = None, sigma: float = 2.0, mode: str = "reference",
                    dtype: Optional[torch.dtype] = None, noise_level: float = 0.0, seed: int = 0, first_index: int = 0,
                    out: Union[None, torch.Tensor, Sequence[torch.Tensor]] = None) -> RenderedHeatmaps:
    """pixels (B,V,J,2) float32 GPU -> one Gaussian heatmap per joint, heatmap_size = (W, H) cells, in one launch.

    The cell m of a joint, in float64 on the float32 inputs: with center, scale (B,V,2), the crop boxes,
    m = (pixel - center) / k + (W/2, H/2), k = scale[...,0] * 200 / W -- the exact inverse of step 3 of decode_heatmaps; with
    stride = (sx, sy), m = pixel / stride, the reference's feat_stride; with neither, pixels are cells.  `cells` is m rounded once.

    mode="reference" is the reference's generate_heatmap for a batch: mu = int(m + 0.5) (towards zero); weight = conf (default 1),
    0 when the patch mu +/- 3 sigma lies wholly outside the map; where weight > 0.5 the patch holds
    exp(-(dx^2 + dy^2) / (2 sigma^2)) at integer dx, dy, every other cell is 0.  3 * sigma must be an integer.
    mode="subpixel": conf * exp(-((x - mx)^2 + (y - my)^2) / (2 sigma^2)) on every cell, weight = conf; a joint whose conf is not
    above 0 gets a zero map and weight 0.
    Both: a cell that is not finite or beyond +/-2^30 gives a zero map and weight 0 (the reference's int(nan) raises).  Values are
    formed in float64 and rounded once to dtype (float32, float16 or bfloat16; default: that of `out`, else float32).

    noise_level = a > 0 adds a * u to every cell of every map before that rounding, u the draws of detrng's stream "render.noise"
    of `seed`, indexed by the cell's position in the uncut run -- first_index is the global index of sample 0 -- so a run cut into
    batches is bitwise the uncut run.  out: one (B,V,J,H,W) tensor or V (B,J,H,W) tensors whose (J,H,W) blocks are dense, written
    where they lie (what decode_heatmaps and rpsm read in place); without it one tensor is allocated.

    Returns RenderedHeatmaps(heatmaps, weight, cells).  Runs on the current stream and does not synchronise; no CPU path."""
    if not isinstance(pixels, torch.Tensor) or pixels.ndim != 4 or pixels.shape[-1] != 2 or min(pixels.shape) < 1:
        raise RuntimeError("pixels: expected a tensor of shape (B,V,J,2), got %s"
                           % (tuple(pixels.shape) if isinstance(pixels, torch.Tensor) else type(pixels).__name__,))
    B, V, J, _ = pixels.shape
    if (center is None) != (scale is None):
        raise RuntimeError("center and scale go together (got only %s)" % ("center" if scale is None else "scale"))
    if stride is not None:
        if center is not None:
            raise RuntimeError("stride and center / scale exclude each other")
        sx, sy = (float(x) for x in _pair(stride, "stride"))
        if not (0.0 < sx < float("inf") and 0.0 < sy < float("inf")):
            raise RuntimeError("stride must be positive, got %r" % (tuple(stride),))
    else:
        sx = sy = 0.0
    views = maps = None
    if out is not None:
        views, maps, oB, oV, oJ, H, W = heatmap_shapes(out, RuntimeError)
        if (oB, oV, oJ) != (B, V, J):
            raise RuntimeError("out holds (B,V,J) = %s, pixels %s" % ((oB, oV, oJ), (B, V, J)))
        if heatmap_size is not None and tuple(int(x) for x in _pair(heatmap_size, "heatmap_size")) != (W, H):
            raise RuntimeError("heatmap_size (W, H) = %s, but out holds maps of %d rows and %d columns" % (tuple(heatmap_size), H, W))
    else:
        if heatmap_size is None:
            raise RuntimeError("heatmap_size (W, H) is needed without out")
        W, H = (int(x) for x in _pair(heatmap_size, "heatmap_size"))
        if W < 1 or H < 1:
            raise RuntimeError("heatmap_size must be positive, got %r" % (tuple(heatmap_size),))
    named = [(n, t, s, torch.float32) for n, t, s in (("conf", conf, (B, V, J)), ("center", center, (B, V, 2)), ("scale", scale, (B, V, 2)))
             if t is not None]
    named_shapes(named, RuntimeError)
    if mode not in cabi.RENDER_MODES:
        raise RuntimeError("mode must be one of %s, got %r" % (", ".join(sorted(cabi.RENDER_MODES)), mode))
    sigma, noise_level = float(sigma), float(noise_level)
    if not 0.0 < sigma <= 1e6:
        raise RuntimeError("sigma must be positive, got %r" % sigma)
    if mode == "reference" and 3.0 * sigma != int(3.0 * sigma):
        raise RuntimeError("mode='reference' needs an integer 3 * sigma, the half width of the patch (sigma is %r)" % sigma)
    if not 0.0 <= noise_level < float("inf"):
        raise RuntimeError("noise_level must not be negative, got %r" % noise_level)
    if first_index < 0:
        raise RuntimeError("first_index must not be negative")
    if V > cabi.MPL_MAX_VIEWS or H * W > 1 << 20 or B * V * J > 1 << 30:
        raise NotImplementedError("at most %d views, 2^20 values per map and 2^30 maps (got %d views, %dx%d maps, %d maps)"
                                  % (cabi.MPL_MAX_VIEWS, V, H, W, B * V * J))
    # dtypes
    if out is not None:
        for t in maps:
            if t.dtype not in HM_DTYPES or t.dtype != maps[0].dtype:
                raise RuntimeError("out must be float32, float16 or bfloat16, all alike (got %s)" % (t.dtype,))
        if dtype is not None and dtype != maps[0].dtype:
            raise RuntimeError("dtype is %s, out is %s" % (dtype, maps[0].dtype))
    elif dtype is None:
        dtype = torch.float32
    elif dtype not in HM_DTYPES:
        raise RuntimeError("dtype must be float32, float16 or bfloat16, got %s" % (dtype,))
    for what, t, _, want in [("pixels", pixels, None, torch.float32)] + named:
        if t.dtype != want:
            raise RuntimeError("%s must be %s (is %s)" % (what, want, t.dtype))
    # devices
    if pixels.device.type != "cuda":
        raise RuntimeError("render_heatmaps has no CPU path: pixels must live on a GPU")
    dev = pixels.device
    for what, t in [(n, t) for n, t, _, _ in named] + [("out", t) for t in (maps or [])]:
        if t.device != dev:
            raise RuntimeError("%s is on %s, pixels on %s" % (what, t.device, dev))
    if out is None:
        out = torch.empty((B, V, J, H, W), dtype=dtype, device=dev)
    keep, hm, bstride, code = heatmap_table(out, views, B, V, J, H, W, writable=True)
    pixels = pixels.contiguous()
    conf = None if conf is None else conf.contiguous()
    if center is not None:
        center, scale = center.contiguous(), scale.contiguous()
    weight = torch.empty((B, V, J), dtype=torch.float32, device=dev)
    cells = torch.empty((B, V, J, 2), dtype=torch.float32, device=dev)
    key = _noise_key(int(seed)) if noise_level > 0.0 else 0
    cabi.launch("render_heatmaps", dev, hm, code, bstride, B, V, J, H, W, pixels.data_ptr(), ptr(conf), ptr(center), ptr(scale), sx, sy,
                cabi.RENDER_MODES[mode], sigma, noise_level, key, int(first_index), weight.data_ptr(), cells.data_ptr())
    return RenderedHeatmaps(out, weight, cells)
