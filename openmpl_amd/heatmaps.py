"""Detector heatmaps decoded into pixel detections, and with cameras into the model's inputs, on the device.

Reference: lib/core/inference.py:22-81 (get_max_preds on an np.ndarray; get_final_preds, a Python double loop over (sample, joint)
for the quarter-pixel shift of TEST.POST_PROCESS, config.py:292, then one cv2.getAffineTransform per sample through
lib/utils/transforms.py:51-94 transform_preds).  One HIP kernel through the C ABI (mpl_decode_heatmaps, csrc/heatmaps.hip) on the
current stream: no synchronisation, no CPU path, and the heatmaps are read where they lie.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence, Tuple, Union

import torch

from . import cabi

_DTYPES = {torch.float32: cabi.HM_F32, torch.float16: cabi.HM_F16, torch.bfloat16: cabi.HM_BF16}


class DecodedHeatmaps(NamedTuple):
    pixels: torch.Tensor                      # (B,V,J,2) image pixels (heatmap cells without center / scale)
    conf: torch.Tensor                        # (B,V,J) the peak values
    coords: Optional[torch.Tensor]            # (B,V,J,2) heatmap cells, with return_coords
    poses: Optional[List[torch.Tensor]]       # with cams: V x (B,J,3), what prepare_inputs(pixels, conf, ...) returns
    rays: Optional[List[torch.Tensor]]        # V x (B,J,3)
    centers: Optional[List[torch.Tensor]]     # V x (B,1,3)


def _in_place(t, inner):
    """(J,H,W) dense inside each sample, samples at a constant non-overlapping stride: the kernel reads such a tensor where it is."""
    J, H, W = inner
    return tuple(t.stride()[-3:]) == (H * W, W, 1) and (t.shape[0] == 1 or t.stride(0) >= J * H * W)


def _check(heatmaps, center, scale, cams, image_size):
    """Shapes first, then dtypes, then devices, as geometry._lines does -> (views, B, V, J, H, W), the views being one (B,J,H,W)
    tensor each or None for the (B,V,J,H,W) tensor."""
    if isinstance(heatmaps, torch.Tensor):
        if heatmaps.ndim != 5 or min(heatmaps.shape) < 1:
            raise RuntimeError("heatmaps: expected one (B,V,J,H,W) tensor or a list of V (B,J,H,W) tensors, got shape %s"
                               % (tuple(heatmaps.shape),))
        B, V, J, H, W = heatmaps.shape
        views = None
        maps = [heatmaps]
    else:
        if not isinstance(heatmaps, (list, tuple)) or len(heatmaps) == 0 or not all(isinstance(t, torch.Tensor) for t in heatmaps):
            raise RuntimeError("heatmaps must be one (B,V,J,H,W) tensor or a non-empty list of tensors, one per view")
        views = maps = list(heatmaps)
        V = len(views)
        if views[0].ndim != 4 or min(views[0].shape) < 1:
            raise RuntimeError("heatmaps[0]: expected shape (B,J,H,W), got %s" % (tuple(views[0].shape),))
        B, J, H, W = views[0].shape
        for v, t in enumerate(views):
            if tuple(t.shape) != (B, J, H, W):
                raise RuntimeError("heatmaps[%d]: expected shape %s, got %s" % (v, (B, J, H, W), tuple(t.shape)))
    if (center is None) != (scale is None):
        raise RuntimeError("center and scale go together (got only %s)" % ("center" if scale is None else "scale"))
    named = [(n, t, s) for n, t, s in (("center", center, (B, V, 2)), ("scale", scale, (B, V, 2)), ("cams", cams, (V, 16))) if t is not None]
    for what, t, shape in named:
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
            raise RuntimeError("%s: expected a tensor of shape %s, got %s" % (what, shape, tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__))
    if cams is not None:
        if image_size is None:
            raise RuntimeError("cams needs image_size (w, h)")
        if not (float(image_size[0]) > 0 and float(image_size[1]) > 0):
            raise RuntimeError("image_size must be positive, got %r" % (tuple(image_size),))
    if V > cabi.MPL_MAX_VIEWS or H * W > 1 << 20 or B * V * J > 1 << 30:
        raise NotImplementedError("at most %d views, 2^20 values per map and 2^30 maps (got %d views, %dx%d maps, %d maps)"
                                  % (cabi.MPL_MAX_VIEWS, V, H, W, B * V * J))
    # dtypes
    for v, t in enumerate(maps):
        if t.dtype not in _DTYPES or t.dtype != maps[0].dtype:
            raise RuntimeError("heatmaps must be float32, float16 or bfloat16, all alike (%s is %s)"
                               % ("heatmaps" if views is None else "heatmaps[%d]" % v, t.dtype))
    for what, t, _ in named:
        want = torch.float64 if what == "cams" else torch.float32
        if t.dtype != want:
            raise RuntimeError("%s must be %s (is %s)%s" % (what, want, t.dtype, " (see pack_cameras)" if what == "cams" else ""))
    # devices
    dev = maps[0].device
    for what, t in [("heatmaps" if views is None else "heatmaps[%d]" % v, t) for v, t in enumerate(maps)] + [(n, t) for n, t, _ in named]:
        if t.device.type != "cuda":
            raise RuntimeError("decode_heatmaps has no CPU path: %s must live on a GPU" % what)
        if t.device != dev:
            raise RuntimeError("%s is on %s, the heatmaps on %s" % (what, t.device, dev))
    return views, B, V, J, H, W


def decode_heatmaps(heatmaps: Union[torch.Tensor, Sequence[torch.Tensor]], center: Optional[torch.Tensor] = None,
                    scale: Optional[torch.Tensor] = None, *, post_process: bool = False, cams: Optional[torch.Tensor] = None,
                    image_size: Optional[Tuple[float, float]] = None, normalize_inputs: bool = True, normalize_cameras: bool = True,
                    return_coords: bool = False) -> DecodedHeatmaps:
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

    Returns DecodedHeatmaps(pixels, conf, coords, poses, rays, centers); what was not asked for is None.  One launch."""
    views, B, V, J, H, W = _check(heatmaps, center, scale, cams, image_size)
    inner = (J, H, W)
    if views is None:
        hm = heatmaps if _in_place(heatmaps, inner) else heatmaps.contiguous()
        keep = [hm]
        ptrs = [hm.data_ptr() + v * hm.stride(1) * hm.element_size() for v in range(V)]
    else:
        ok = all(_in_place(t, inner) for t in views) and (B == 1 or len({t.stride(0) for t in views}) == 1)
        keep = views if ok else [t.contiguous() for t in views]
        ptrs = [t.data_ptr() for t in keep]
    stride = keep[0].stride(0) if B > 1 else J * H * W
    dev = keep[0].device
    lib = cabi.load()
    if center is not None:
        center, scale = center.contiguous(), scale.contiguous()
    pixels = torch.empty((B, V, J, 2), dtype=torch.float32, device=dev)
    conf = torch.empty((B, V, J), dtype=torch.float32, device=dev)
    coords = torch.empty((B, V, J, 2), dtype=torch.float32, device=dev) if return_coords else None
    poses = rays = centers = None
    w = h = 0.0
    if cams is not None:
        cams = cams.contiguous()
        w, h = float(image_size[0]), float(image_size[1])
        mk = lambda *s: [torch.empty(s, dtype=torch.float32, device=dev) for _ in range(V)]
        poses, rays, centers = mk(B, J, 3), mk(B, J, 3), mk(B, 1, 3)
    arr = lambda lst: None if lst is None else (cabi._fp * V)(*[t.data_ptr() for t in lst])
    ptr = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(dev):
        rc = lib.mpl_decode_heatmaps((cabi._fp * V)(*ptrs), _DTYPES[keep[0].dtype], stride, B, V, J, H, W, int(bool(post_process)),
                                     ptr(center), ptr(scale), pixels.data_ptr(), conf.data_ptr(), ptr(coords), ptr(cams), w, h,
                                     int(bool(normalize_inputs)), int(bool(normalize_cameras)), arr(poses), arr(rays), arr(centers),
                                     torch.cuda.current_stream().cuda_stream)
    cabi.check(rc, "mpl_decode_heatmaps")
    return DecodedHeatmaps(pixels, conf, coords, poses, rays, centers)
