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
from ._marshal import dtypes_and_devices, heatmap_shapes, heatmap_table, named_shapes, ptr, table, view_lists


class DecodedHeatmaps(NamedTuple):
    pixels: torch.Tensor                      # (B,V,J,2) image pixels (heatmap cells without center / scale)
    conf: torch.Tensor                        # (B,V,J) the peak values
    coords: Optional[torch.Tensor]            # (B,V,J,2) heatmap cells, with return_coords
    poses: Optional[List[torch.Tensor]]       # with cams: V x (B,J,3), what prepare_inputs(pixels, conf, ...) returns
    rays: Optional[List[torch.Tensor]]        # V x (B,J,3)
    centers: Optional[List[torch.Tensor]]     # V x (B,1,3)


def _check(heatmaps, center, scale, cams, image_size):
    """Shapes first, then dtypes, then devices, as geometry._lines does -> (views, B, V, J, H, W), the views being one (B,J,H,W)
    tensor each or None for the (B,V,J,H,W) tensor."""
    views, maps, B, V, J, H, W = heatmap_shapes(heatmaps, RuntimeError)
    if (center is None) != (scale is None):
        raise RuntimeError("center and scale go together (got only %s)" % ("center" if scale is None else "scale"))
    named = [(n, t, s, d) for n, t, s, d in (("center", center, (B, V, 2), torch.float32), ("scale", scale, (B, V, 2), torch.float32),
                                             ("cams", cams, (V, 16), torch.float64)) if t is not None]
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
    keep, hm, stride, dtype = heatmap_table(heatmaps, views, B, V, J, H, W)
    dev = keep[0].device
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
        poses, rays, centers = view_lists(B, V, J, dev)
    cabi.launch("decode_heatmaps", dev, hm, dtype, stride, B, V, J, H, W, int(bool(post_process)), ptr(center), ptr(scale),
                pixels.data_ptr(), conf.data_ptr(), ptr(coords), ptr(cams), w, h, int(bool(normalize_inputs)), int(bool(normalize_cameras)),
                table(poses), table(rays), table(centers))
    return DecodedHeatmaps(pixels, conf, coords, poses, rays, centers)
