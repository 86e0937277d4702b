"""What the utility wrappers share on their way into the C ABI: pointers and pointer tables, 3-vectors, the model-input lists
(poses, rays, centers) and the heatmap argument of decode_heatmaps and rpsm.  The launch itself is cabi.launch.
"""
from __future__ import annotations

import torch

from . import cabi

HM_DTYPES = {torch.float32: cabi.HM_F32, torch.float16: cabi.HM_F16, torch.bfloat16: cabi.HM_BF16}


def ptr(t):
    return None if t is None else t.data_ptr()


def table(lst):
    """A list of tensors as the host array of device pointers the C ABI takes; None stays None."""
    return None if lst is None else (cabi._fp * len(lst))(*[t.data_ptr() for t in lst])


def vec3(v, default, what="scale / offset / weight_axis take 3 values"):
    """None, a number, 3 values or a tensor of 3 -> 3 floats; `what` is the complaint about any other length."""
    if v is None:
        return [default] * 3
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().reshape(-1).tolist()
    elif isinstance(v, (int, float)):
        v = [float(v)] * 3
    v = [float(x) for x in v]
    if len(v) != 3:
        raise RuntimeError(what)
    return v


def view_lists(B, V, J, dev):
    """Freshly allocated (poses, rays, centers): V tensors (B,J,3), (B,J,3), (B,1,3) each, what model(poses, rays=, centers=) takes."""
    mk = lambda *s: [torch.empty(s, dtype=torch.float32, device=dev) for _ in range(V)]
    return mk(B, J, 3), mk(B, J, 3), mk(B, 1, 3)


# ---- the heatmap argument: one (B,V,J,H,W) tensor or a list of V (B,J,H,W) tensors.  A caller checks in three steps, with its own
# checks between them -- shapes (heatmap_shapes, named_shapes), then dtypes and devices (dtypes_and_devices), each complaint naming
# its argument -- and then resolves the argument into what the C ABI takes (heatmap_table).

def heatmap_shapes(heatmaps, exc):
    """-> (views, maps, B, V, J, H, W): views the list of (B,J,H,W) tensors or None for the one tensor, maps the tensors to check."""
    if isinstance(heatmaps, torch.Tensor):
        if heatmaps.ndim != 5 or min(heatmaps.shape) < 1:
            raise exc("heatmaps: expected one (B,V,J,H,W) tensor or a list of V (B,J,H,W) tensors, got shape %s" % (tuple(heatmaps.shape),))
        B, V, J, H, W = heatmaps.shape
        return None, [heatmaps], B, V, J, H, W
    if not isinstance(heatmaps, (list, tuple)) or len(heatmaps) == 0 or not all(isinstance(t, torch.Tensor) for t in heatmaps):
        raise exc("heatmaps must be one (B,V,J,H,W) tensor or a non-empty list of tensors, one per view")
    views = list(heatmaps)
    if views[0].ndim != 4 or min(views[0].shape) < 1:
        raise exc("heatmaps[0]: expected shape (B,J,H,W), got %s" % (tuple(views[0].shape),))
    B, J, H, W = views[0].shape
    for v, t in enumerate(views):
        if tuple(t.shape) != (B, J, H, W):
            raise exc("heatmaps[%d]: expected shape %s, got %s" % (v, (B, J, H, W), tuple(t.shape)))
    return views, views, B, len(views), J, H, W


def named_shapes(named, exc):
    """named: (name, tensor, shape, dtype) per tensor argument."""
    for what, t, shape, _ in named:
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
            raise exc("%s: expected a tensor of shape %s, got %s" % (what, shape, tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__))


def dtypes_and_devices(views, maps, named, fn, exc):
    """The dtype complaints (exc) of the maps and the named tensors, then the device complaints (RuntimeError: `fn` has no CPU path)."""
    names = ["heatmaps" if views is None else "heatmaps[%d]" % v for v in range(len(maps))]
    for what, t in zip(names, maps):
        if t.dtype not in HM_DTYPES or t.dtype != maps[0].dtype:
            raise exc("heatmaps must be float32, float16 or bfloat16, all alike (%s is %s)" % (what, t.dtype))
    for what, t, _, want in named:
        if t.dtype != want:
            raise exc("%s must be %s (is %s)%s" % (what, want, t.dtype, " (see pack_cameras)" if what == "cams" else ""))
    dev = maps[0].device
    for what, t in list(zip(names, maps)) + [(n, t) for n, t, _, _ in named]:
        if t.device.type != "cuda":
            raise RuntimeError("%s has no CPU path: %s must live on a GPU" % (fn, what))
        if t.device != dev:
            raise RuntimeError("%s is on %s, the heatmaps on %s" % (what, t.device, dev))


def _in_place(t, inner):
    """(J,H,W) dense inside each sample, samples at a constant non-overlapping stride: the kernels read such a tensor where it is."""
    J, H, W = inner
    return tuple(t.stride()[-3:]) == (H * W, W, 1) and (t.shape[0] == 1 or t.stride(0) >= J * H * W)


def heatmap_table(heatmaps, views, B, V, J, H, W, writable=False):
    """-> (keep, table, batch stride in elements, dtype code): the tensors the table points into and the first three arguments of
    mpl_decode_heatmaps / mpl_rpsm / mpl_render_heatmaps.  Nothing is copied unless a (J,H,W) block is not dense or the views
    differ in their batch stride.  writable: the table is written (render_heatmaps' out=), so a copy would be of no use and the
    views of one tensor must not overlap either: such an argument raises RuntimeError."""
    inner = (J, H, W)
    if views is None:
        ok = _in_place(heatmaps, inner) and (not writable or V == 1 or heatmaps.stride(1) >= J * H * W)
        if writable and not ok:
            raise RuntimeError("out must be written where it lies: every (J,H,W) block dense, samples and views at non-overlapping strides")
        hm = heatmaps if ok else heatmaps.contiguous()
        keep = [hm]
        ptrs = [hm.data_ptr() + v * hm.stride(1) * hm.element_size() for v in range(V)]
    else:
        ok = all(_in_place(t, inner) for t in views) and (B == 1 or len({t.stride(0) for t in views}) == 1)
        if writable and not ok:
            raise RuntimeError("out must be written where it lies: every (J,H,W) block dense, samples of all views at one non-overlapping stride")
        keep = views if ok else [t.contiguous() for t in views]
        ptrs = [t.data_ptr() for t in keep]
    stride = keep[0].stride(0) if B > 1 else J * H * W
    return keep, (cabi._fp * V)(*ptrs), stride, HM_DTYPES[keep[0].dtype]
