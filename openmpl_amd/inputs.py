"""Device-side replacement of the per-sample input preparation of OpenMPL's datasets.

Reference: lib/dataset/joints_dataset_mpl.py:615-623, :646, :762-774, :817-820, :872-904.  From raw detections
(B,V,J,2) [+ confidences (B,V,J)] and one calibration per view it produces exactly what the model call
`model(input, centers=centers, rays=rays)` (function_mpl.py:350) takes.  One HIP kernel through the C ABI; no CPU path.

The lens: `distortion` is a (V,5) float64 tensor k1 k2 k3 p1 p2 per view (pack_distortion), the radial / tangential polynomial of
lib/multiviews/cameras.py:22-46 (project_point_radial), stated once on the device with its Newton inverse (csrc/views.hpp).  Every
call that projects applies it and every call that builds a ray inverts it; without the argument a call launches what it always has.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import cabi
from ._marshal import ptr, table, view_lists


def pack_cameras(cameras, device) -> torch.Tensor:
    """cameras: sequence of dicts with fx, fy, cx, cy, R (3x3 world->camera), t (camera centre, 3) -> device (V,16) f64."""
    rows = [np.concatenate([[float(c["fx"]), float(c["fy"]), float(c["cx"]), float(c["cy"])],
                            np.asarray(c["R"], np.float64).reshape(-1), np.asarray(c["t"], np.float64).reshape(-1)])
            for c in cameras]
    return torch.from_numpy(np.stack(rows)).to(device)


def pack_distortion(cameras, device) -> torch.Tensor:
    """cameras: the sequence of dicts pack_cameras takes; `k` (3 radial) and `p` (2 tangential coefficients) as the reference's
    camera dicts carry them (lib/dataset/joints_dataset_mpl.py:269, :337) -> device (V,5) f64 k1 k2 k3 p1 p2.  A camera without them
    gives zeros, the pinhole."""
    rows = []
    for c in cameras:
        k = np.zeros(3) if c.get("k") is None else np.asarray(c["k"], np.float64).reshape(-1)
        p = np.zeros(2) if c.get("p") is None else np.asarray(c["p"], np.float64).reshape(-1)
        if k.shape != (3,) or p.shape != (2,):
            raise RuntimeError("a camera's k takes 3 values and its p 2 (got %d and %d)" % (k.size, p.size))
        rows.append(np.concatenate([k, p]))
    return torch.from_numpy(np.stack(rows)).to(device)


def check_distortion(distortion, V, dev):
    """distortion=None stays None; anything else must be the (V,5) float64 table on `dev` -> contiguous"""
    if distortion is None:
        return None
    if not isinstance(distortion, torch.Tensor) or tuple(distortion.shape) != (V, 5) or distortion.dtype != torch.float64:
        raise RuntimeError("distortion must be float64 (V,5) = (%d,5): k1 k2 k3 p1 p2 per view (see pack_distortion)" % V)
    if distortion.device != dev:
        raise RuntimeError("distortion must live on the device of the other tensors (is on %s)" % (distortion.device,))
    return distortion.contiguous()


def _check_pixels(pixels, cams, fn, what="joints_px"):
    if not isinstance(pixels, torch.Tensor) or pixels.device.type != "cuda":
        raise RuntimeError("%s has no CPU path: tensors must live on a GPU" % fn)
    if pixels.ndim != 4 or pixels.shape[-1] != 2 or pixels.dtype != torch.float32:
        raise RuntimeError("%s must be float32 (B,V,J,2)" % what)
    B, V, J, _ = pixels.shape
    if not isinstance(cams, torch.Tensor) or tuple(cams.shape) != (V, 16) or cams.dtype != torch.float64 or cams.device != pixels.device:
        raise RuntimeError("cams must be float64 (V,16) on the same device (see pack_cameras)")
    return B, V, J


def prepare_inputs(joints_px: torch.Tensor, conf: Optional[torch.Tensor], cams: torch.Tensor, image_size: Tuple[float, float],
                   normalize_inputs: bool = True, normalize_cameras: bool = True, distortion: Optional[torch.Tensor] = None
                   ) -> Tuple[List[torch.Tensor], List[torch.Tensor], List[torch.Tensor]]:
    """joints_px (B,V,J,2) float32 GPU, conf (B,V,J) or None, cams (V,16) float64 GPU (pack_cameras).
    Returns (poses, rays, centers): lists of V tensors (B,J,3), (B,J,3), (B,1,3).

    distortion (V,5) float64 (pack_distortion): poses stay what they are, the observed pixel and the confidence; the ray goes
    through the undistorted pixel.  A joint whose pixel no pinhole point maps to (it lies beyond the fold of the polynomial) keeps
    its pinhole ray and gets confidence 0 in poses[..., 2], like a missing joint, so that the triangulations and the epipolar score
    drop the view.  Zero coefficients give the bits of the call without the argument."""
    B, V, J = _check_pixels(joints_px, cams, "prepare_inputs")
    dev = joints_px.device
    distortion = check_distortion(distortion, V, dev)
    joints_px = joints_px.contiguous()
    if conf is not None:
        conf = conf.reshape(B, V, J).to(torch.float32).contiguous()
    poses, rays, centers = view_lists(B, V, J, dev)
    tail = (B, V, J, float(image_size[0]), float(image_size[1]), int(normalize_inputs), int(normalize_cameras), table(poses), table(rays),
            table(centers))
    if distortion is None:
        cabi.launch("prepare_inputs", dev, joints_px.data_ptr(), ptr(conf), cams.data_ptr(), *tail)
    else:
        cabi.launch("prepare_inputs_ex", dev, joints_px.data_ptr(), ptr(conf), cams.data_ptr(), distortion.data_ptr(), *tail)
    return poses, rays, centers


def _lens(pixels, cams, distortion, direction, fn):
    B, V, J = _check_pixels(pixels, cams, fn, "pixels")
    if V > cabi.MPL_MAX_VIEWS or B * V * J > 1 << 30:
        raise RuntimeError("at most %d views and 2^30 points, got %d views, %d points" % (cabi.MPL_MAX_VIEWS, V, B * V * J))
    dev = pixels.device
    if distortion is None:
        raise RuntimeError("%s needs distortion, float64 (V,5) (see pack_distortion)" % fn)
    distortion = check_distortion(distortion, V, dev)
    out = torch.empty((B, V, J, 2), dtype=torch.float32, device=dev)
    valid = torch.empty((B, V, J), dtype=torch.bool, device=dev) if direction == cabi.DISTORT_REMOVE else None
    cabi.launch("undistort_points", dev, pixels.contiguous().data_ptr(), cams.contiguous().data_ptr(), distortion.data_ptr(), B, V, J, direction,
                out.data_ptr(), ptr(valid))
    return out, valid


def undistort_points(pixels: torch.Tensor, cams: torch.Tensor, distortion: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Observed pixels (B,V,J,2) float32 GPU -> (the pixels a pinhole camera with the same intrinsics would have seen, valid (B,V,J)
    bool).  The inverse of the lens polynomial by Newton's iteration in float64; a pixel that is not invertible -- no pinhole point
    maps to it -- is NaN and not valid.  Zero coefficients return the input.  One launch, no synchronisation."""
    return _lens(pixels, cams, distortion, cabi.DISTORT_REMOVE, "undistort_points")


def distort_points(pixels: torch.Tensor, cams: torch.Tensor, distortion: torch.Tensor) -> torch.Tensor:
    """Pinhole pixels (B,V,J,2) float32 GPU -> the pixels the lens puts them at (the forward polynomial).  One launch."""
    return _lens(pixels, cams, distortion, cabi.DISTORT_APPLY, "distort_points")[0]


class HostStager:
    """One pinned staging buffer + ONE host-to-device copy per batch for callers that hold the inputs on the host (the
    loop of validate(), function_mpl.py:334-351, hands `model(input, centers=, rays=)` CPU tensors): the V x {(b,J,3) poses,
    (b,J,3) rays, (b,1,3) centers} are packed back to back into pinned memory and cross PCIe as one transfer instead of
    3V small ones; the returned lists are views into one device buffer (layouts exactly those the model expects).

    `batch` is the LARGEST batch: a shorter one (the ragged last batch of a loader without drop_last) is staged into a
    prefix.  The returned views ALIAS the stager's device buffer, which the next stage() overwrites: consume them on the
    stream that was current when stage() ran (the copy is enqueued there, so a forward launched on it afterwards is ordered
    behind the copy and ahead of the next one), or use two stagers alternately as bench.py does."""

    def __init__(self, batch: int, views: int, joints: int, device):
        self.shape = (batch, views, joints)
        n = views * batch * (2 * joints * 3 + 3)
        self.host = torch.empty(n, dtype=torch.float32).pin_memory()
        self.dev = torch.empty(n, dtype=torch.float32, device=device)
        self._copied = None          # event behind the last host-to-device copy out of self.host

    def stage(self, poses, rays, centers):
        B, V, J = self.shape
        if self._copied is not None:
            self._copied.synchronize()      # the previous transfer has read the pinned buffer before it is overwritten
        b = poses[0].shape[0] if len(poses) else 0
        if len(poses) != V or len(rays) != V or len(centers) != V or not 0 < b <= B:
            raise RuntimeError("HostStager was built for %d views of at most %d poses" % (V, B))
        off, views = 0, ([], [], [])
        for k, (lst, shp) in enumerate(((poses, (b, J, 3)), (rays, (b, J, 3)), (centers, (b, 1, 3)))):
            n = shp[0] * shp[1] * shp[2]
            for t in lst:
                if tuple(t.shape) != shp:
                    raise RuntimeError("HostStager: expected a tensor of shape %s, got %s" % (shp, tuple(t.shape)))
                self.host[off:off + n].view(shp).copy_(t)
                views[k].append(self.dev[off:off + n].view(shp))
                off += n
        self.dev[:off].copy_(self.host[:off], non_blocking=True)
        self._copied = torch.cuda.Event()
        self._copied.record(torch.cuda.current_stream(self.dev.device))
        return views
