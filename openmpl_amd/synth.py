"""Multi-view model inputs synthesized from 3D poses on the device: what OpenMPL's synthetic datasets do per sample and view in
numpy inside Dataset.__getitem__, for a whole batch in one HIP kernel (csrc/synth.hip) through the C ABI; no CPU path.

Reference: lib/dataset/multiview_amass_h36m_mpl.py:317-342 (rotation about z, room translation), lib/utils/calib.py:42-77
(projection), lib/dataset/joints_dataset_mpl.py:592-613 (detection noise and confidence penalty), :701-727 (visibility under
NO_AUGMENTATION), :735-740 (missing joints), :762-774, :615-623, :872-904 (normalisation, rays, centres).  Random numbers are the
counter-based streams of detrng ("synth.rot", "synth.room", "synth.noise", "synth.missing"), indexed by the global pose index
first_index + b: a run cut into batches gets the values of the uncut run.  DESIGN.md section 7 states the contract.
"""
from __future__ import annotations

import ctypes as C
import functools
from collections import namedtuple
from typing import Optional, Sequence, Tuple

import torch

from . import cabi, detrng
from ._marshal import ptr, table, vec3, view_lists
from .inputs import check_distortion

SynthViews = namedtuple("SynthViews", "poses rays centers target pixels pixels_clean")


@functools.lru_cache(maxsize=64)
def _keys(seed):
    """the six stream keys of a seed, in the order of the key_* fields of mpl_synth_options"""
    return tuple(int(detrng._stream_key(seed, name, lane)) for name, lane in (("synth.rot", 0), ("synth.room", 0), ("synth.room", 1),
                                                                              ("synth.noise", 0), ("synth.noise", 1), ("synth.missing", 0)))


def _optional(t, shape, what, dev):
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != torch.float32:
        raise RuntimeError("%s must be float32 %s" % (what, "(" + ",".join(str(s) for s in shape) + ")"))
    if t.device != dev:
        raise RuntimeError("%s must live on the device of poses3d" % what)
    return t.contiguous()


def _check_scene(poses3d, cams, fn):
    if not isinstance(poses3d, torch.Tensor) or poses3d.device.type != "cuda":
        raise RuntimeError("%s has no CPU path: tensors must live on a GPU" % fn)
    if poses3d.ndim != 3 or poses3d.shape[-1] != 3 or poses3d.dtype != torch.float32 or poses3d.shape[0] < 1 or poses3d.shape[1] < 1:
        raise RuntimeError("poses3d must be float32 (B,J,3)")
    if not isinstance(cams, torch.Tensor) or cams.ndim != 2 or cams.shape[1] != 16 or cams.shape[0] < 1 or cams.dtype != torch.float64 \
            or cams.device != poses3d.device:
        raise RuntimeError("cams must be float64 (V,16) on the same device (see pack_cameras)")
    if cams.shape[0] > cabi.MPL_MAX_VIEWS:
        raise RuntimeError("at most %d views, got %d" % (cabi.MPL_MAX_VIEWS, cams.shape[0]))
    return poses3d.shape[0], cams.shape[0], poses3d.shape[1]


def synthesize_views(poses3d: torch.Tensor, cams: torch.Tensor, image_size: Tuple[float, float], *, seed: int = 0, first_index: int = 0,
                     rotate: bool = False, room: Optional[Sequence[float]] = None, noise_level: float = 0.0, penalize: str = "none",
                     penalize_a: float = 1.0, penalize_b: float = 0.0, clip: bool = True, missing_level: float = 0.0,
                     conf: Optional[torch.Tensor] = None, normalize_inputs: bool = True, normalize_cameras: bool = True,
                     target_scale=None, target_offset=None, rotation_deg: Optional[torch.Tensor] = None,
                     translation: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None,
                     missing_u: Optional[torch.Tensor] = None, return_pixels: bool = False,
                     distortion: Optional[torch.Tensor] = None) -> SynthViews:
    """poses3d (B,J,3) float32 GPU (world units), cams (V,16) float64 GPU (pack_cameras), image_size (w, h) in pixels.

    rotate: turn every pose about the world z axis by 360 * u degrees; room = (min_x, max_x, min_y, max_y): add
    (min_x + u (max_x - min_x), min_y + u' (max_y - min_y), 0); noise_level: standard deviation of the detection noise in pixels,
    with the confidence multiplied by penalize ("none", "exp_error": a exp(-b d), "linear": a d + b, "exp_sqrt": exp(-d / 2), d the
    length of the noise in pixels); clip: out-of-image joints are clamped to the border (True) or zeroed (False), confidence 0 in
    both; missing_level: the share of joints dropped (confidence and pixel 0); conf (B,V,J): detector confidences to start from
    (default 1).  rotation_deg (B), translation (B,3), noise (B,V,J,2) and missing_u (B,V,J) replace the stream of their step.
    target = (placed pose - target_offset) / target_scale per axis: with the same two vectors as scale / offset of
    PoseEvaluator.update the evaluator scores in world units.
    distortion (V,5) float64 (pack_distortion): the projection goes through the lens (project_point_radial,
    lib/multiviews/cameras.py:22-46); pixels_clean, the noise, the visibility step and the missing joints act on distorted pixels, as
    a detector sees them; the rays go through the undistorted pixels, exactly as prepare_inputs(distortion=) builds them.  Without
    it the launch and the bits are what they always were; zero coefficients agree with that to float64 rounding, not bitwise.

    Returns SynthViews(poses, rays, centers, target, pixels, pixels_clean): the first three are the lists of V tensors (B,J,3),
    (B,J,3), (B,1,3) that model(poses, rays=, centers=) takes; target (B,J,3); pixels (after the missing-joint step) and
    pixels_clean (the plain projection, the reference's joints_2d_org), both (B,V,J,2), or None unless return_pixels.
    Runs on the current stream and does not synchronise."""
    B, V, J = _check_scene(poses3d, cams, "synthesize_views")
    dev = poses3d.device
    distortion = check_distortion(distortion, V, dev)
    if penalize not in cabi.SYNTH_PENALIZE:
        raise RuntimeError("penalize must be one of %s, got %r" % (", ".join(sorted(cabi.SYNTH_PENALIZE)), penalize))
    w, h = float(image_size[0]), float(image_size[1])
    if not (w > 0 and h > 0):
        raise RuntimeError("image_size must be positive, got %r" % (tuple(image_size),))
    scale, offset = vec3(target_scale, 1.0, "target_scale takes 3 values"), vec3(target_offset, 0.0, "target_offset takes 3 values")
    if any(s == 0.0 or s != s for s in scale):
        raise RuntimeError("target_scale must not hold a zero")
    if room is not None:
        room = [float(x) for x in room]
        if len(room) != 4 or room[1] < room[0] or room[3] < room[2]:
            raise RuntimeError("room takes (min_x, max_x, min_y, max_y) with max >= min")
    if first_index < 0:
        raise RuntimeError("first_index must not be negative")
    conf = _optional(conf, (B, V, J), "conf", dev)
    rotation_deg = _optional(rotation_deg, (B,), "rotation_deg", dev)
    translation = _optional(translation, (B, 3), "translation", dev)
    noise = _optional(noise, (B, V, J, 2), "noise", dev)
    missing_u = _optional(missing_u, (B, V, J), "missing_u", dev)

    o = cabi.SynthOptions()
    o.penalize, o.clip, o.rotate, o.room = cabi.SYNTH_PENALIZE[penalize], int(bool(clip)), int(bool(rotate)), int(room is not None)
    o.normalize_inputs, o.normalize_cameras = int(bool(normalize_inputs)), int(bool(normalize_cameras))
    o.noise_level, o.missing_level, o.penalize_a, o.penalize_b = float(noise_level), float(missing_level), float(penalize_a), float(penalize_b)
    o.room_min_x, o.room_max_x, o.room_min_y, o.room_max_y = room if room is not None else (0.0, 0.0, 0.0, 0.0)
    o.img_w, o.img_h = w, h
    o.target_scale[:], o.target_offset[:] = scale, offset
    o.key_rot, o.key_room_x, o.key_room_y, o.key_noise0, o.key_noise1, o.key_missing = _keys(int(seed))
    o.first_index = int(first_index)

    poses3d, cams = poses3d.contiguous(), cams.contiguous()
    poses, rays, centers = view_lists(B, V, J, dev)
    target = torch.empty((B, J, 3), dtype=torch.float32, device=dev)
    pixels = torch.empty((B, V, J, 2), dtype=torch.float32, device=dev) if return_pixels else None
    clean = torch.empty((B, V, J, 2), dtype=torch.float32, device=dev) if return_pixels else None
    _launch(dev, distortion, poses3d.data_ptr(), cams.data_ptr(), C.byref(o), ptr(conf), ptr(rotation_deg), ptr(translation),
            ptr(noise), ptr(missing_u), B, V, J, table(poses), table(rays), table(centers), target.data_ptr(), ptr(pixels), ptr(clean), None)
    return SynthViews(poses, rays, centers, target, pixels, clean)


def _launch(dev, distortion, poses3d, cams, *rest):
    """mpl_synthesize_views, or with a distortion table its _ex form"""
    if distortion is None:
        cabi.launch("synthesize_views", dev, poses3d, cams, *rest)
    else:
        cabi.launch("synthesize_views_ex", dev, poses3d, cams, distortion.data_ptr(), *rest)


def project_points(points3d: torch.Tensor, cams: torch.Tensor, distortion: Optional[torch.Tensor] = None
                   ) -> Tuple[torch.Tensor, torch.Tensor]:
    """points3d (B,J,3) float32 GPU, cams (V,16) float64 GPU -> (pixels (B,V,J,2), depth (B,V,J)): x_cam = R (X - t),
    pixel = (fx x / z + cx, fy y / z + cy), depth = z.  The same launch as synthesize_views with every perturbation off: the
    reprojection that scores a predicted pose against detections.  A point at depth <= 1e-9 gets pixel (0,0).
    distortion (V,5) float64 (pack_distortion): the pixel is f y_d + c, y_d the lens polynomial of y = x_cam.xy / z -- the
    reference's project_pose (lib/multiviews/cameras.py:22-51)."""
    B, V, J = _check_scene(points3d, cams, "project_points")
    dev = points3d.device
    distortion = check_distortion(distortion, V, dev)
    o = cabi.SynthOptions()
    o.img_w = o.img_h = 1.0
    o.target_scale[:] = [1.0] * 3
    points3d, cams = points3d.contiguous(), cams.contiguous()
    pixels = torch.empty((B, V, J, 2), dtype=torch.float32, device=dev)
    depth = torch.empty((B, V, J), dtype=torch.float32, device=dev)
    _launch(dev, distortion, points3d.data_ptr(), cams.data_ptr(), C.byref(o), None, None, None, None, None, B, V, J, None, None,
            None, None, None, pixels.data_ptr(), depth.data_ptr())
    return pixels, depth
