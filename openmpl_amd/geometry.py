"""Multi-view geometry on the tensors the model call receives: triangulation of the rays and epipolar consistency of the detections.

Reference: lib/multiviews/triangulate.py (the triangulation baseline, on pymvg), lib/utils/calib.py:94-113
distance_between_two_skew_lines and :116-169 smart_pseudo_remove_weight (numpy, per sample, inside the datasets' __getitem__).
`rays` is a list of V (B,J,3) tensors, a world point on each joint's line of sight (joints_dataset_mpl.py:872-904), `centers` a list
of V (B,1,3) camera centres -- what prepare_inputs returns and `model(input, centers=centers, rays=rays)` takes.  `conf` is a list of
V tensors, each (B,J) or one of the model's own (B,J,3) pose tensors, whose channel 2 is read in place.  Two HIP kernels through the
C ABI (mpl_triangulate_rays, mpl_epipolar_errors, csrc/geometry.hip) on the current stream; no synchronisation, no CPU path.
triangulate_rays_robust (mpl_triangulate_robust, a third kernel) puts the view selection of lib/multiviews/triangulate.py:88-112
and a pair consensus in front of the same least-squares fit.  refine_points / reprojection_errors (mpl_refine_points,
csrc/refine.hip) work in the detector's unit: Levenberg-Marquardt on the reprojection error of a point in pixels, and that error for
any 3D estimate.  refine_poses (mpl_refine_poses, csrc/refine_poses.hip) refines the joints of a pose together, the same error plus
bone-length terms on the tree of rpsm.  refine_cameras (mpl_refine_cameras, csrc/refine_cameras.hip) is the transpose of
refine_points -- the points given, the camera poses moved --, and bundle_adjust alternates the two.  locate_cameras (mpl_locate_cameras, csrc/locate_cameras.hip) is the step before
them: a camera located from no pose at all by hypothesise-and-score over 6-point resections.  relative_pose (mpl_relative_pose,
csrc/relative_pose.hip) is the step before that one: the relative pose of two views from their detections and intrinsics alone, by
hypothesise-and-score over five-point solutions.  smooth_tracks (mpl_smooth_tracks, csrc/smooth_tracks.hip) works along the time
axis of a batch in frame order: every (sequence, joint) track smoothed, its gaps filled, its outlier frames held down.
"""
from __future__ import annotations

import math
import operator
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import cabi
from ._marshal import ptr, table


def _listed(lst, what, n=None):
    if not isinstance(lst, (list, tuple)) or len(lst) == 0 or not all(isinstance(t, torch.Tensor) for t in lst):
        raise RuntimeError("%s must be a non-empty list of tensors, one per view" % what)
    if n is not None and len(lst) != n:
        raise RuntimeError("%s holds %d tensors for %d views" % (what, len(lst), n))
    return list(lst)


def _lines(rays, centers, conf, weight=None):
    """Shapes first, then dtypes, then devices (so that each complaint names the argument it is about, with or without a GPU)
    -> contiguous float32 GPU tensors, the confidence stride and the sizes."""
    rays = _listed(rays, "rays")
    V = len(rays)
    if rays[0].ndim != 3 or rays[0].shape[2] != 3 or rays[0].shape[0] < 1 or rays[0].shape[1] < 1:
        raise RuntimeError("rays[0]: expected shape (B,J,3), got %s" % (tuple(rays[0].shape),))
    B, J, _ = rays[0].shape
    groups = [("rays", rays, (B, J, 3)), ("centers", _listed(centers, "centers", V), (B, 1, 3))]
    stride = 1
    if conf is not None:
        conf = _listed(conf, "conf", V)
        stride = 3 if conf[0].ndim == 3 else 1           # one of the model's pose tensors: x, y, confidence
        groups.append(("conf", conf, (B, J, 3) if stride == 3 else (B, J)))
    if weight is not None:
        groups.append(("weight", _listed(weight, "weight", V), (B, J)))
    for what, lst, shape in groups:
        for v, t in enumerate(lst):
            if tuple(t.shape) != shape:
                raise RuntimeError("%s[%d]: expected shape %s, got %s" % (what, v, shape, tuple(t.shape)))
    for what, lst, _ in groups:
        for v, t in enumerate(lst):
            if t.dtype != torch.float32:
                raise RuntimeError("float32 tensors required (%s[%d] is %s)" % (what, v, t.dtype))
    dev = rays[0].device
    for what, lst, _ in groups:
        for v, t in enumerate(lst):
            if t.device.type != "cuda":
                raise RuntimeError("the geometry kernels have no CPU path: %s[%d] must live on a GPU" % (what, v))
            if t.device != dev:
                raise RuntimeError("%s[%d] is on %s, rays[0] on %s" % (what, v, t.device, dev))
    if V > cabi.MPL_MAX_VIEWS or J > 64:
        raise NotImplementedError("at most %d views and 64 joints (got %d, %d)" % (cabi.MPL_MAX_VIEWS, V, J))
    out = [[t.contiguous() for t in lst] for _, lst, _ in groups]
    rays, centers = out[0], out[1]
    conf = out[2] if conf is not None else None
    weight = out[-1] if weight is not None else None
    return rays, centers, conf, weight, stride, B, V, J


def triangulate_rays(rays: Sequence[torch.Tensor], centers: Sequence[torch.Tensor], conf: Optional[Sequence[torch.Tensor]] = None
                     ) -> Tuple[torch.Tensor, torch.Tensor]:
    """The point closest to the V lines, weighted by the confidences: (points (B,J,3), residual (B,J)), residual the weighted
    root-mean-square distance of the point to its lines.  A view whose confidence is <= 0 or not finite does not take part; a
    joint with fewer than two views taking part, or with lines within about 2e-5 rad of parallel, is NaN in both outputs.
    `points` is what PoseEvaluator.update(points, target, ...) takes."""
    rays, centers, conf, _, stride, B, V, J = _lines(rays, centers, conf)
    dev = rays[0].device
    points = torch.empty((B, J, 3), dtype=torch.float32, device=dev)
    residual = torch.empty((B, J), dtype=torch.float32, device=dev)
    cabi.launch("triangulate_rays", dev, table(rays), table(centers), table(conf), stride, B, V, J, points.data_ptr(), residual.data_ptr())
    return points, residual


def triangulate_rays_robust(rays: Sequence[torch.Tensor], centers: Sequence[torch.Tensor],
                            conf: Optional[Sequence[torch.Tensor]] = None, threshold: Optional[float] = None,
                            conf_threshold: Optional[float] = None, min_inliers: int = 2
                            ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """triangulate_rays with the outliers taken out first: (points (B,J,3), residual (B,J), inliers (B,V,J) of 0 / 1; the layout
    of epipolar_errors, so inliers.unbind(1) is a conf or a weight list).  Per (sample, joint), in this order:

    1. candidates: the views that take part (conf > 0 and finite).  With `conf_threshold` (conf required) the reference's rule
       (triangulate.py:94-102) selects among all V confidences: th = conf_threshold; while at most one conf > th and th >= -1:
       th -= 0.05.  Two deviations: below th = 0 the reference would select zero-confidence views, here they stay out; and every
       joint starts at conf_threshold, where the reference hands a lowered threshold on to the later joints of the pose.
    2. consensus, with `threshold` (tau, world units): every candidate pair is a hypothesis, the midpoint of the common
       perpendicular of its two lines; the winner has the most candidates within tau, then the lowest sum of conf * min(dist^2,
       tau^2), then the lowest pair.  Its within-tau set is the inlier set; without `threshold` every candidate is an inlier.
    3. refit: the point and residual of triangulate_rays over the inlier set.

    Fewer than two candidates, no pair further than about 2e-5 rad from parallel, a winner with fewer than `min_inliers` views
    within tau, or a degenerate refit make the joint NaN in points and residual and its inliers all 0.  With threshold=None and
    conf_threshold=None this is triangulate_rays.  One launch, no synchronisation, identical bits from run to run and from
    batching to batching."""
    V = len(_listed(rays, "rays"))
    tau = cth = -1.0                                     # the C ABI's "off"
    if threshold is not None:
        tau = float(threshold)
        if not tau > 0.0:
            raise RuntimeError("threshold must be a positive distance in world units (got %r)" % (threshold,))
    if conf_threshold is not None:
        cth = float(conf_threshold)
        if cth != cth or cth > 64.0:
            raise RuntimeError("conf_threshold must be a number of at most 64 (got %r)" % (conf_threshold,))
        if conf is None:
            raise RuntimeError("conf_threshold needs conf")
    if int(min_inliers) != min_inliers or not 2 <= min_inliers <= V:
        raise RuntimeError("min_inliers must be an integer in [2, %d views] (got %r)" % (V, min_inliers))
    rays, centers, conf, _, stride, B, V, J = _lines(rays, centers, conf)
    dev = rays[0].device
    points = torch.empty((B, J, 3), dtype=torch.float32, device=dev)
    residual = torch.empty((B, J), dtype=torch.float32, device=dev)
    inliers = torch.empty((B, V, J), dtype=torch.float32, device=dev)
    cabi.launch("triangulate_robust", dev, table(rays), table(centers), table(conf), stride, B, V, J, tau, cth, int(min_inliers),
                points.data_ptr(), residual.data_ptr(), inliers.data_ptr())
    return points, residual, inliers


def triangulate_pixels(pixels: torch.Tensor, conf: Optional[torch.Tensor], cams: torch.Tensor,
                       image_size: Optional[Tuple[float, float]] = None, distortion: Optional[torch.Tensor] = None,
                       threshold: Optional[float] = None, conf_threshold: Optional[float] = None, refine: bool = False,
                       huber: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The call shape of the reference's triangulate_poses(camera_params, poses2d, confs) (lib/multiviews/triangulate.py:59-115) for
    a batch: pixels (B,V,J,2) float32 GPU, conf (B,V,J) or None, cams (V,16) float64 (pack_cameras), distortion (V,5) float64
    (pack_distortion) or None -> (points (B,J,3), residual (B,J), inliers (B,V,J)).

    A thin wrapper, no kernel of its own: prepare_inputs(pixels, conf, cams, image_size, False, False, distortion=) -- the rays go
    through the undistorted pixels, and a joint whose pixel is not invertible takes no part in that view -- then
    triangulate_rays_robust(rays, centers, poses as the confidences, threshold, conf_threshold), which with both stages off is
    triangulate_rays.  Without normalisation image_size is not looked at; it defaults to (1, 1).  Where the reference hands its
    coefficients to pymvg's OpenCV model, this inverts the model the projection uses (include/mpl_hip.h).

    refine=True adds a third launch: the returned `points` are those of refine_points(points, pixels, conf * inliers, cams,
    distortion, huber) -- the linear point moved to the minimum of its reprojection error in pixels over the inlier views (one torch
    multiply forms the weights; a NaN point stays NaN).  `residual` and `inliers` stay those of the linear stage.  `huber` (pixels)
    without `refine` raises.  With the default the call makes the two launches it always made and returns the same bits."""
    from .inputs import prepare_inputs
    if huber is not None and not refine:
        raise RuntimeError("huber is an option of the refinement: it needs refine=True")
    poses, rays, centers = prepare_inputs(pixels, conf, cams, (1.0, 1.0) if image_size is None else image_size, False, False,
                                          distortion=distortion)
    points, residual, inliers = triangulate_rays_robust(rays, centers, poses, threshold=threshold, conf_threshold=conf_threshold)
    if refine:
        weight = inliers if conf is None else conf.reshape(inliers.shape).to(torch.float32) * inliers
        points = refine_points(points, pixels, weight, cams, distortion=distortion, huber=huber).points
    return points, residual, inliers


class Refined(NamedTuple):
    """what refine_points returns"""
    points: torch.Tensor          # (B,J,3) float32
    error: torch.Tensor           # (B,J) float32: the weighted root-mean-square reprojection error, pixels
    errors: torch.Tensor          # (B,V,J) float32: |r_v| in pixels, NaN for a view that takes no part
    iterations: torch.Tensor      # (B,J) int32: trial steps made
    status: torch.Tensor          # (B,J) uint8: 0 converged, 1 capped, 2 passed through, 3 invalid


def _observations(points, pixels, conf, cams, distortion, with_points=True):
    """The argument checks of refine_points in the order of _lines: shapes first, then dtypes, then devices, each complaint naming
    its argument and raised before any device is touched; cams and distortion as prepare_inputs checks them.  with_points=False (the
    call that knows no points: relative_pose) leaves the points out of the checks and of the returned list."""
    from .inputs import check_distortion
    for what, t in ((("points", points),) if with_points else ()) + (("pixels", pixels),) + ((("conf", conf),) if conf is not None else ()):
        if not isinstance(t, torch.Tensor):
            raise RuntimeError("%s must be a tensor" % what)
    if pixels.ndim != 4 or pixels.shape[3] != 2 or min(pixels.shape[:3]) < 1:
        raise RuntimeError("pixels: expected shape (B,V,J,2), got %s" % (tuple(pixels.shape),))
    B, V, J, _ = pixels.shape
    groups = ([("points", points, (B, J, 3))] if with_points else []) + [("pixels", pixels, (B, V, J, 2))] + \
        ([("conf", conf, (B, V, J))] if conf is not None else [])
    for what, t, shape in groups:
        if tuple(t.shape) != shape:
            raise RuntimeError("%s: expected shape %s, got %s" % (what, shape, tuple(t.shape)))
    for what, t, _ in groups:
        if t.dtype != torch.float32:
            raise RuntimeError("float32 tensors required (%s is %s)" % (what, t.dtype))
    dev = pixels.device
    for what, t, _ in groups:
        if t.device.type != "cuda":
            raise RuntimeError("the geometry kernels have no CPU path: %s must live on a GPU" % what)
        if t.device != dev:
            raise RuntimeError("%s is on %s, pixels on %s" % (what, t.device, dev))
    if not isinstance(cams, torch.Tensor) or tuple(cams.shape) != (V, 16) or cams.dtype != torch.float64 or cams.device != dev:
        raise RuntimeError("cams must be float64 (V,16) on the same device (see pack_cameras)")
    distortion = check_distortion(distortion, V, dev)
    if V > cabi.MPL_MAX_VIEWS or J > 64 or B * V * J > 1 << 30:
        raise NotImplementedError("at most %d views, 64 joints and 2^30 observations (got %d, %d, %d)" % (cabi.MPL_MAX_VIEWS, V, J, B * V * J))
    return [t.contiguous() for _, t, _ in groups] + [None] * (conf is None), cams.contiguous(), distortion, B, V, J


def _refine(points, pixels, conf, cams, distortion, huber, max_iterations, step_tolerance):
    (points, pixels, conf), cams, distortion, B, V, J = _observations(points, pixels, conf, cams, distortion)
    dev = pixels.device
    out = Refined(torch.empty((B, J, 3), dtype=torch.float32, device=dev), torch.empty((B, J), dtype=torch.float32, device=dev),
                  torch.empty((B, V, J), dtype=torch.float32, device=dev), torch.empty((B, J), dtype=torch.int32, device=dev),
                  torch.empty((B, J), dtype=torch.uint8, device=dev))
    cabi.launch("refine_points", dev, points.data_ptr(), pixels.data_ptr(), ptr(conf), cams.data_ptr(), ptr(distortion), B, V, J, huber,
                max_iterations, step_tolerance, *(t.data_ptr() for t in out))
    return out


def refine_points(points: torch.Tensor, pixels: torch.Tensor, conf: Optional[torch.Tensor], cams: torch.Tensor,
                  distortion: Optional[torch.Tensor] = None, huber: Optional[float] = None, max_iterations: int = 20,
                  step_tolerance: float = 1e-8) -> Refined:
    """points (B,J,3) moved to the minimum of their reprojection error: E(X) = sum_v w_v rho(|proj_v(X) - pixels_v|^2) in pixels,
    by Levenberg-Marquardt from the given point.  pixels (B,V,J,2), conf (B,V,J) or None (the weights w), cams (V,16) float64,
    distortion (V,5) float64 or None: the arguments of triangulate_pixels, and the projection of project_points(distortion=).
    -> Refined(points, error, errors, iterations, status).

    A view takes part when its weight is finite and > 0 and its pixel is finite.  huber=None: rho(s) = s, least squares.
    huber=h (pixels): rho(s) = s up to h^2, 2 h sqrt(s) - h^2 beyond -- a detection far off pulls with a bounded force; the soft
    counterpart of the pair consensus of triangulate_rays_robust, in the detector's unit.  A trial step is accepted only if it
    lowers E, so E never rises; every trial counts in `iterations`, at most `max_iterations` (0 .. 1000).  Converged (status 0) when
    the step is <= step_tolerance times the depth of the nearest camera, else capped (1).  Passed through (2): fewer than two views
    take part or max_iterations == 0; the point is returned bit for bit.  Invalid (3): the point is not finite, no view takes part,
    or the point lies behind a camera that takes part; point, error and errors are NaN.  error (B,J) is the weighted
    root-mean-square of |r_v| in both modes, errors (B,V,J) the |r_v|, NaN where a view takes no part.  One launch, no
    synchronisation, identical bits from run to run and from batching to batching."""
    h, max_iterations, tol = _refine_options(huber, max_iterations, step_tolerance)
    return _refine(points, pixels, conf, cams, distortion, h, max_iterations, tol)


def reprojection_errors(points: torch.Tensor, pixels: torch.Tensor, conf: Optional[torch.Tensor], cams: torch.Tensor,
                        distortion: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The score of a 3D estimate in image units, which needs no ground truth: (errors (B,V,J), error (B,J)) of refine_points at
    the points as they are (the same launch with max_iterations=0).  points (B,J,3): triangulated points, rpsm poses, or the model's
    predictions after de-normalisation."""
    r = _refine(points, pixels, conf, cams, distortion, 0.0, 0, 0.0)
    return r.errors, r.error


class PosesRefined(NamedTuple):
    """what refine_poses returns"""
    points: torch.Tensor          # (B,J,3) float32
    error: torch.Tensor           # (B,J) float32: the weighted root-mean-square reprojection error per joint, pixels
    bone_error: torch.Tensor      # (B,J) float32: |X_j - X_parent(j)| - limb_length in world units; NaN at the root and dead bones
    cost0: torch.Tensor           # (B,) float64: E at the given pose, in the mode of the call
    cost: torch.Tensor            # (B,) float64: E at the final pose; never above cost0
    iterations: torch.Tensor      # (B,) int32: trial steps made
    status: torch.Tensor          # (B,) uint8: 0 converged, 1 capped, 2 passed through, 3 invalid


def _parents(parents, J):
    """`parents` as rpsm takes them -> a list of J ints that is one tree; the messages are those of rpsm"""
    from . import rpsm as _rpsm
    if parents is None:
        if J != len(_rpsm.HUMAN_BODY_PARENTS):
            raise ValueError("the default tree has %d joints, the points %d: pass parents" % (len(_rpsm.HUMAN_BODY_PARENTS), J))
        parents = _rpsm.HUMAN_BODY_PARENTS
    if isinstance(parents, torch.Tensor):
        if parents.device.type != "cpu":
            raise ValueError("parents is read on the host: pass a list or a CPU tensor")
        parents = parents.tolist()
    parents = [int(q) for q in parents]
    if len(parents) != J:
        raise ValueError("parents has %d entries, the points %d joints" % (len(parents), J))
    _rpsm.tree_levels(parents)
    return parents


def bone_lengths(points: torch.Tensor, parents: Optional[Sequence[int]] = None) -> torch.Tensor:
    """Plumbing, plain torch, no kernel: points (B,J,3) -> (B,J) float32, |X_j - X_parent(j)| and 0 at the root; NaN where an end is
    NaN.  What feeds refine_poses' limb_length, for instance bone_lengths(p).nanmedian(0).values over the poses of a sequence.
    parents: as refine_poses takes them (default: the 17-joint HumanBody tree)."""
    if not isinstance(points, torch.Tensor) or points.ndim != 3 or points.shape[2] != 3:
        raise RuntimeError("points: expected a tensor of shape (B,J,3), got %s"
                           % (tuple(points.shape) if isinstance(points, torch.Tensor) else type(points).__name__,))
    J = points.shape[1]
    parents = _parents(parents, J)
    idx = torch.tensor([q if q >= 0 else j for j, q in enumerate(parents)], dtype=torch.long, device=points.device)
    return (points - points.index_select(1, idx)).to(torch.float32).norm(dim=-1)


def refine_poses(points: torch.Tensor, pixels: torch.Tensor, conf: Optional[torch.Tensor], cams: torch.Tensor, limb_length: torch.Tensor,
                 *, parents: Optional[Sequence[int]] = None, bone_weight: float = 1e4, distortion: Optional[torch.Tensor] = None,
                 huber: Optional[float] = None, max_iterations: int = 50, step_tolerance: float = 1e-8) -> PosesRefined:
    """Whole poses moved to the minimum of reprojection error plus bone-length error: the continuous counterpart of rpsm, and the
    polish of any 3D estimate (triangulated, from rpsm, or the model's prediction) against the pixels.  Per pose,

        E(X) = sum_{v,j} w_vj rho(|proj_v(X_j) - pixels_vj|^2) + bone_weight * sum_{bones j} ((|X_j - X_parent(j)| - L_j) / L_j)^2

    by Levenberg-Marquardt over the joints of the pose at once, from the given pose.  points (B,J,3), pixels (B,V,J,2), conf (B,V,J) or
    None, cams (V,16) float64, distortion (V,5) float64 or None, huber, max_iterations (0 .. 1000), step_tolerance: the arguments,
    checks and limits of refine_points, and the first sum is its cost to the letter (px^2).  limb_length: float32 (J,) or (B,J) on
    the device, indexed by the child joint; the root's entry is not read (bone_lengths makes one from poses).  parents: J ints, -1
    for the one root, read on the host; default the 17-joint HumanBody tree of rpsm when J = 17, otherwise required; anything but
    one tree is a ValueError before anything is launched.  bone_weight: finite, >= 0; the bone residual is relative, so the weight is
    px^2 per unit of relative length error whatever the world unit, and the default 1e4 is (2 px / 2 %)^2.  The bone term is always
    quadratic.  -> PosesRefined(points, error, bone_error, cost0, cost, iterations, status).

    A bone is live when both its ends have a finite given point and a view that takes part, and its length is finite and > 0: a NaN
    length switches a bone off.  A joint takes part when its given point is finite and it is seen by two views that take part, or by
    one and is an end of a live bone -- which is what makes occluded joints and two-camera rigs usable.  A joint that takes no part
    is returned bit for bit with error NaN.  A trial is accepted only if it lowers E and leaves every joint that takes part in front
    of its cameras, so cost <= cost0.  Status per pose: converged (0) when the step is <= step_tolerance times the smallest depth of
    the pose; capped (1); passed through (2): max_iterations == 0 or no joint takes part, points bit for bit, everything scored;
    invalid (3): a joint that takes part is behind one of its cameras at the given pose, every output of the pose NaN.  error (B,J):
    the plain weighted RMS of |r_v| per joint as in refine_points; bone_error (B,J): |d| - L at the result, NaN at the root and at
    bones that are not live.  What stays underdetermined stays so and may end capped: a whole pose seen by one camera (its depth is
    held by nothing but the lengths), a leaf seen by one view (one ray and one bone leave a near and a far solution; the start
    decides).  One launch (one wave per pose), no synchronisation, identical bits from run to run and from batching to batching."""
    h, max_iterations, tol = _refine_options(huber, max_iterations, step_tolerance)
    try:
        bw = float(bone_weight)
    except (TypeError, ValueError):
        bw = float("nan")
    if not (bw >= 0.0 and math.isfinite(bw)):
        raise RuntimeError("bone_weight must be a finite number >= 0 (got %r)" % (bone_weight,))
    if isinstance(pixels, torch.Tensor) and pixels.ndim == 4 and min(pixels.shape[:3]) >= 1:
        # a pixels tensor of another form is _observations' to complain about
        B, J = pixels.shape[0], pixels.shape[2]
        parents = _parents(parents, J)
        if not isinstance(limb_length, torch.Tensor) or tuple(limb_length.shape) not in ((J,), (B, J)):
            raise RuntimeError("limb_length: expected a tensor of shape %s or %s, got %s"
                               % ((J,), (B, J), tuple(limb_length.shape) if isinstance(limb_length, torch.Tensor) else type(limb_length).__name__))
        if limb_length.dtype != torch.float32:
            raise RuntimeError("float32 tensors required (limb_length is %s)" % limb_length.dtype)
    (points, pixels, conf), cams, distortion, B, V, J = _observations(points, pixels, conf, cams, distortion)
    dev = pixels.device
    if limb_length.device != dev:
        raise RuntimeError("limb_length is on %s, pixels on %s" % (limb_length.device, dev))
    limb_length = limb_length.contiguous()
    out = PosesRefined(torch.empty((B, J, 3), dtype=torch.float32, device=dev), torch.empty((B, J), dtype=torch.float32, device=dev),
                       torch.empty((B, J), dtype=torch.float32, device=dev), torch.empty((B,), dtype=torch.float64, device=dev),
                       torch.empty((B,), dtype=torch.float64, device=dev), torch.empty((B,), dtype=torch.int32, device=dev),
                       torch.empty((B,), dtype=torch.uint8, device=dev))
    cabi.launch("refine_poses", dev, points.data_ptr(), pixels.data_ptr(), ptr(conf), cams.data_ptr(), ptr(distortion),
                limb_length.data_ptr(), J if limb_length.ndim == 2 else 0, (cabi.C.c_int * J)(*parents), B, V, J, h, bw, max_iterations, tol,
                *(t.data_ptr() for t in out))
    return out


class TracksSmoothed(NamedTuple):
    """what smooth_tracks returns"""
    points: torch.Tensor          # (T,J,3) float32: the minimiser, gaps filled
    residual: torch.Tensor        # (T,J) float32: |X_t - Y_t|, NaN at gaps
    irls_weight: torch.Tensor     # (T,J) float32: min(1, huber / residual) at the result; 1 in the plain mode, 0 at gaps
    cost0: torch.Tensor           # (S,J) float64: E after the first solve, in the mode of the call
    cost: torch.Tensor            # (S,J) float64: E at the result; never above cost0
    iterations: torch.Tensor      # (S,J) int32: solves made
    status: torch.Tensor          # (S,J) uint8: 0 converged, 1 capped, 2 passed through
    points64: Optional[torch.Tensor] = None      # (T,J,3) float64 with return_float64=True: the points before their rounding


def _segments(segments, T):
    """`segments` -> a list of positive ints that sum to T and stay inside the kernel's limits; default one segment"""
    if segments is None:
        segments = (T,)
    if isinstance(segments, torch.Tensor):
        if segments.device.type != "cpu":
            raise ValueError("segments is read on the host: pass a sequence of ints or a CPU tensor")
        segments = segments.tolist()
    try:
        seg = [operator.index(n) for n in segments]
    except TypeError:
        raise ValueError("segments must be a sequence of ints (got %r)" % (segments,)) from None
    if not seg or min(seg) < 1:
        raise ValueError("segments must be positive frame counts (got %r)" % (segments,))
    if sum(seg) != T:
        raise ValueError("segments sum to %d, the points have %d frames" % (sum(seg), T))
    if max(seg) > cabi.SMOOTH_MAX_SEGMENT:
        raise ValueError("a segment of %d frames: at most %d" % (max(seg), cabi.SMOOTH_MAX_SEGMENT))
    return seg


def smooth_tracks(points: torch.Tensor, weight: Optional[torch.Tensor] = None, *, segments: Optional[Sequence[int]] = None,
                  smoothness: float, order: int = 2, huber: Optional[float] = None, max_iterations: int = 20,
                  step_tolerance: float = 1e-6, return_float64: bool = False, _single_lane: bool = False) -> TracksSmoothed:
    """Pose tracks smoothed along time on the device: jitter taken out, gaps filled, single outlier frames held down.  points
    (T,J,3) float32: the poses of one or several sequences frame after frame -- what refine_points(...).points,
    refine_poses(...).points, triangulate_*, rpsm or the model return for a batch in frame order.  weight (T,J) float32 or None (all
    ones): a confidence, 1 / error**2 of refine_points, a status < 3 mask.  A frame of a joint takes part when its coordinates are
    finite and its weight is finite and > 0; everything else is a gap.  segments: the frame counts of the sequences, positive ints
    that sum to T (default (T,)), read on the host; no term crosses a boundary.  Per track (segment, joint) the minimiser of

        E(X) = sum_{t takes part} w_t rho(|X_t - Y_t|^2) + smoothness * sum_t |D^order X|_t^2

    D^1 X_t = X_t+1 - X_t, D^2 X_t = X_t+1 - 2 X_t + X_t-1 inside the segment; rho(s) = s, or with huber = h (world units, on the 3D
    distance) s up to h^2 and 2 h sqrt(s) - h^2 beyond.  smoothness: finite, > 0; order: 1 or 2; a huber that is None, <= 0 or not
    finite is the plain mode, as the C ABI reads it; max_iterations (0 .. 1000) and step_tolerance as refine_points checks them.
    Plain mode: one solve.  Huber mode: iteratively reweighted least squares,
    w' = w min(1, h / |X - Y|) from the previous iterate, until the largest coordinate step is <= step_tolerance times the extent of
    the track (its largest coordinate spread over the frames that take part) or the cost stops falling (the earlier iterate is
    kept); cost0 is E after the first solve, so cost <= cost0.  -> TracksSmoothed(points, residual, irls_weight, cost0, cost,
    iterations, status): every frame of every track is written.  Gaps get the minimiser's value: interpolated linearly (order 1) or
    by a cubic (order 2), and continued as a constant or a straight line before the first and after the last frame that takes part.
    irls_weight is the call's outlier report.  status per track: 0 converged, 1 capped at max_iterations, 2 passed through
    (max_iterations == 0, or fewer than `order` frames take part: the points bit for bit, residual 0 where a frame takes part, costs
    0); 3 is never written.  return_float64=True adds points64, the points before their rounding.  One launch, one wave per track,
    the time axis split among its lanes; no synchronisation; identical bits from run to run, and a track's bits do not depend on
    which other segments and joints share the call."""
    _, max_iterations, tol = _refine_options(None, max_iterations, step_tolerance)
    h = 0.0 if huber is None else float(huber)
    h = h if (h > 0.0 and math.isfinite(h)) else 0.0           # <= 0, NaN, inf: the plain mode, as the C ABI reads it
    try:
        lam = float(smoothness)
    except (TypeError, ValueError):
        lam = float("nan")
    if not (lam > 0.0 and math.isfinite(lam)):
        raise RuntimeError("smoothness must be a finite number > 0 (got %r)" % (smoothness,))
    if order not in (1, 2):
        raise RuntimeError("order must be 1 or 2 (got %r)" % (order,))
    if not isinstance(points, torch.Tensor):
        raise RuntimeError("points must be a tensor")
    if points.ndim != 3 or points.shape[2] != 3 or min(points.shape[:2]) < 1:
        raise RuntimeError("points: expected shape (T,J,3), got %s" % (tuple(points.shape),))
    T, J = points.shape[:2]
    if weight is not None:
        if not isinstance(weight, torch.Tensor):
            raise RuntimeError("weight must be a tensor")
        if tuple(weight.shape) != (T, J):
            raise RuntimeError("weight: expected shape %s, got %s" % ((T, J), tuple(weight.shape)))
    if T > cabi.SMOOTH_MAX_FRAMES or J > cabi.SMOOTH_MAX_JOINTS:
        raise RuntimeError("points of shape %s: at most %d frames and %d joints" % (tuple(points.shape), cabi.SMOOTH_MAX_FRAMES, cabi.SMOOTH_MAX_JOINTS))
    seg = _segments(segments, T)
    for what, t in (("points", points), ("weight", weight)):
        if t is not None and t.dtype != torch.float32:
            raise RuntimeError("float32 tensors required (%s is %s)" % (what, t.dtype))
    if points.device.type != "cuda":
        raise RuntimeError("points must be on the GPU (got %s)" % points.device)
    dev = points.device
    if weight is not None and weight.device != dev:
        raise RuntimeError("weight is on %s, points on %s" % (weight.device, dev))
    points = points.contiguous()
    weight = None if weight is None else weight.contiguous()
    S = len(seg)
    offsets = [0]
    for n in seg:
        offsets.append(offsets[-1] + n)
    table = torch.empty((S + 1,), dtype=torch.int32, device=dev)
    table.copy_(torch.tensor(offsets, dtype=torch.int32), non_blocking=False)
    ws = torch.empty((cabi.load().mpl_smooth_tracks_workspace_bytes(T, J, S),), dtype=torch.uint8, device=dev)
    f32, f64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.float64, device=dev)
    out = TracksSmoothed(torch.empty((T, J, 3), **f32), torch.empty((T, J), **f32), torch.empty((T, J), **f32), torch.empty((S, J), **f64),
                         torch.empty((S, J), **f64), torch.empty((S, J), dtype=torch.int32, device=dev),
                         torch.empty((S, J), dtype=torch.uint8, device=dev), torch.empty((T, J, 3), **f64) if return_float64 else None)
    cabi.launch("smooth_tracks", dev, points.data_ptr(), ptr(weight), (cabi.C.c_int * S)(*seg), table.data_ptr(), S, T, J, lam, order, h,
                max_iterations, tol, cabi.SMOOTH_F_SINGLE_LANE if _single_lane else 0, ws.data_ptr(), ws.numel(),
                *(t.data_ptr() for t in out[:7]), ptr(out.points64))
    return out


class CamerasRefined(NamedTuple):
    """what refine_cameras returns"""
    cams: torch.Tensor            # (V,16) float64: the records with the refined poses, intrinsics as given
    error: torch.Tensor           # (V,) float64: the weighted root-mean-square reprojection error at the final pose, pixels
    cost0: torch.Tensor           # (V,) float64: E at the given pose, in the mode of the call
    cost: torch.Tensor            # (V,) float64: E at the final pose; never above cost0
    used: torch.Tensor            # (V,) int32: observations that take part
    iterations: torch.Tensor      # (V,) int32: trial steps made
    status: torch.Tensor          # (V,) uint8: 0 converged, 1 capped, 2 passed through, 3 invalid


class BundleAdjusted(NamedTuple):
    """what bundle_adjust returns"""
    points: torch.Tensor          # (B,J,3) float32
    cams: torch.Tensor            # (V,16) float64
    cost: torch.Tensor            # (rounds+1,) float64: the total cost before every round, and after the last
    cameras: Optional[CamerasRefined]    # the last round's refine_cameras; None with rounds=0
    refined: Optional[Refined]           # the last round's refine_points; None with rounds=0


def _refine_options(huber, max_iterations, step_tolerance):
    """the value checks refine_points makes -> (h, max_iterations, tol) as the C ABI takes them"""
    h = 0.0                                              # the C ABI's "plain"
    if huber is not None:
        h = float(huber)
        if not (h > 0.0 and math.isfinite(h)):
            raise RuntimeError("huber must be a positive finite number of pixels (got %r)" % (huber,))
    if int(max_iterations) != max_iterations or not 0 <= max_iterations <= 1000:
        raise RuntimeError("max_iterations must be an integer in [0, 1000] (got %r)" % (max_iterations,))
    tol = float(step_tolerance)
    if not (tol >= 0.0 and math.isfinite(tol)):
        raise RuntimeError("step_tolerance must be a finite number >= 0 (got %r)" % (step_tolerance,))
    return h, int(max_iterations), tol


def _fixed_mask(fixed, V):
    """`fixed`, an iterable of view indices in 0 .. V-1 -> the C ABI's bit mask"""
    try:
        fixed = list(fixed)
    except TypeError:
        raise RuntimeError("fixed must be a sequence of view indices (got %r)" % (fixed,))
    mask = 0
    for v in fixed:
        try:
            i = -1 if isinstance(v, bool) else operator.index(v)      # Python and numpy integers; no bools, floats or strings
        except TypeError:
            i = -1
        if not 0 <= i < V:
            raise RuntimeError("fixed holds view indices, integers in [0, %d] (got %r)" % (V - 1, v))
        mask |= 1 << i
    return mask


def _refine_cameras(points, pixels, conf, cams, distortion, h, max_iterations, tol, mask):
    (points, pixels, conf), cams, distortion, B, V, J = _observations(points, pixels, conf, cams, distortion)
    dev = pixels.device
    out = CamerasRefined(torch.empty((V, 16), dtype=torch.float64, device=dev), torch.empty((V,), dtype=torch.float64, device=dev),
                         torch.empty((V,), dtype=torch.float64, device=dev), torch.empty((V,), dtype=torch.float64, device=dev),
                         torch.empty((V,), dtype=torch.int32, device=dev), torch.empty((V,), dtype=torch.int32, device=dev),
                         torch.empty((V,), dtype=torch.uint8, device=dev))
    cabi.launch("refine_cameras", dev, points.data_ptr(), pixels.data_ptr(), ptr(conf), cams.data_ptr(), ptr(distortion), B, V, J, h,
                max_iterations, tol, mask, *(t.data_ptr() for t in out))
    return out


def refine_cameras(points: torch.Tensor, pixels: torch.Tensor, conf: Optional[torch.Tensor], cams: torch.Tensor,
                   distortion: Optional[torch.Tensor] = None, huber: Optional[float] = None, max_iterations: int = 20,
                   step_tolerance: float = 1e-8, fixed: Sequence[int] = ()) -> CamerasRefined:
    """The transpose of refine_points: the points (B,J,3) are given and the camera poses move.  Per view v,
    E_v(R, t) = sum_{b,j} w_bvj rho(|proj_v(X_bj) - pixels_bvj|^2) is minimised over the rotation and the centre of the camera by
    Levenberg-Marquardt from the given pose; the arguments, the projection, the lens, the weights and `huber` are those of
    refine_points, and the intrinsics and the lens coefficients stay as given.  -> CamerasRefined(cams, error, cost0, cost, used,
    iterations, status), one entry per view.

    An observation takes part when its weight is finite and > 0, its pixel is finite and its point is finite (NaN joints of a
    triangulation drop out); `used` counts them.  A trial pose is R' = exp([w]x) R, t' = t + dt; it is accepted only if it lowers E
    and leaves every participating point in front of the camera, so cost <= cost0.  Converged (status 0) when |w| <=
    step_tolerance and |dt| <= step_tolerance times the depth of the nearest participating point, else capped (1) after
    `max_iterations` trials (0 .. 1000).  Passed through (2): the view is in `fixed`, max_iterations == 0 or fewer than 3
    observations take part; its record is returned bit for bit, error and costs are computed.  Invalid (3): no observation takes
    part, the record is not finite, or a participating point is not in front of the given camera; the record is returned as given,
    error and costs are NaN.  `error` is the plain weighted root-mean-square of |r| in pixels in both modes.  A fit needs
    observations: with 68 or more and 2 px of noise the centre comes back to 1e-3 .. 2e-2 scene units, with 17 the fit follows the
    noise.  A given R that is not orthonormal stays so -- the steps are rotations --; cleaning such a table is the caller's.
    One launch (one workgroup per view), no synchronisation, identical bits from run to run."""
    h, max_iterations, tol = _refine_options(huber, max_iterations, step_tolerance)
    V = pixels.shape[1] if isinstance(pixels, torch.Tensor) and pixels.ndim == 4 else 0
    mask = _fixed_mask(fixed, V) if V else 0             # a pixels tensor of another form is _observations' to complain about
    return _refine_cameras(points, pixels, conf, cams, distortion, h, max_iterations, tol, mask)


def _consensus_options(huber, refine, threshold, hypotheses, seed):
    """The options locate_cameras and relative_pose share -> (h, tau, H, seed): `huber` as _refine_options has it and only with
    `refine`, a positive finite threshold in pixels, 1 .. 65536 hypotheses, an integer seed"""
    if huber is not None and not refine:
        raise RuntimeError("huber is an option of the refinement: it needs refine=True")
    h = _refine_options(huber, 20, 1e-8)[0]
    try:
        tau = float(threshold)
    except (TypeError, ValueError):
        tau = math.nan
    if not (tau > 0.0 and math.isfinite(tau)):
        raise RuntimeError("threshold must be a positive finite number of pixels (got %r)" % (threshold,))
    try:
        H = -1 if isinstance(hypotheses, bool) else operator.index(hypotheses)
    except TypeError:
        H = -1
    if not 1 <= H <= 65536:
        raise RuntimeError("hypotheses must be an integer in [1, 65536] (got %r)" % (hypotheses,))
    try:
        seed = -1 if isinstance(seed, bool) else operator.index(seed)
    except TypeError:
        raise RuntimeError("seed must be an integer (got %r)" % (seed,))
    return h, tau, H, seed


class CamerasLocated(NamedTuple):
    """what locate_cameras returns"""
    cams: torch.Tensor            # (V,16) float64: the records with the located (refine=True: polished) poses, intrinsics as given
    inliers: torch.Tensor         # (B,V,J) float32, 0 / 1: the observations within the threshold of the winning hypothesis
    count: torch.Tensor           # (V,) int32: how many
    best: torch.Tensor            # (V,) int32: the winning hypothesis, -1 where there is none
    error: torch.Tensor           # (V,) float64: the plain root-mean-square of |r| over the inliers, pixels
    status: torch.Tensor          # (V,) uint8: 0 located, 2 passed through, 3 invalid
    refined: Optional[CamerasRefined]    # the polish; None without refine=True
    poses: Optional[torch.Tensor]        # (V,H,12) float64: R row-major, then the centre; None without return_hypotheses=True
    scores: Optional[torch.Tensor]       # (V,H,2) float64: count, cost


def locate_cameras(points: torch.Tensor, pixels: torch.Tensor, conf: Optional[torch.Tensor], cams: torch.Tensor,
                   distortion: Optional[torch.Tensor] = None, threshold: float = 6.0, hypotheses: int = 1024, seed: int = 0,
                   fixed: Sequence[int] = (), refine: bool = False, huber: Optional[float] = None,
                   return_hypotheses: bool = False) -> CamerasLocated:
    """Cameras located from scratch: the step from no pose at all into the basin of refine_cameras, in the presence of wrong
    detections.  points (B,J,3), pixels (B,V,J,2), conf (B,V,J) or None, cams (V,16) float64 and distortion (V,5) or None are the
    arguments of refine_cameras, but of a view's record only fx fy cx cy and its lens row are read: the pose fields of a view that
    is not in `fixed` are not looked at and may be NaN.  -> CamerasLocated(cams, inliers, count, best, error, status, refined,
    poses, scores), one entry per view.

    Per view, `hypotheses` (1 .. 65536) poses are formed, each the 6-point DLT of six participating observations drawn with the
    counter-based generator of synthesize_views under `seed`, and each is scored over all participating observations by its
    reprojection error in pixels, lens included: count = the observations within `threshold` (pixels, finite and > 0), cost = sum w
    min(|r|^2, threshold^2).  The winner has the most inliers, then the lowest cost, then the lowest number (include/mpl_hip.h has
    the six steps).  An observation takes part as in refine_cameras, and its pixel has to go back through the lens.

    Located (status 0): the record carries the winner's pose.  Passed through (2): the view is in `fixed`; its record is returned
    bit for bit, inliers, count and error are those of the given pose.  Invalid (3): fewer than 6 observations take part, no
    hypothesis is valid, the winner has fewer than 6 inliers or the intrinsics are not finite; the record is returned as given, error
    is NaN, count 0 and the inliers 0.  A winner is a start, not a fit: from 136 observations with 2 px of noise and a quarter of
    them planted 40 to 120 px off it lies within a few degrees and tenths of a unit.  refine=True adds one launch, the polish:
    refine_cameras(points, pixels, conf * inliers (inliers with conf=None), cams, distortion, huber=huber, fixed=fixed), whose
    records become `cams` and which is returned whole as `refined`; inliers, count, best and error stay those of the hypothesis
    stage.  `huber` without `refine` raises.  Below about 68 observations of a view the result follows the noise, as that of
    refine_cameras does.  return_hypotheses=True hands out every hypothesis: poses (V,H,12), NaN where void, and scores (V,H,2),
    (0, inf) where void.

    The recipe for a rig of which two cameras are calibrated: triangulate_pixels with those two views -> locate_cameras(fixed=(0, 1),
    refine=True) -> bundle_adjust(fixed=(0, 1)).  Three launches before the polish, no synchronisation, nothing read back, identical
    bits from run to run."""
    from . import detrng
    h, tau, H, seed = _consensus_options(huber, refine, threshold, hypotheses, seed)
    V = pixels.shape[1] if isinstance(pixels, torch.Tensor) and pixels.ndim == 4 else 0
    mask = _fixed_mask(fixed, V) if V else 0             # a pixels tensor of another form is _observations' to complain about
    (points, pixels, conf), cams, distortion, B, V, J = _observations(points, pixels, conf, cams, distortion)
    dev = pixels.device
    keys = (cabi.C.c_uint64 * V)(*(int(detrng._stream_key(seed, "locate_cameras", lane=v)) for v in range(V)))
    ws = torch.empty((cabi.load().mpl_locate_cameras_workspace_bytes(B, V, J),), dtype=torch.uint8, device=dev)
    out_cams = torch.empty((V, 16), dtype=torch.float64, device=dev)
    inliers = torch.empty((B, V, J), dtype=torch.float32, device=dev)
    count = torch.empty((V,), dtype=torch.int32, device=dev)
    best = torch.empty((V,), dtype=torch.int32, device=dev)
    error = torch.empty((V,), dtype=torch.float64, device=dev)
    status = torch.empty((V,), dtype=torch.uint8, device=dev)
    poses = torch.empty((V, H, 12), dtype=torch.float64, device=dev)
    scores = torch.empty((V, H, 2), dtype=torch.float64, device=dev)
    cabi.launch("locate_cameras", dev, points.data_ptr(), pixels.data_ptr(), ptr(conf), cams.data_ptr(), ptr(distortion), B, V, J, tau, H,
                keys, mask, ws.data_ptr(), ws.numel(), out_cams.data_ptr(), inliers.data_ptr(), count.data_ptr(), best.data_ptr(),
                error.data_ptr(), status.data_ptr(), poses.data_ptr(), scores.data_ptr())
    refined = None
    if refine:
        refined = _refine_cameras(points, pixels, inliers if conf is None else conf * inliers, out_cams, distortion, h, 20, 1e-8, mask)
        out_cams = refined.cams
    return CamerasLocated(out_cams, inliers, count, best, error, status, refined, poses if return_hypotheses else None,
                          scores if return_hypotheses else None)


class RelativeRefined(NamedTuple):
    """what refine_relative_pose returns"""
    rotation: torch.Tensor        # (P,3,3) float64
    direction: torch.Tensor       # (P,3) float64, of unit length
    cams: torch.Tensor            # (P,2,16) float64: the two records of relative_pose under the final pose
    error: torch.Tensor           # (P,) float64: the weighted root-mean-square Sampson distance at the final pose, pixels
    cost0: torch.Tensor           # (P,) float64: E at the given pose, in the mode of the call
    cost: torch.Tensor            # (P,) float64: E at the final pose; never above cost0
    used: torch.Tensor            # (P,) int32: correspondences that take part
    iterations: torch.Tensor      # (P,) int32: trial steps made
    status: torch.Tensor          # (P,) uint8: 0 converged, 1 capped, 2 passed through, 3 invalid


class RelativePose(NamedTuple):
    """what relative_pose returns"""
    rotation: torch.Tensor        # (P,3,3) float64: R of x_b = R x_a + t, NaN where the pair is invalid
    direction: torch.Tensor       # (P,3) float64: t, of unit length
    cams: torch.Tensor            # (P,2,16) float64: view a as the gauge (R = I, centre 0), view b at -baseline R^T t; intrinsics as given
    inliers: torch.Tensor         # (B,P,J) float32, 0 / 1: the correspondences within the threshold of the winning hypothesis
    count: torch.Tensor           # (P,) int32: how many
    best: torch.Tensor            # (P,) int32: the winning hypothesis, -1 where there is none
    error: torch.Tensor           # (P,) float64: the root-mean-square Sampson distance over the inliers, pixels
    status: torch.Tensor          # (P,) uint8: 0 located, 3 invalid
    refined: Optional["RelativeRefined"]     # the polish; None without refine=True
    poses: Optional[torch.Tensor]        # (P,H,12) float64: R row-major, then t; None without return_hypotheses=True
    scores: Optional[torch.Tensor]       # (P,H,2) float64: count, cost
    roots: Optional[torch.Tensor]        # (P,H) int32: the real candidates of every hypothesis


def _pairs(pairs, V):
    """`pairs`, a sequence of (a, b) with a != b view indices in 0 .. V-1 -> a flat list of ints"""
    try:
        pairs = [tuple(p) for p in pairs]
    except TypeError:
        raise RuntimeError("pairs must be a sequence of (a, b) view indices (got %r)" % (pairs,))
    if not 1 <= len(pairs) <= cabi.MPL_MAX_VIEWS:
        raise RuntimeError("between 1 and %d pairs (got %d)" % (cabi.MPL_MAX_VIEWS, len(pairs)))
    flat = []
    for p in pairs:
        idx = []
        for v in p:
            try:
                idx.append(-1 if isinstance(v, bool) else operator.index(v))
            except TypeError:
                idx.append(-1)
        if len(idx) != 2 or not all(0 <= i < V for i in idx) or idx[0] == idx[1]:
            raise RuntimeError("pairs holds two distinct view indices, integers in [0, %d] (got %r)" % (V - 1, p))
        flat += idx
    return flat


def _baseline(baseline):
    try:
        base = float(baseline)
    except (TypeError, ValueError):
        base = math.nan
    if not (base > 0.0 and math.isfinite(base)):
        raise RuntimeError("baseline must be a positive finite length (got %r)" % (baseline,))
    return base


def _refine_relative(pixels, conf, weight, cams, flat, rotation, direction, distortion, h, max_iterations, tol, base):
    (pixels, conf), cams, distortion, B, V, J = _observations(None, pixels, conf, cams, distortion, with_points=False)
    dev = pixels.device
    P = len(flat) // 2
    for what, t, shape, dt in (("rotation", rotation, (P, 3, 3), torch.float64), ("direction", direction, (P, 3), torch.float64)) + \
            ((("weight", weight, (B, P, J), torch.float32),) if weight is not None else ()):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != dt or t.device != dev:
            raise RuntimeError("%s must be %s %s on the device of pixels" % (what, str(dt).replace("torch.", ""), shape))
    f64 = dict(dtype=torch.float64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    out = RelativeRefined(torch.empty((P, 3, 3), **f64), torch.empty((P, 3), **f64), torch.empty((P, 2, 16), **f64), torch.empty((P,), **f64),
                          torch.empty((P,), **f64), torch.empty((P,), **f64), torch.empty((P,), **i32), torch.empty((P,), **i32),
                          torch.empty((P,), dtype=torch.uint8, device=dev))
    cabi.launch("refine_relative_pose", dev, pixels.data_ptr(), ptr(conf), ptr(None if weight is None else weight.contiguous()),
                cams.data_ptr(), ptr(distortion), B, V, J, (cabi.C.c_int * len(flat))(*flat), P, rotation.contiguous().data_ptr(),
                direction.contiguous().data_ptr(), h, max_iterations, tol, base, *(t.data_ptr() for t in out))
    return out


def refine_relative_pose(pixels: torch.Tensor, conf: Optional[torch.Tensor], cams: torch.Tensor, pairs: Sequence[Tuple[int, int]],
                         rotation: torch.Tensor, direction: torch.Tensor, distortion: Optional[torch.Tensor] = None,
                         huber: Optional[float] = None, max_iterations: int = 20, step_tolerance: float = 1e-8, baseline: float = 1.0,
                         weight: Optional[torch.Tensor] = None) -> RelativeRefined:
    """The polish of relative_pose: rotation (P,3,3) and direction (P,3) float64 of x_b = R x_a + t moved to the minimum of
    E(R, t) = sum w rho(d^2), d the signed Sampson distance in pixels of a correspondence on the undistorted pixels, by
    Levenberg-Marquardt on the 5 unknowns (a rotation, and t on the unit sphere) from the given pose.  pixels, conf, cams, pairs and
    distortion are the arguments of relative_pose; w = conf_a * conf_b, times `weight` (B,P,J) float32 where given -- the inlier
    mask of relative_pose is such a tensor, and a correspondence whose weight is not finite and > 0 takes no part.  `huber` as in
    refine_points.  -> RelativeRefined(rotation, direction, cams, error, cost0, cost, used, iterations, status), one entry per pair.

    A trial is accepted only if it lowers E, so cost <= cost0.  Converged (status 0) when the step is <= step_tolerance, else capped
    (1) after `max_iterations` trials (0 .. 1000).  Passed through (2): max_iterations == 0 or fewer than 6 correspondences take
    part; the pose is returned bit for bit, error and costs are computed.  Invalid (3): the given pose or the intrinsics are not
    finite, or nothing takes part; the pose is returned as given, the records' poses, error and costs are NaN.  One launch, one
    workgroup per pair, no synchronisation, identical bits from run to run."""
    h, max_iterations, tol = _refine_options(huber, max_iterations, step_tolerance)
    base = _baseline(baseline)
    V = pixels.shape[1] if isinstance(pixels, torch.Tensor) and pixels.ndim == 4 else 0
    flat = _pairs(pairs, V) if V else []
    return _refine_relative(pixels, conf, weight, cams, flat, rotation, direction, distortion, h, max_iterations, tol, base)


def relative_pose(pixels: torch.Tensor, conf: Optional[torch.Tensor], cams: torch.Tensor, pairs: Sequence[Tuple[int, int]] = ((0, 1),),
                  distortion: Optional[torch.Tensor] = None, threshold: float = 6.0, hypotheses: int = 1024, seed: int = 0,
                  baseline: float = 1.0, refine: bool = False, huber: Optional[float] = None,
                  return_hypotheses: bool = False) -> RelativePose:
    """The relative pose of pairs of views from their detections and intrinsics alone: the step from pixels into locate_cameras, in
    the presence of wrong detections.  pixels (B,V,J,2), conf (B,V,J) or None, cams (V,16) float64 and distortion (V,5) or None are
    the arguments of locate_cameras, but of a record only fx fy cx cy and its lens row are read: the pose fields may be NaN.
    pairs: up to 32 (a, b) of distinct view indices.  -> RelativePose(rotation, direction, cams, inliers, count, best, error,
    status, refined, poses, scores, roots), one entry per pair; x_b = R x_a + t with |t| = 1.

    Per pair, `hypotheses` (1 .. 65536) five-point problems are solved, each on five participating correspondences drawn with the
    counter-based generator of synthesize_views under `seed`; each of its up to ten essential matrices gives a pose (the one that
    puts the five samples in front of both cameras) and is scored over all participating correspondences by the Sampson distance in
    pixels on the undistorted pixels: count = the correspondences within `threshold` (pixels, finite and > 0), cost = sum w
    min(d^2, threshold^2), w = conf_a * conf_b.  A hypothesis keeps its best candidate; the winner has the most inliers, then the
    lowest cost, then the lowest number (include/mpl_hip.h has the five steps).  A correspondence takes part when in both views
    the weight is finite and > 0 and the pixel is finite and goes back through the lens.

    Located (status 0): the winner has at least 6 inliers.  `cams` then holds a rig of the pair in the gauge of view a: record 0 is
    view a with R = I at the origin, record 1 view b with R at -baseline * R^T t -- `baseline` (finite, > 0) is the length the
    caller gives to what two views cannot see.  Invalid (3): fewer than 5 correspondences take part, no hypothesis is valid, the
    winner has fewer than 6 inliers or the intrinsics are not finite; the poses are NaN, count 0, the inliers 0.  A winner is a
    start, not a fit: from 136 correspondences with 2 px of noise and a quarter of each view's detections planted off it lies within
    a few degrees; a detection moved along its epipolar line is an inlier of any two-view test, so a few planted ones remain.
    refine=True adds one launch, the polish: refine_relative_pose(pixels, conf, cams, pairs, rotation, direction, distortion,
    huber=huber, baseline=baseline, weight=inliers), whose pose becomes `rotation`, `direction` and `cams` and which is returned
    whole as `refined`; inliers, count, best and error stay those of the hypothesis stage.  `huber` without `refine` raises.
    return_hypotheses=True hands out every hypothesis: poses (P,H,12), NaN where void, scores (P,H,2), (0, inf) where void, and
    roots (P,H), the real candidates.

    The recipe from pixels and intrinsics to a rig: relative_pose(pairs=((0, 1),), refine=True) -> triangulate_pixels on views 0 and 1 under
    .cams[0] -> locate_cameras(fixed=(0, 1), refine=True) with those two records in place -> bundle_adjust(fixed=(0, 1)).  Three
    launches before the polish, no synchronisation, nothing read back, identical bits from run to run."""
    from . import detrng
    h, tau, H, seed = _consensus_options(huber, refine, threshold, hypotheses, seed)
    base = _baseline(baseline)
    V = pixels.shape[1] if isinstance(pixels, torch.Tensor) and pixels.ndim == 4 else 0
    flat = _pairs(pairs, V) if V else []                 # a pixels tensor of another form is _observations' to complain about
    (pixels, conf), cams, distortion, B, V, J = _observations(None, pixels, conf, cams, distortion, with_points=False)
    dev = pixels.device
    P = len(flat) // 2
    keys = (cabi.C.c_uint64 * P)(*(int(detrng._stream_key(seed, "relative_pose", lane=p)) for p in range(P)))
    ws = torch.empty((cabi.load().mpl_relative_pose_workspace_bytes(B, P, J),), dtype=torch.uint8, device=dev)
    f64 = dict(dtype=torch.float64, device=dev)
    rotation, direction, out_cams = torch.empty((P, 3, 3), **f64), torch.empty((P, 3), **f64), torch.empty((P, 2, 16), **f64)
    inliers = torch.empty((B, P, J), dtype=torch.float32, device=dev)
    count = torch.empty((P,), dtype=torch.int32, device=dev)
    best = torch.empty((P,), dtype=torch.int32, device=dev)
    error = torch.empty((P,), **f64)
    status = torch.empty((P,), dtype=torch.uint8, device=dev)
    poses, scores = torch.empty((P, H, 12), **f64), torch.empty((P, H, 2), **f64)
    roots = torch.empty((P, H), dtype=torch.int32, device=dev)
    cabi.launch("relative_pose", dev, pixels.data_ptr(), ptr(conf), cams.data_ptr(), ptr(distortion), B, V, J, (cabi.C.c_int * len(flat))(*flat),
                P, tau, H, keys, base, ws.data_ptr(), ws.numel(), rotation.data_ptr(), direction.data_ptr(), out_cams.data_ptr(),
                inliers.data_ptr(), count.data_ptr(), best.data_ptr(), error.data_ptr(), status.data_ptr(), poses.data_ptr(),
                scores.data_ptr(), roots.data_ptr())
    refined = None
    if refine:
        refined = _refine_relative(pixels, conf, inliers, cams, flat, rotation, direction, distortion, h, 20, 1e-8, base)
        rotation, direction, out_cams = refined.rotation, refined.direction, refined.cams
    return RelativePose(rotation, direction, out_cams, inliers, count, best, error, status, refined, poses if return_hypotheses else None,
                        scores if return_hypotheses else None, roots if return_hypotheses else None)


def bundle_adjust(points: torch.Tensor, pixels: torch.Tensor, conf: Optional[torch.Tensor], cams: torch.Tensor,
                  distortion: Optional[torch.Tensor] = None, huber: Optional[float] = None, rounds: int = 5,
                  fixed: Sequence[int] = (), max_iterations: int = 20, step_tolerance: float = 1e-8) -> BundleAdjusted:
    """Alternating bundle adjustment: `rounds` times refine_cameras on the current points, then refine_points under the new
    cameras, and a last refine_cameras(max_iterations=0) that scores the result -- 2 * rounds + 1 launches, no kernel of its own,
    nothing read back.  -> BundleAdjusted(points, cams, cost, cameras, refined): cost (rounds+1,) float64 on the device, entry r
    the sum over the views of the cost before round r, the last entry the cost of the result; cameras / refined the last round's
    CamerasRefined / Refined (None with rounds=0, which returns the points and cameras it was given).  Both half-steps only ever
    lower the same total cost, so `cost` does not rise beyond the float32 rounding of the points.

    The gauge: with points and cameras both free the minimum is determined only up to a similarity of the world (a rotation, a
    translation and a scale move points and cameras together and leave every pixel where it is).  Two cameras in `fixed` pin it.
    One fixed camera pins rotation and translation but leaves the scale free: the cost still falls, but the points need not get
    closer to the truth.  With no camera fixed the result drifts within the gauge; it is then a statement about reprojection only.
    A point that is NaN stays NaN and takes no part in the camera fits.  A view that is invalid (status 3 of refine_cameras) has a
    NaN cost, and `cost`, a plain sum over the views, is then NaN in every entry: the trace says so instead of leaving the view out."""
    h, max_iterations, tol = _refine_options(huber, max_iterations, step_tolerance)
    try:
        n_rounds = -1 if isinstance(rounds, bool) else operator.index(rounds)
    except TypeError:
        n_rounds = -1
    if not 0 <= n_rounds <= 1000:
        raise RuntimeError("rounds must be an integer in [0, 1000] (got %r)" % (rounds,))
    V = pixels.shape[1] if isinstance(pixels, torch.Tensor) and pixels.ndim == 4 else 0
    mask = _fixed_mask(fixed, V) if V else 0
    costs, cameras, refined = [], None, None
    for _ in range(n_rounds):
        cameras = _refine_cameras(points, pixels, conf, cams, distortion, h, max_iterations, tol, mask)
        cams = cameras.cams
        costs.append(cameras.cost0.sum())
        refined = _refine(points, pixels, conf, cams, distortion, h, max_iterations, tol)
        points = refined.points
    score = _refine_cameras(points, pixels, conf, cams, distortion, h, 0, tol, mask)
    costs.append(score.cost0.sum())
    return BundleAdjusted(points, cams, torch.stack(costs), cameras, refined)


def _epipolar(rays, centers, conf, weight, threshold):
    rays, centers, conf, weight, stride, B, V, J = _lines(rays, centers, conf, weight)
    if V < 2:
        raise NotImplementedError("the epipolar error needs at least two views")
    dev = rays[0].device
    w_in = w_out = None
    if weight is not None:
        w_in = torch.stack(weight, dim=1)                # (B,V,J), the layout of the errors
        w_out = torch.empty_like(w_in)
    err = torch.empty((B, V, J), dtype=torch.float32, device=dev)
    cabi.launch("epipolar_errors", dev, table(rays), table(centers), table(conf), stride, B, V, J, err.data_ptr(), ptr(w_in), float(threshold),
                ptr(w_out))
    return err, w_out


def epipolar_errors(rays: Sequence[torch.Tensor], centers: Sequence[torch.Tensor], conf: Optional[Sequence[torch.Tensor]] = None
                    ) -> torch.Tensor:
    """(B,V,J): err[b,i,j] = conf_i / (V - 1) * sum over the other views k of the distance between lines i and k of joint j
    (calib.py:160-165; conf_i = 1 without confidences).  Parallel lines, where the reference divides 0 by 0, contribute the
    distance of the other centre to line i."""
    return _epipolar(rays, centers, conf, None, 0.0)[0]


def consistency_weights(rays: Sequence[torch.Tensor], centers: Sequence[torch.Tensor], conf: Optional[Sequence[torch.Tensor]],
                        weight: Sequence[torch.Tensor], threshold: float = 5.0) -> List[torch.Tensor]:
    """smart_pseudo_remove_weight (calib.py:116-169) for a whole batch: `weight` is a list of V (B,J) tensors; returns their copies
    with the joints whose epipolar error exceeds `threshold` set to 0 (views of one (B,V,J) tensor)."""
    if weight is None:
        raise RuntimeError("weight must be a non-empty list of tensors, one per view")
    return list(_epipolar(rays, centers, conf, weight, threshold)[1].unbind(1))
