"""The closed loop of smooth_tracks on the device, shared by tests/test_smooth_tracks_gpu.py and tools/smooth_tracks_prof.py: a body
moving along sinusoids (T = 256 frames, V = 4 cameras, J = 17) -> synthesize_views(noise_level=2) under the H36M-like lens ->
triangulate_pixels(refine=True) -> smooth_tracks, beside the float64 chain on the device's own fp32 pixels (the restatements of
tests/refine_cases.py, then of tests/smooth_tracks_cases.py)."""
import functools

import numpy as np
import torch

from tests import distortion_cases as dc
from tests import refine_cases as rc
from tests import smooth_tracks_cases as stc
from tests import synth_cases as sc

SMOOTHNESS, ORDER = 30.0, 2            # the window is about 2.9 * SMOOTHNESS^(1/4) = 7 frames; the slowest motion bends over 150


def sequence(T=256, V=4, J=17, seed=13):
    """placed poses (T,J,3) float32: one pose of synth_cases.scene carried along three sinusoids of 150 to 400 frames (0.15 units)
    with every joint swinging 0.03 units on its own; and the cameras"""
    pose, cams = sc.scene(1, V, J, seed=seed, focal=dc.FOCAL)
    rs = np.random.RandomState(500 + seed)
    t = np.arange(T)[:, None, None]

    def waves(shape, amplitude):
        x = np.zeros((T,) + shape)
        for _ in range(3):
            x = x + rs.uniform(0.5, 1.0, (1,) + shape) * np.sin(2 * np.pi * t / rs.uniform(150.0, 400.0, (1,) + shape) + rs.uniform(0, 2 * np.pi, (1,) + shape))
        return amplitude * x / 2.0
    placed = pose.astype(np.float64) + waves((1, 3), 0.15) + waves((J, 3), 0.03)
    return placed.astype(np.float32), cams


@functools.lru_cache(maxsize=None)
def closed_loop(T=256, V=4, J=17, seed=13):
    """-> dict(raw, device, float64): mean distance to the placed poses of the refined triangulation, of its smoothing on the device
    and of the float64 chain's smoothing; and iterations / status of the device's call"""
    from openmpl_amd import smooth_tracks, synthesize_views, triangulate_pixels
    placed, cams = sequence(T, V, J, seed)
    dist = dc.table("h36m", V)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    P, Cm, D = dev(placed), dev(cams), dev(dist)
    r = synthesize_views(P, Cm, rc.WH, seed=21, noise_level=2.0, normalize_inputs=False, normalize_cameras=False, return_pixels=True,
                         distortion=D)
    conf = torch.stack([p[..., 2] for p in r.poses], dim=1).contiguous()
    tri, _, _ = triangulate_pixels(r.pixels, conf, Cm, rc.WH, distortion=D, refine=True)
    sm = smooth_tracks(tri, smoothness=SMOOTHNESS, order=ORDER)
    truth = placed.astype(np.float64)
    dist_to = lambda x: float(np.linalg.norm(np.asarray(x, dtype=np.float64) - truth, axis=-1).mean())      # noqa: E731
    # the float64 chain on the same fp32 pixels
    px, cf = r.pixels.cpu().numpy(), conf.cpu().numpy()
    x64 = rc.linear_points(px, cf, cams, dist).astype(np.float32)
    r64 = rc.refine(x64, px, cf, cams, dist)
    s64 = stc.smooth(r64["points"].astype(np.float32), None, None, smoothness=SMOOTHNESS, order=ORDER)
    return dict(raw=dist_to(tri.cpu().numpy()), device=dist_to(sm.points.cpu().numpy()), float64=dist_to(s64["points"]),
                raw64=dist_to(r64["points"]), status=sm.status.cpu().numpy(), iterations=sm.iterations.cpu().numpy())
