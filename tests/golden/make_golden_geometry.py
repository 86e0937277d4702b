"""Golden vectors for the geometry kernels (openmpl_amd/geometry.py) from the REFERENCE's own code (build container only).

lib/utils/calib.py is loaded in place.  Per case (V = 2, 3, 4 views, J = 17, 5 samples): cameras on an inward-looking ring (metres),
world points projected with the reference's world_to_cam / cam_to_image, detections = projections + pixel noise from detrng, a few
of them far off (the joints the threshold is there to catch).  The lines the kernels read follow the reference's own convention:
centers = cam_to_world of the camera origin, rays = cam_to_world of the depth-1 back-projection [(u - cx) / fx, (v - cy) / fy, 1],
both float64 and rounded once to float32.  smart_pseudo_remove_weight is called once per sample, as the datasets do; its calls
of distance_between_two_skew_lines (on find_3_points_on_ray + cam_to_world points) are recorded, the per-view errors before the
threshold are its lines :162-165 on those recorded distances, and the weights are what it returns.

Detections keep |u - cx|, |v - cy| >= 1 px, where find_3_points_on_ray is finite; the threshold is one no stored error lies within
1e-3 (relative) of, so float32 kernels must reproduce the weights exactly.      python tests/golden/make_golden_geometry.py
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from openmpl_amd import detrng  # noqa: E402
from oracle.ref_import import REFERENCE_ROOT  # noqa: E402

spec = importlib.util.spec_from_file_location("_ref_calib", os.path.join(REFERENCE_ROOT, "MPL", "lib", "utils", "calib.py"))
calib = importlib.util.module_from_spec(spec)
spec.loader.exec_module(calib)

RECORDED = []
_dist = calib.distance_between_two_skew_lines


def rec_dist(p0, p1):
    r = _dist(p0, p1)
    RECORDED.append(r)
    return r


calib.distance_between_two_skew_lines = rec_dist

B, J, THRESHOLD = 5, 17, 0.03


def look_at(centre):
    """world->camera rotation of a camera at `centre` whose optical axis points at the origin"""
    z = -centre / np.linalg.norm(centre)
    x = np.cross(np.array([0.0, 0.0, 1.0]), z)
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z])


out = {}
for V in (2, 3, 4):
    tag = "v%d" % V
    az = np.deg2rad(40.0) * (np.arange(V) + detrng.uniform(21, "az." + tag, (V,), 0.0, 0.3).astype(np.float64))      # no two cameras face each other
    cen = np.stack([4.0 * np.cos(az), 4.0 * np.sin(az), 1.0 + detrng.uniform(21, "h." + tag, (V,), 0.0, 1.5).astype(np.float64)], axis=1)
    cams = []
    for v in range(V):
        R = look_at(cen[v])
        cams.append(dict(fx=1100.0 + 37 * v, fy=1120.0 - 11 * v, cx=500.0 + 13.0 * v, cy=500.0 - 7.0 * v, R=R,
                         t=(-R @ cen[v]).reshape(3, 1)))           # [R | t]: x_cam = R x_world + t (calib.py:22-40)
    world = detrng.uniform(21, "pts." + tag, (B, J, 3), -0.8, 0.8).astype(np.float64) + np.array([0.0, 0.0, 1.0])
    px = np.zeros((V, B, J, 2))
    for v, cam in enumerate(cams):
        K = np.array([[cam["fx"], 0, cam["cx"]], [0, cam["fy"], cam["cy"]], [0, 0, 1.0]])
        px[v] = calib.cam_to_image(calib.world_to_cam(world, cam["R"], cam["t"]), K)
        px[v] += detrng.normal(21, "noise.%s.%d" % (tag, v), (B, J, 2), 0.0, 3.0)
        far = detrng.uniform(21, "far.%s.%d" % (tag, v), (B, J, 1), 0.0, 1.0) < 0.08
        px[v] += far * detrng.uniform(21, "off.%s.%d" % (tag, v), (B, J, 2), 30.0, 90.0)
        for a, c0 in ((0, cam["cx"]), (1, cam["cy"])):             # keep the reference's own formula finite
            near = np.abs(px[v, ..., a] - c0) < 1.0
            px[v, ..., a] = np.where(near, c0 + 1.5, px[v, ..., a])
    conf = np.stack([detrng.uniform(21, "conf.%s.%d" % (tag, v), (B, J), 0.05, 1.0) for v in range(V)]).astype(np.float32)
    weight = np.stack([detrng.uniform(21, "w.%s.%d" % (tag, v), (B, J), 0.1, 1.0) for v in range(V)]).astype(np.float32)

    rays, centers = np.zeros((V, B, J, 3), np.float32), np.zeros((V, B, 1, 3), np.float32)
    for v, cam in enumerate(cams):
        u = np.stack([(px[v, ..., 0] - cam["cx"]) / cam["fx"], (px[v, ..., 1] - cam["cy"]) / cam["fy"], np.ones((B, J))], axis=-1)
        rays[v] = calib.cam_to_world(u, cam["R"], cam["t"])
        centers[v] = calib.cam_to_world(np.zeros((B, 1, 3)), cam["R"], cam["t"])

    n_pairs = V * (V - 1) // 2
    pairs, err, wout = np.zeros((n_pairs, B, J)), np.zeros((B, V, J)), np.zeros((V, B, J), np.float32)
    for b in range(B):
        meta = [dict(joints_2d=px[v, b], joints_2d_conf=conf[v, b].astype(np.float64), camera=cams[v]) for v in range(V)]
        del RECORDED[:]
        res = calib.smart_pseudo_remove_weight([None] * V, [weight[v, b].copy() for v in range(V)], meta, epipolar_error_threshold=THRESHOLD)
        assert len(RECORDED) == n_pairs
        e, p = np.zeros((V, J)), 0
        for i in range(V):
            for k in range(i + 1, V):
                pairs[p, b] = RECORDED[p]
                e[i] += RECORDED[p] * meta[i]["joints_2d_conf"]        # :162-163
                e[k] += RECORDED[p] * meta[k]["joints_2d_conf"]
                p += 1
        err[b] = e / (V - 1)                                           # :165
        for v in range(V):
            wout[v, b] = res[v]
            assert np.array_equal(res[v], np.where(err[b, v] > THRESHOLD, 0.0, weight[v, b]).astype(np.float32))
    assert np.isfinite(err).all() and np.abs(err / THRESHOLD - 1.0).min() > 1e-3
    assert (wout == 0).any() and (wout != 0).any()
    out.update({tag + "_rays": rays, tag + "_centers": centers, tag + "_conf": conf, tag + "_weight": weight, tag + "_pairs": pairs,
                tag + "_err": err, tag + "_weights_out": wout, tag + "_threshold": np.float64(THRESHOLD), tag + "_px": px.astype(np.float32)})
    print(tag, "max err %.4f  zeroed %d of %d  closest to the threshold %.2e" % (err.max(), int((wout == 0).sum()), wout.size,
                                                                              np.abs(err / THRESHOLD - 1.0).min()))
np.savez_compressed(os.path.join(HERE, "geometry.npz"), **out)
