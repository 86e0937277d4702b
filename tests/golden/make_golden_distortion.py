"""Golden vectors for the lens model (csrc/views.hpp, project_points(distortion=)) from the REFERENCE's own code (build container
only).  lib/multiviews/cameras.py is loaded in place (numpy only) and its project_pose is called itself.

Cases: B = 4, J = 17 points seen by V = 3 cameras at the focal length of H36M, under zero coefficients ("zeros"), the H36M-like set
("h36m") and the strong set ("strong") of tests/distortion_cases.py.  Points (float32, what the kernel reads), cameras, coefficient
tables and the float64 pixels are stored.      python tests/golden/make_golden_distortion.py
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle.ref_import import REFERENCE_ROOT  # noqa: E402
from tests import distortion_cases as dc  # noqa: E402
from tests import synth_cases as sc  # noqa: E402

spec = importlib.util.spec_from_file_location("_ref_cameras", os.path.join(REFERENCE_ROOT, "MPL", "lib", "multiviews", "cameras.py"))
cameras = importlib.util.module_from_spec(spec)
spec.loader.exec_module(cameras)

B, V, J = 4, 3, 17
points, cams = sc.scene(B, V, J, seed=3, focal=dc.FOCAL)
out = dict(points=points, cams=cams)
for name in ("zeros", "h36m", "strong"):
    dist = dc.table(name, V)
    px = np.zeros((B, V, J, 2))
    for v in range(V):
        # fx .. cy as arrays of one value: unfold_camera_param stacks them into the (2,1) columns the projection broadcasts with
        camera = dict(R=cams[v, 4:13].reshape(3, 3), T=cams[v, 13:16].reshape(3, 1), fx=cams[v, 0:1], fy=cams[v, 1:2], cx=cams[v, 2:3],
                      cy=cams[v, 3:4], k=dist[v, :3].reshape(3, 1), p=dist[v, 3:].reshape(2, 1))
        for b in range(B):
            px[b, v] = cameras.project_pose(points[b].astype(np.float64), camera)
    # the restatement agrees before anything is stored
    mine, depth = dc.project(points, cams, dist)
    assert depth.min() > 0.5
    np.testing.assert_allclose(mine, px, rtol=1e-12, atol=0)
    out[name + "_dist"], out[name + "_pixels"] = dist, px
    print(name, "largest shift against the pinhole: %.3f px" % np.abs(px - out["zeros_pixels"]).max())

path = os.path.join(HERE, "distortion.npz")
np.savez_compressed(path, **out)
print("%s: %d bytes, %d arrays" % (path, os.path.getsize(path), len(out)))
