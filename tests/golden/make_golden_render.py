"""Golden vectors for render_heatmaps(mode="reference") (openmpl_amd/heatmaps.py) from the REFERENCE's own generate_heatmap
(lib/dataset/joints_dataset_mpl.py:828-870), loaded in place (build container only).

Per map size (64 x 64, 64 x 48) and sigma (1, 2, 3), with the reference's feat_stride of 4 image pixels per cell: joints whose
patch lies inside the map, is cut by each of the four borders, lies wholly outside on each side, has a negative m + 0.5 (int()
truncates towards zero), ends exactly at the border (an empty patch that keeps its weight), and visibilities 0, 0.4 and 1.
The joints are float32 values, handed to the reference widened.  Only arrays are stored.
python tests/golden/make_golden_render.py"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from openmpl_amd import detrng  # noqa: E402
from tests import render_cases as rc  # noqa: E402

sys.modules.setdefault("cv2", types.ModuleType("cv2"))
LIB = "/root/reference/MPL/lib"
sys.path.insert(0, LIB)
spec = importlib.util.spec_from_file_location("_ref_joints_dataset", os.path.join(LIB, "dataset", "joints_dataset_mpl.py"))
mod = importlib.util.module_from_spec(spec)
spec.loader.exec_module(mod)
DS = mod.JointsDataset_MPL

STRIDE = 4.0
out = {}
for tag, W, H in rc.GOLDEN_SIZES:
    for sigma in rc.GOLDEN_SIGMAS:
        t = 3 * sigma
        r = detrng.uniform(7, "gold.render.%s.%d" % (tag, sigma), (4, 2), 0.0, 1.0).astype(np.float64)
        mid = lambda i: (t + 1 + r[i, 0] * (W - 2 * t - 3), t + 1 + r[i, 1] * (H - 2 * t - 3))          # the patch is inside
        cells = [mid(0),                                  # inside
                 (1.3, mid(1)[1]), (W - 2 + 0.4, mid(1)[1]), (mid(1)[0], 0.6), (mid(1)[0], H - 1.2),     # cut by each border
                 (-(t + 3.0), mid(2)[1]), (W + t + 0.2, mid(2)[1]), (mid(2)[0], -(t + 2.7)), (mid(2)[0], H + t + 1.0),   # outside
                 (-0.8, mid(3)[1]), (mid(3)[0], -1.7),    # m + 0.5 = -0.3 -> 0, -1.2 -> -1: truncation, not floor
                 (-(t + 1.5), mid(3)[1]),                 # br == 0: not "outside" for the reference, yet nothing to write
                 (W - 1 + t, H - 1 + t),                  # ul == size - 1: one cell, the patch's corner
                 mid(1), mid(2), mid(3)]                  # the visibilities below
        vis = np.ones(len(cells), np.float32)
        vis[-3:] = (0.0, 0.4, 1.0)
        vis[1] = 0.6                                      # above one half: written
        joints = (np.array(cells, np.float64) * STRIDE).astype(np.float32)
        n = len(cells)
        fake = types.SimpleNamespace(num_joints=n, heatmap_size=np.array([W, H]), image_size=np.array([STRIDE * W, STRIDE * H]), sigma=sigma)
        j3 = np.concatenate([joints.astype(np.float64), np.zeros((n, 1))], axis=1)
        target, weight = DS.generate_heatmap(fake, j3, np.repeat(vis[:, None], 3, axis=1))
        assert target.shape == (n, H, W) and target.dtype == np.float32 and weight.shape == (n, 1)
        key = "%s_s%d" % (tag, sigma)
        out[key + "_joints"], out[key + "_vis"], out[key + "_target"], out[key + "_weight"] = joints, vis, target, weight[:, 0]
        print(key, "maps:", n, "weights:", weight[:, 0].tolist(), "non-zero maps:", int((target.reshape(n, -1) != 0).any(1).sum()))
out["stride"] = np.array([STRIDE, STRIDE])
path = os.path.join(HERE, "render.npz")
np.savez_compressed(path, **out)
print(path, os.path.getsize(path), "bytes")
