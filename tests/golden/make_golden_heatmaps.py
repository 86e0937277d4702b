"""Golden vectors for the heatmap decoder (openmpl_amd/heatmaps.py) from the REFERENCE's own functions (build container only):
get_max_preds and get_final_preds (lib/core/inference.py:22-81, both TEST.POST_PROCESS values) with transform_preds
(lib/utils/transforms.py:51-94), and generate_heatmap (lib/dataset/joints_dataset_mpl.py:828-870), loaded in place.

OpenCV is not installed where this runs: the stub `cv2` provides getAffineTransform as a float64 solve of the three point pairs
in numpy (cv2 solves the same 6x6 system in double precision), on the float32-rounded points the reference hands it.  The
coordinates after the quarter-pixel shift, which get_final_preds does not return, are recorded at its call of transform_preds.
Only arrays are stored.  python tests/golden/make_golden_heatmaps.py"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from openmpl_amd import detrng  # noqa: E402
from tests import heatmap_cases as hc  # noqa: E402


def get_affine_transform(src, dst):
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    assert src.shape == (3, 2) and dst.shape == (3, 2)
    return np.linalg.solve(np.concatenate([src, np.ones((3, 1))], axis=1), dst).T        # (2,3): dst = M [x, y, 1]


cv2 = types.ModuleType("cv2")
cv2.getAffineTransform = get_affine_transform
sys.modules["cv2"] = cv2

LIB = "/root/reference/MPL/lib"
sys.path.insert(0, LIB)


def load(name, *path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(LIB, *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


inference = load("_ref_inference", "core", "inference.py")
DS = load("_ref_joints_dataset", "dataset", "joints_dataset_mpl.py").JointsDataset_MPL

seen = []
transform_preds = inference.transform_preds


def recording_transform_preds(coords, center, scale, output_size):
    seen.append(np.array(coords, copy=True))
    return transform_preds(coords, center, scale, output_size)


inference.transform_preds = recording_transform_preds

N, J = 12, 3
out = {}
for tag, (H, W) in (("64x64", (64, 64)), ("64x48", (64, 48))):
    # 27 maps of the case builders (Gaussians, special maps, edge peaks), then 9 of the reference's own generate_heatmap
    fake = types.SimpleNamespace(num_joints=9, heatmap_size=np.array([W, H]), image_size=np.array([4 * W, 4 * H]), sigma=2)
    joints = np.concatenate([detrng.uniform(3, "gold.joints." + tag, (9, 2), -0.05, 1.05) * np.array([4.0 * W, 4.0 * H]), np.zeros((9, 1))],
                            axis=1)                          # image pixels, some of them just outside the image
    joints[0, :2] = (4.0 * 1, 4.0 * (H - 2))                 # peaks at cell (1, H-2) and at (W-2, 2)
    joints[1, :2] = (4.0 * (W - 2), 4.0 * 2)
    target, weight = DS.generate_heatmap(fake, joints, np.ones((9, 3), np.float32))
    assert target.shape == (9, H, W) and weight.sum() >= 7
    hm = np.concatenate([hc.maps(27, H, W, seed=5), target.astype(np.float32)]).reshape(N, J, H, W)
    center = detrng.uniform(5, "gold.center." + tag, (N, 2), 100.0, 900.0)
    scale = detrng.uniform(5, "gold.scale." + tag, (N, 2), 0.8, 2.5)
    coords, maxvals = inference.get_max_preds(hm)
    out[tag + "_hm"], out[tag + "_center"], out[tag + "_scale"] = hm, center, scale
    out[tag + "_coords"], out[tag + "_maxvals"] = coords, maxvals[..., 0]
    for post in (False, True):
        del seen[:]
        cfg = types.SimpleNamespace(TEST=types.SimpleNamespace(POST_PROCESS=post))
        preds, mv = inference.get_final_preds(cfg, hm, center, scale)
        assert preds.dtype == np.float32 and np.array_equal(mv, maxvals, equal_nan=True) and len(seen) == N
        out[tag + ("_preds_post" if post else "_preds")] = preds
        out[tag + ("_coords_post" if post else "_coords_plain")] = np.stack(seen).astype(np.float32)
    assert np.array_equal(out[tag + "_coords_plain"], coords)
    print(tag, "shifted:", int((out[tag + "_coords_post"] != coords).any(-1).sum()), "of", N * J, "maps; NaN maxvals:",
          int(np.isnan(maxvals).sum()))
path = os.path.join(HERE, "heatmaps.npz")
np.savez_compressed(path, **out)
print(path, os.path.getsize(path), "bytes")
