"""What the REFERENCE's find_tensor_peak_batch (lib/core/inference.py:84-134) returns, called in place under the installed torch, on
500 clean Gaussians (build container only).  It is a recorded comparison, not an oracle: `index / W` is a true division, so the
row is fractional, and normalize() is written for align_corners=True while affine_grid / grid_sample default to False.  Stored:
the means and amplitudes of the maps (tests regenerate the maps with heatmap_cases.gaussian) and the function's outputs at radius
2 and 6 with downsample 1 (pix2coord is then the identity).  python tests/golden/make_golden_subpixel.py"""
import importlib.util
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from openmpl_amd import detrng  # noqa: E402
from tests import heatmap_cases as hc  # noqa: E402

sys.modules.setdefault("cv2", types.ModuleType("cv2"))
LIB = "/root/reference/MPL/lib"
sys.path.insert(0, LIB)
spec = importlib.util.spec_from_file_location("_ref_inference", os.path.join(LIB, "core", "inference.py"))
inference = importlib.util.module_from_spec(spec)
spec.loader.exec_module(inference)

N, H, W = 500, 64, 64
mx = detrng.uniform(13, "gold.subpixel.mx", (N,), 3.0, W - 4.0)
my = detrng.uniform(13, "gold.subpixel.my", (N,), 3.0, H - 4.0)
amp = detrng.uniform(13, "gold.subpixel.amp", (N,), 0.2, 1.0)
hm = torch.from_numpy(hc.gaussian(H, W, mx, my, amp))
out = dict(mx=mx, my=my, amp=amp)
for radius in (2, 6):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        xy, score = inference.find_tensor_peak_batch(hm, radius, 1)
    out["r%d" % radius] = xy.numpy().astype(np.float32)
    err = np.abs(out["r%d" % radius].astype(np.float64) - np.stack([mx, my], -1))
    print("radius %d: mean |error| x %.3f, y %.3f cells" % (radius, err[:, 0].mean(), err[:, 1].mean()))
path = os.path.join(HERE, "subpixel.npz")
np.savez_compressed(path, **out)
print(path, os.path.getsize(path), "bytes")
