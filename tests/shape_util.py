"""Loading of the shape fixtures (tests/golden/shape_cases.py); weights are regenerated from detrng like the other goldens."""
import json
import os

import numpy as np
import torch

from openmpl_amd import detrng
from oracle import mpl_oracle
from tests.golden.shape_cases import SHAPE_BY_NAME

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_shape_golden(name):
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    g = {k: z[k] for k in z.files}
    g["flags"] = json.loads(bytes(g["flags"]).decode())
    g["meta"] = json.loads(bytes(g["meta"]).decode())
    g["name"] = name
    assert g["flags"] == SHAPE_BY_NAME[name]["flags"], "fixture is stale w.r.t. shape_cases.py"
    return g


def shape_inputs(g, device="cpu"):
    V = g["poses"].shape[0]
    mk = lambda a: [torch.from_numpy(np.ascontiguousarray(a[v])).to(device) for v in range(V)]
    return mk(g["poses"]), mk(g["rays"]), mk(g["centers"])


def shape_state_dict(g):
    shapes = mpl_oracle.param_shapes(g["flags"])
    return {k: torch.from_numpy(v) for k, v in detrng.make_state_dict(shapes, seed=g["meta"]["wseed"]).items()}
