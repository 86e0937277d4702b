"""Pin the oracle: it must reproduce every golden vector captured from the reference."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import mpl_oracle
from openmpl_amd import detrng
from tests.golden.cases import CASES, MICRO
from tests.util import GOLDEN_DIR, golden_inputs, golden_state_dict, load_golden

ALL = [c["name"] for c in CASES] + [MICRO["name"]]
TOL = 2e-6   # oracle and reference run the same ATen ops; observed <= 2e-7


@pytest.mark.parametrize("name", ALL)
def test_oracle_matches_reference_golden(name):
    g = load_golden(name)
    sd = golden_state_dict(name, g)
    poses, rays, centers = golden_inputs(g)
    taps = {}
    out = mpl_oracle.forward(sd, g["flags"], poses, rays, centers, taps=taps)
    if isinstance(out, tuple):
        out, inter = out
        for got, key in zip(inter, ("out_x1", "out_x2")):
            mx, nw = mpl_oracle.rel_errors(got, torch.from_numpy(g[key]))
            assert mx < TOL and nw < TOL, (key, mx, nw)
    mx, nw = mpl_oracle.rel_errors(out, torch.from_numpy(g["out"]))
    assert mx < TOL and nw < TOL, (mx, nw)
    for k in ("spt_view0", "fpt_in", "fused"):
        mx, nw = mpl_oracle.rel_errors(taps[k], torch.from_numpy(g["tap_" + k]))
        assert mx < TOL and nw < TOL, (k, mx, nw)


def test_param_shapes_cover_state_dict_of_micro_fixture():
    g = load_golden(MICRO["name"])
    shapes = mpl_oracle.param_shapes(g["flags"])
    stored = {k[2:]: tuple(v.shape) for k, v in g.items() if k.startswith("w:")}
    assert shapes == stored


def test_flop_count_matches_survey_table():
    # SURVEY.md section 8d / BASELINE.md section 3
    ch = dict(depth=12, num_views=4, pose_3d_emb_learnable=True)
    full = dict(ch, confidence_input_as_third=True, input_rays_as_token=True,
                multiple_spatial_blocks=True, add_3D_pos_encoding_to_rays=True)
    assert abs(mpl_oracle.flop_count(ch) / 1e6 - 263.1) < 0.2
    assert abs(mpl_oracle.flop_count(full) / 1e6 - 1002.3) < 0.3


def test_block_schedule_last_block_twice():
    assert mpl_oracle.block_schedule(3) == [(0, False), (1, False), (2, False), (2, False)]
    assert mpl_oracle.block_schedule(2, True) == [(0, True), (0, False), (1, True), (1, False), (1, False)]


@pytest.mark.parametrize("name", ["chosen_v4_b8_l2", "full_v4_b8_l2", "conf_attnw_v3_b3_l2", "kadkhod_v3_b3_l2"])
def test_oracle_matches_live_reference_on_fresh_inputs(name):
    """Different weights/inputs than the fixtures: guards against over-fitting to the goldens.  The reference's outputs
    for them were recorded by tests/golden/make_golden_reference.py (reference_fresh.npz); weights and inputs are
    regenerated from the same detrng seeds."""
    flags = load_golden(name)["flags"]
    fresh = np.load(os.path.join(GOLDEN_DIR, "reference_fresh.npz"))
    meta = json.loads(bytes(fresh["meta"]).decode())
    shapes = mpl_oracle.param_shapes(flags)
    sd = {k: torch.from_numpy(v) for k, v in detrng.make_state_dict(shapes, seed=meta["wseed"]).items()}
    p, r, c = detrng.make_inputs(meta["batch"], flags["num_views"], seed=meta["iseed"])
    P = [torch.from_numpy(x) for x in p]
    R = [torch.from_numpy(x) for x in r]
    C = [torch.from_numpy(x) for x in c]
    ref = torch.from_numpy(fresh[name])
    out = mpl_oracle.forward(sd, flags, P, R, C)
    if isinstance(out, tuple):
        out = out[0]
    mx, nw = mpl_oracle.rel_errors(out, ref)
    assert mx < TOL and nw < TOL
