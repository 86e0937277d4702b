"""Models outside NUM_JOINTS 17 / DIM 32 / HEADS 8, CPU side: the fp64 oracle against the shape fixtures (reference outputs),
the supported envelope as the binding reports it, and the library's predicate export."""
import ctypes
import types

import pytest
import torch

from openmpl_amd import cabi
from openmpl_amd import build as mpl_build
from openmpl_amd import detrng
from openmpl_amd.multiview_mpl import MultiView_MPL, get_multiview_mpl_net
from oracle import mpl_oracle
from tests.golden.shape_cases import SHAPE_CASES
from tests.shape_util import load_shape_golden, shape_inputs, shape_state_dict

NAMES = [c["name"] for c in SHAPE_CASES]
TOL = 2e-6


@pytest.mark.parametrize("name", NAMES)
def test_oracle_matches_reference_shape_golden(name):
    g = load_shape_golden(name)
    sd = shape_state_dict(g)
    poses, rays, centers = shape_inputs(g)
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


@pytest.mark.parametrize("name", NAMES)
def test_shape_cases_are_inside_the_envelope(name):
    flags = next(c["flags"] for c in SHAPE_CASES if c["name"] == name)
    m = MultiView_MPL(**flags)
    assert m._find_unsupported() is None
    assert m._unsupported is None
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == mpl_oracle.param_shapes(flags)


def _ns(d):
    return types.SimpleNamespace(**d)


def test_factory_accepts_reference_config_defaults():
    """lib/core/config.py:65-69 defaults DIM = 2, TRANSFORMER_HEADS = 2: a yaml that does not set them builds a model that runs."""
    net = dict(NUM_JOINTS=17, DIM=2, TRANSFORMER_DEPTH=4, TRANSFORMER_HEADS=2, TRANSFORMER_DROP_RATE=0.0,
               TRANSFORMER_ATTN_DROP_RATE=0.0, TRANSFORMER_DROP_PATH_RATE=0.1, TRANSFORMER_ADD_CONFIDENCE_INPUT=False,
               TRANSFORMER_MULT_CONFIDENCE_EMB=False, TRANSFORMER_CONCAT_CONFIDENCE_EMB=False,
               TRANSFORMER_CONFIDENCE_INPUT_AS_THIRD=False, POSE_3D_EMB_LEARNABLE=False,
               TRANSFORMER_LINEAR_WEIGHTED_MEAN=False, TRANSFORMER_ADD_3D_POS_ENCODING_IN_SPATIAL=False,
               TRANSFORMER_INPUT_RAYS_AS_TOKEN=False, TRANSFORMER_ADD_3D_POS_ENCODING_TO_RAYS=False,
               TRANSFORMER_CONF_ATTENTION_UNCERTAINTY_WEIGHT=False, TRANSFORMER_MULTIPLE_SPATIAL_BLOCKS=False,
               TRANSFORMER_NO_SPT=False, TRANSFORMER_NO_FPT=False, TRANSFORMER_CONFIDENCE_IN_FPT=False,
               TRANSFORMER_OUTPUT_HEAD_DEEP=False, TRANSFORMER_OUTPUT_HEAD_KADKHOD=False,
               TRANSFORMER_OUTPUT_HEAD_HIDDEN_DIM=1024, TRANSFORMER_FPT_BLOCKS_VIEW_KEYPOINT_TOKENS=False,
               INIT_WEIGHTS=True, INIT_WEIGHTS_FROM="scratch", PRETRAINED="")
    ds = dict(TEST_DATASET="multiview_h36m_mpl", TRAIN_VIEWS=None, USE_HELPER_CAMERAS=False, TRAIN_VIEWS_HELPER=None,
              TRAIN_ON_ALL_CAMERAS=False, TEST_ON_ALL_CAMERAS=False, N_VIEWS_TRAIN_TEST_ALL=4)
    model = get_multiview_mpl_net(_ns(dict(NETWORK=_ns(net), DATASET=_ns(ds))), is_train=False)
    assert model.features.embed_dim_ratio == 2 and model.features.num_heads == 2
    assert model.features._find_unsupported() is None
    for J in (14, 15, 19, 20):
        net.update(NUM_JOINTS=J, DIM=32, TRANSFORMER_HEADS=8)
        assert get_multiview_mpl_net(_ns(dict(NETWORK=_ns(net), DATASET=_ns(ds))), is_train=False).features._unsupported is None


@pytest.mark.parametrize("kw,limit", [
    (dict(num_joints=65), "NUM_JOINTS"),
    (dict(num_joints=64, embed_dim_ratio=128, num_heads=8), "4096"),
    (dict(num_joints=40, embed_dim_ratio=64, num_heads=8, input_rays_as_token=True), "4096"),
    (dict(embed_dim_ratio=129, num_heads=1), "DIM"),
    (dict(embed_dim_ratio=30, num_heads=8), "multiple of TRANSFORMER_HEADS"),
    (dict(num_joints=20, num_views=4, embed_dim_ratio=4, num_heads=2, FPT_blocks_view_keypoint_tokens=True), "head dim 4 or 8"),
])
def test_outside_the_envelope_names_the_limit(kw, limit):
    m = MultiView_MPL(**kw)
    msg = m._find_unsupported()
    assert msg is not None and limit in msg, msg
    assert cabi.load().mpl_config_supported(ctypes.byref(m._config())) == -2


def test_predicate_edges():
    lib = cabi.load()

    def ok(J, d, H, V=4, flags=cabi.F_POS3D_LEARN, depth=2):
        return lib.mpl_config_supported(ctypes.byref(cabi.Config(J, d, depth, H, V, 2, flags, 0))) == 0

    assert ok(17, 32, 8) and ok(1, 1, 1) and ok(64, 64, 64) and ok(32, 128, 1) and ok(17, 2, 2) and ok(15, 32, 8, V=32)
    assert not ok(0, 32, 8) and not ok(65, 32, 8) and not ok(17, 0, 1) and not ok(17, 32, 0) and not ok(17, 32, 3)
    assert not ok(17, 32, 8, V=33) and not ok(64, 65, 5)
    assert ok(32, 64, 2, flags=cabi.F_RAYS_TOKEN) and not ok(33, 64, 2, flags=cabi.F_RAYS_TOKEN)
    kp = cabi.F_POS3D_LEARN | cabi.F_KPTOK
    assert ok(8, 6, 3, V=4, flags=kp)                       # 32 tokens, head dim 2: short attention
    assert not ok(11, 6, 3, V=3, flags=kp)                  # 33 tokens, head dim 2
    assert ok(17, 32, 8, V=31, flags=kp) and ok(17, 16, 2, V=8, flags=kp)
    assert ok(11, 6, 3, V=3, flags=kp | cabi.F_NO_FPT)      # no FPT blocks: no token attention at all
    assert lib.mpl_config_supported(None) == -1


def test_library_exports_the_predicate_and_abi_matches():
    lib = ctypes.CDLL(mpl_build.build())
    assert hasattr(lib, "mpl_config_supported") and "mpl_config_supported" in cabi.EXPORTS
    lib.mpl_hip_abi_version.restype = ctypes.c_int
    assert lib.mpl_hip_abi_version() == cabi.ABI_VERSION == 14


def test_micro_and_fresh_models_build_in_the_envelope():
    for kw in (dict(num_joints=17, embed_dim_ratio=8, num_heads=2, depth=1, num_views=2),
               dict(num_joints=15, embed_dim_ratio=32, num_heads=8, depth=12, num_views=4, pose_3d_emb_learnable=True)):
        m = MultiView_MPL(**kw)
        detrng.fill_module_(m, seed=1)
        assert m._unsupported is None
