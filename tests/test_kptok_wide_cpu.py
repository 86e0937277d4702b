"""The joints x views token grid (FPT_blocks_view_keypoint_tokens) at head dims 16 .. 128, CPU side: what the library's
predicate (mpl_config_supported) and the binding (_find_unsupported) accept and refuse.  Beyond 32 tokens the rule is: head dim 4
or 8 with K / V of a head in 64 KiB of LDS, or a multiple of 16 up to 128 with at most 2048 tokens."""
import ctypes

import pytest

from openmpl_amd import cabi
from openmpl_amd.multiview_mpl import MultiView_MPL

E_UNSUPPORTED = -2
NEW_RULE = "head dim 4 or 8, or a multiple of 16 up to 128"


def _model(J, d, H, V, depth=2, **extra):
    return MultiView_MPL(num_joints=J, embed_dim_ratio=d, num_heads=H, num_views=V, depth=depth,
                         FPT_blocks_view_keypoint_tokens=True, **extra)


def _supported(m):
    return cabi.load().mpl_config_supported(ctypes.byref(m._config()))


ACCEPTED = [
    # J, DIM, H, V, depth
    (17, 32, 2, 2, 2),      # 34 tokens, hd 16
    (17, 32, 1, 4, 2),      # 68 tokens, hd 32
    (17, 64, 1, 3, 2),      # 51 tokens, hd 64
    (17, 128, 1, 2, 2),     # hd 128
    (17, 48, 1, 2, 2),      # hd 48
    (64, 16, 1, 32, 2),     # 2048 tokens, hd 16
    (64, 64, 1, 32, 2),     # 2048 tokens x hd 64
    (17, 32, 2, 31, 12),    # 527 tokens, depth 12
]


@pytest.mark.parametrize("J,d,H,V,depth", ACCEPTED, ids=["J%d-d%d-H%d-V%d-L%d" % c for c in ACCEPTED])
def test_wide_head_keypoint_token_models_are_accepted(J, d, H, V, depth):
    m = _model(J, d, H, V, depth)
    assert _supported(m) == 0
    assert m._find_unsupported() is None and m._unsupported is None


REFUSED = [
    # J, DIM, H, V
    (11, 6, 2, 3),      # 33 tokens, hd 3
    (11, 6, 3, 3),      # 33 tokens, hd 2
    (20, 4, 2, 4),      # 80 tokens, hd 2
    (17, 20, 1, 2),     # hd 20
    (17, 24, 2, 2),     # hd 12
]


@pytest.mark.parametrize("J,d,H,V", REFUSED, ids=["J%d-d%d-H%d-V%d" % c for c in REFUSED])
def test_other_head_dims_beyond_32_tokens_are_refused_and_the_message_names_the_rule(J, d, H, V):
    m = _model(J, d, H, V)
    assert _supported(m) == E_UNSUPPORTED
    msg = m._find_unsupported()
    assert msg is not None and NEW_RULE in msg and "head dim %d" % (d // H) in msg, msg


def test_resident_kernels_keep_their_length_limit():
    """hd 4 / 8 beyond 64 KiB of K / V per head stay refused (hd 8 x 2048 tokens = 128 KiB); at the limit they run as before."""
    m = _model(64, 8, 1, 32)
    assert _supported(m) == E_UNSUPPORTED and m._find_unsupported()
    assert _supported(_model(64, 4, 1, 32)) == 0 and _supported(_model(64, 8, 1, 16)) == 0


def test_keypoint_tokens_with_ray_tokens_stay_refused():
    m = _model(17, 32, 2, 2, input_rays_as_token=True)
    assert _supported(m) == E_UNSUPPORTED
    assert "input_rays_as_token" in m._find_unsupported()


def test_predicate_edges_of_the_wide_rule():
    def ok(J, d, H, V, depth=2, flags=cabi.F_POS3D_LEARN | cabi.F_KPTOK):
        return cabi.load().mpl_config_supported(ctypes.byref(cabi.Config(J, d, depth, H, V, 2, flags, 0))) == 0

    assert ok(33, 16, 1, 1) and ok(32, 128, 1, 32) and ok(32, 128, 8, 32) and ok(64, 64, 4, 32) and ok(17, 112, 1, 2) and ok(17, 96, 2, 2)
    assert not ok(17, 20, 1, 2) and not ok(17, 36, 1, 2) and not ok(17, 24, 1, 2) and not ok(17, 2, 1, 2)
    assert ok(16, 20, 1, 2)                                   # 32 tokens: the short kernels, any head dim
    assert ok(17, 20, 1, 2, depth=0) and ok(17, 20, 1, 2, flags=cabi.F_KPTOK | cabi.F_NO_FPT)     # no FPT blocks: no attention


def test_bf16_still_raises_on_an_accepted_wide_head_model():
    m = _model(17, 32, 2, 2)
    assert m._unsupported is None
    with pytest.raises(NotImplementedError):
        m.set_matmul_precision("bf16")
    assert m.matmul_precision == "fp32"
