"""The shape-general bf16 engine without a GPU: its exports, the size and layout rules, and the predicate that decides which
bf16 operand layout a block stack carries (mpl_bf16_operand_layout)."""
import ctypes as C

import pytest

from openmpl_amd import cabi
from openmpl_amd.multiview_mpl import MultiView_MPL
from tests import bf16_any_cases


def test_pack_bf16_any_bytes_exists_and_answers_without_a_gpu():
    lib = cabi.load()
    assert "mpl_pack_bf16_any_bytes" in cabi.EXPORTS and "mpl_pack_bf16_any" in cabi.EXPORTS
    assert lib.mpl_pack_bf16_any_bytes(45, 15) > 0
    # one 64-column block, one 32-deep k-tile of 4 KiB, then c[45] and s[45] in fp32, padded to 16 bytes
    assert lib.mpl_pack_bf16_any_bytes(45, 15) == 4096 + (2 * 45 * 4 + 15) // 16 * 16
    assert lib.mpl_pack_bf16_any_bytes(65, 33) == 2 * 2 * 4096 + (2 * 65 * 4 + 15) // 16 * 16
    for n, k in ((1, 1), (8192, 8192), (12288, 4096), (4096, 8192), (255, 8192), (136, 32)):
        assert lib.mpl_pack_bf16_any_bytes(n, k) > 0, (n, k)
    for n, k in ((0, 5), (5, 0), (-1, 5), (5, -7), (5, 8193), (16385, 5)):
        assert lib.mpl_pack_bf16_any_bytes(n, k) == 0, (n, k)
    assert lib.mpl_ln_linear_bf16_any_workspace_bytes(3, 33) == 3 * 64 * 2
    assert lib.mpl_ln_linear_bf16_any_workspace_bytes(0, 33) == 0


def test_tuned_operand_sizes_are_untouched():
    lib = cabi.load()
    assert lib.mpl_pack_bf16_bytes(544, 544) == 4 * 9 * 18 * 1024 + (5 * 544 + 8) * 4
    for n, k in ((100, 544), (544, 40), (136, 32), (45, 15)):
        assert lib.mpl_pack_bf16_bytes(n, k) == 0


def test_layout_predicate():
    lib = cabi.load()
    lay = lib.mpl_bf16_operand_layout
    assert (cabi.BF16_NONE, cabi.BF16_TUNED, cabi.BF16_ANY) == (0, 1, 2)
    assert lay(544, 8, 4) == cabi.BF16_TUNED and lay(1088, 8, 8) == cabi.BF16_TUNED and lay(544, 8, 32) == cabi.BF16_TUNED
    assert lay(544, 16, 4) == cabi.BF16_ANY             # width 544, head 34: the tuned engine cannot fuse its attention
    for D, H in ((480, 8), (640, 8), (34, 2), (1024, 16), (85, 5), (64, 1), (32, 8), (4096, 8), (2176, 1), (1, 1)):
        assert lay(D, H, 4) == cabi.BF16_ANY, (D, H)
    # wider multiples of 544 with a head the tuned engine fuses (68): it packs no LayerNorm operand beyond K = 1088 -> shape-general
    assert lay(1632, 24, 4) == cabi.BF16_ANY and lay(2176, 32, 4) == cabi.BF16_ANY and lay(1088, 16, 4) == cabi.BF16_TUNED
    assert lay(480, 8, 33) == cabi.BF16_NONE and lay(544, 8, 33) == cabi.BF16_NONE      # beyond 32 tokens per sequence
    assert lay(480, 7, 4) == cabi.BF16_NONE and lay(4097, 1, 4) == cabi.BF16_NONE
    assert lay(0, 8, 4) < 0 and lay(480, 0, 4) < 0 and lay(480, 8, 0) < 0
    # the form query names the engine without a launch: invalid arguments are refused before any device query
    assert cabi.FORM_BF16_ANY == 8 and cabi.FORM_KERNELS[cabi.FORM_BF16_ANY] == "b1a_gemm_kernel"


def test_block_weights_struct_and_abi_did_not_move():
    lib = cabi.load()
    assert lib.mpl_hip_abi_version() == cabi.ABI_VERSION == 14
    assert C.sizeof(cabi.BlockWeights) == 24 * C.sizeof(C.c_void_p)


def test_precision_knob_accepts_every_view_token_model_and_names_what_it_refuses():
    for name, flags, _ in bf16_any_cases.PARITY_CASES:
        if flags["num_joints"] * flags["embed_dim_ratio"] > 1700:
            continue                                   # (the wide ones only cost construction time here; the GPU test runs them)
        m = MultiView_MPL(**flags)
        assert m._unsupported is None, (name, m._unsupported)
        assert m.set_matmul_precision("bf16").matmul_precision == "bf16"
        assert m._bf16_layout() == cabi.BF16_ANY, name
    tuned = MultiView_MPL(num_joints=17, embed_dim_ratio=32, num_heads=8, depth=1, num_views=8, pose_3d_emb_learnable=True)
    assert tuned.set_matmul_precision("bf16")._bf16_layout() == cabi.BF16_TUNED and tuned._x3_supported()
    base = dict(num_joints=15, embed_dim_ratio=32, num_heads=8, depth=2, num_views=3, pose_3d_emb_learnable=True)
    for extra in (dict(FPT_blocks_view_keypoint_tokens=True), dict(no_transformer_fpt=True), dict(depth=0)):
        m = MultiView_MPL(**dict(base, **extra))
        with pytest.raises(NotImplementedError, match="FPT_blocks_view_keypoint_tokens"):
            m.set_matmul_precision("bf16")
        assert m.matmul_precision == "fp32"
    # extra models the knob must take: ray tokens, no SPT transformer, one view, 32 views
    for extra in (dict(input_rays_as_token=True), dict(no_transformer_spt=True), dict(num_views=1), dict(num_views=32)):
        assert MultiView_MPL(**dict(base, **extra)).set_matmul_precision("bf16").matmul_precision == "bf16"


def test_corner_cases_are_the_corners_of_the_stage_shape_tests():
    from tests.test_stage_shapes_gpu import CORNERS
    theirs = {n: (f, b) for n, f, b in CORNERS}
    assert [c[0] for c in bf16_any_cases.CORNER_CASES] == list(bf16_any_cases.CORNER_NAMES)
    for name, flags, B in bf16_any_cases.CORNER_CASES:
        assert theirs[name] == (flags, B), name
    # and they are ALL the view-token ones
    assert set(bf16_any_cases.CORNER_NAMES) == set(n for n, f, _ in CORNERS if not f.get("FPT_blocks_view_keypoint_tokens"))
