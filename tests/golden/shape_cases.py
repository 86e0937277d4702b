"""Golden cases of models that are not NUM_JOINTS 17 / DIM 32 / HEADS 8 (the supported envelope of mpl_config_supported).

Same record as ``cases.py`` (name, flags, batch, weight seed, input seed); weights are regenerated from ``openmpl_amd.detrng``.
Fixtures: ``make_golden_shapes.py``.
"""
from tests.golden.cases import CHOSEN, FULL


def _c(name, J, d, H, extra, V, B, L, wseed=13, iseed=9):
    f = dict(num_joints=J, embed_dim_ratio=d, num_heads=H, depth=L, num_views=V)
    f.update(extra)
    return dict(name=name, flags=f, batch=B, wseed=wseed, iseed=iseed)


SHAPE_CASES = [
    # a 15-joint skeleton: D_f 480 (unpacked FPT, K % 32 == 0)
    _c("shape_j15_d32_h8_chosen_v4_b6", 15, 32, 8, CHOSEN, 4, 6, 2),
    # E = 640: past the fused LDS tail
    _c("shape_j20_d32_h8_chosen_v4_b4_l12", 20, 32, 8, CHOSEN, 4, 4, 12),
    # the reference's config.py defaults DIM = 2, TRANSFORMER_HEADS = 2: SPT head dim 1, D_f 34, FPT head dim 17
    _c("shape_j17_d2_h2_chosen_v4_b5", 17, 2, 2, CHOSEN, 4, 5, 2),
    # rays as tokens, confidence as third channel, one SPT per view, 3D encoding to rays, at d = 16: D_f 448
    _c("shape_j14_d16_h4_full_v3_b5", 14, 16, 4, FULL, 3, 5, 2),
    # d = 64, E = 1024, deep head
    _c("shape_j16_d64_h16_deep_v3_b5", 16, 64, 16, dict(CHOSEN, deep_head=True, hidden_dim=256), 3, 5, 2),
    # confidence-weighted SPT attention (weighted-then-plain schedule) + kadkhod tail
    _c("shape_j21_d32_h8_confattn_kadkhod_v5_b3", 21, 32, 8,
       dict(CHOSEN, confidence_as_attention_uncertainty_weight=True, head_kadkhod=True, hidden_dim=256), 5, 3, 2),
    # keypoint tokens: 24-token short attention, head dim 8, d = 24
    _c("shape_j12_d24_h3_kptok_v2_b4", 12, 24, 3, dict(CHOSEN, FPT_blocks_view_keypoint_tokens=True), 2, 4, 2),
    # linear weighted mean at E 608
    _c("shape_j19_d32_h8_lwmean_v4_b3", 19, 32, 8, dict(CHOSEN, linear_weighted_mean=True), 4, 3, 2),
]

SHAPE_BY_NAME = {c["name"]: c for c in SHAPE_CASES}
