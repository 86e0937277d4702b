"""Models of the shape-general bf16 engine's parity test (tests/test_bf16_any_gpu.py), shared with tests/test_bf16_any_cpu.py: the
view-token corners of tests/test_stage_shapes_gpu.py::CORNERS plus the shapes the engine was asked for.  (name, flags, batch)."""
from tests.golden.cases import FULL


def _m(J, d, H, V, depth, **extra):
    return dict(num_joints=J, embed_dim_ratio=d, num_heads=H, depth=depth, num_views=V, pose_3d_emb_learnable=True, **extra)


# the view-token models among test_stage_shapes_gpu.CORNERS (same flags, same batch; test_bf16_any_cpu.py checks that they are)
CORNER_NAMES = ("J1", "J64_Df4096", "d128_H1", "hd1", "J64_d1", "rays_4096", "V32_E640")
CORNER_CASES = [
    ("J1", _m(1, 32, 8, 4, 2), 17),
    ("J64_Df4096", _m(64, 64, 8, 2, 1), 2),
    ("d128_H1", _m(17, 128, 1, 3, 2), 2),
    ("hd1", _m(17, 5, 5, 3, 2), 22),
    ("J64_d1", _m(64, 1, 1, 3, 2), 2),
    ("rays_4096", _m(64, 32, 8, 2, 1, input_rays_as_token=True), 2),
    ("V32_E640", _m(20, 32, 8, 32, 2), 2),
]
FURTHER_CASES = [
    ("j15_d32_h8", _m(15, 32, 8, 4, 2), 70),
    ("j20_d32_h8", _m(20, 32, 8, 4, 2), 70),
    ("j17_d2_h2", _m(17, 2, 2, 4, 2), 70),
    ("j16_d64_h16", _m(16, 64, 16, 4, 2), 33),
    ("j17_d32_h16", _m(17, 32, 16, 4, 2), 33),        # width 544, but a head (34) the tuned engine cannot fuse
    ("j15_v1", _m(15, 32, 8, 1, 2), 70),
    ("j15_full", dict(FULL, num_joints=15, embed_dim_ratio=32, num_heads=8, depth=2, num_views=4), 19),
    ("j15_l12_b64", _m(15, 32, 8, 4, 12), 64),
    # width 1632 = 3 x 544 with head 68: the tuned engine fuses this head but packs no LayerNorm operand beyond K = 1088
    ("j34_d48_h24", _m(34, 48, 24, 4, 2), 9),
]
PARITY_CASES = CORNER_CASES + FURTHER_CASES
WEIGHT_SEED, INPUT_SEED = 41, 9

# floors of the gate: the bounds of tests/test_gpu_parity.py::test_bf16_matmul_path (max-scaled, norm-wise)
FLOOR_SHALLOW, FLOOR_DEEP = (1e-3, 7e-4), (3e-3, 2.5e-3)


def floor_of(flags):
    return FLOOR_DEEP if flags["depth"] > 2 else FLOOR_SHALLOW
