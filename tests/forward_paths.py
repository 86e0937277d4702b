"""The reachable paths of the model forward, one model per path: shared by the tests that must visit every one of them
(tests/test_memory_contract_gpu.py, tests/test_nonfinite_gpu.py).  Importing this module needs no GPU; _fresh_model does.

FORWARD_MODELS has one model per launch form of the block stack, per SPT form and per tail (view fuse + head variants).  The
library is asked which path a launch took (mpl_block_stack_last_form, mpl_spt_form), and a test fails if the form a case is there
for was not reached.  Batches: the smallest the library's own rule sends to the form on this device (None = search).

FLAG_MODELS has one model per flag set that changes which input channel the forward reads (confidence in the embedding, in the
attention, in the FPT; rays and centers in the positional encodings and as tokens) or which stage exists at all, with the flags of
the golden case of that name, at default precision and with the small-batch engine allowed -- and the confidence-weighted
attention once more on the native-fp32 engine, whose SPT kernel is a different one.
"""
from tests.golden.cases import BY_NAME, CHOSEN, FULL

DEV = "cuda:0"


def _flags(J=17, d=32, H=8, V=4, L=2, **extra):
    return dict(num_joints=J, embed_dim_ratio=d, num_heads=H, depth=L, num_views=V, **extra)


KPTOK = dict(CHOSEN, FPT_blocks_view_keypoint_tokens=True)
# name: (flags, precision, small-batch engine, stack form wanted (None: no stack), SPT form wanted (a set; None: no SPT), batch or None = search)
FORWARD_MODELS = {
    "small_engine_b1": (_flags(V=2, **CHOSEN), "fp32", "auto", "SMALL", {"PACKED"}, 1),
    "team_rows16_direct": (_flags(V=2, **CHOSEN), "fp32", False, "ROWS16_DIRECT", {"PACKED"}, None),
    "team_rows16_ring": (_flags(V=2, **FULL), "fp32", False, "ROWS16", {"PACKED"}, None),
    "team_rows32": (_flags(V=8, **CHOSEN), "fp32", False, "ROWS32", {"PACKED"}, None),
    "team_whole_tile": (_flags(V=5, **CHOSEN), "fp32", False, "TEAMS", {"PACKED"}, None),
    "team_pairs": (_flags(V=8, **CHOSEN), "fp32", False, "PAIRS", {"PACKED"}, None),
    "bf16_team": (_flags(V=4, **CHOSEN), "bf16", False, "TEAMS", {"PACKED"}, None),
    "j15_unpacked": (_flags(J=15, **CHOSEN), "fp32", False, "UNPACKED", {"ANY"}, 6),
    "j15_bf16_any": (_flags(J=15, **CHOSEN), "bf16", "auto", "BF16_ANY", {"ANY"}, 6),
    "grid_d32": (_flags(V=3, **KPTOK), "fp32", "auto", "UNPACKED", {"PACKED"}, 3),
    "grid_wide_head": (_flags(H=2, V=2, **KPTOK), "fp32", "auto", "UNPACKED", {"ANY"}, 3),
    "fp32_mfma": (_flags(V=4, **CHOSEN), "fp32_mfma", False, "UNPACKED", {"STAGED", "FRAGS"}, 3),
    "fuse_any_tail_e640": (_flags(J=20, **CHOSEN), "fp32", False, "UNPACKED", {"ANY"}, 4),
    "linear_weighted_mean": (_flags(V=3, **dict(CHOSEN, linear_weighted_mean=True)), "fp32", "auto", None, {"PACKED"}, 3),
    "deep_head": (_flags(V=3, **dict(CHOSEN, deep_head=True, hidden_dim=64)), "fp32", "auto", None, {"PACKED"}, 3),
    "head_kadkhod": (_flags(V=3, **dict(CHOSEN, head_kadkhod=True, hidden_dim=64)), "fp32", "auto", None, {"PACKED"}, 3),
}

FLAG_CASES = ("chosen_conf3rd", "conf_add", "conf_mult", "conf_attnw", "conf_fpt", "geo3d", "inspatial_learn", "inspatial_geo", "raytoken",
              "multi_spt", "no_spt", "no_fpt")
FLAG_BATCH = 5


def _golden_flags(case):
    return dict(BY_NAME[case + "_v3_b3_l2"]["flags"])


def _flag_forms(case, prec):
    """(stack form, SPT forms) of a flag-tier model at FLAG_BATCH: 15 rows of 544 (1088 with the ray tokens) are far below the
    rows at which the team kernels start, so the small-batch engine takes the stack, at native fp32 too (it reads the nn.Linear
    tensors in place); a model without FPT launches no stack.  The SPT stage is the packed kernel wherever there are packed
    block operands: not at native fp32, and not without SPT blocks, where the native kernel runs the embedding and the norm."""
    stack = None if case == "no_fpt" else "SMALL"
    return stack, ({"STAGED", "FRAGS"} if prec == "fp32_mfma" or case == "no_spt" else {"PACKED"})


# the same record as FORWARD_MODELS
FLAG_MODELS = {case: (_golden_flags(case), "fp32", "auto") + _flag_forms(case, "fp32") + (FLAG_BATCH,) for case in FLAG_CASES}
FLAG_MODELS["conf_attnw_fp32_mfma"] = (_golden_flags("conf_attnw"), "fp32_mfma", "auto") + _flag_forms("conf_attnw", "fp32_mfma") + (FLAG_BATCH,)


def _fresh_model(flags, prec, small):
    from openmpl_amd import detrng
    from openmpl_amd.multiview_mpl import MultiView_MPL
    m = detrng.fill_module_(MultiView_MPL(**flags), seed=11)
    assert m._unsupported is None, m._unsupported
    return m.to(DEV).eval().use_torch_op(False).set_matmul_precision(prec).set_small_batch_engine(small)


def _stack_shape(flags):
    J, d, V = flags["num_joints"], flags["embed_dim_ratio"], flags["num_views"]
    if flags.get("FPT_blocks_view_keypoint_tokens"):
        return J * V, d
    return V, J * d * (2 if flags.get("input_rays_as_token") else 1)
