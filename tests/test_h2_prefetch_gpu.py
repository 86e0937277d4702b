"""GPU tests of the cross-phase W prefetch of the whole-tile chain form (h2_stack_kernel, openmpl_amd/csrc/h2_phase.hpp): a phase
requests the W pieces of the next phase's first stages under its own tail stages, and the next phase starts on a rotated ring.
That is scheduling only -- k order, product order and every stored value are those of a phase that fills its own ring -- so the
poses must be bitwise those of the per-GEMM launch form (mpl_x3_stack_mode bit 0, what MPL_X3_LAUNCHES=1 sets), which has no
phase to prefetch across.  Depth 2 = 3 block applications = 12 phases: every phase-kind boundary and the tile-to-tile boundary."""
import pytest
import torch

from openmpl_amd import cabi, detrng
from openmpl_amd.multiview_mpl import MultiView_MPL
from oracle import mpl_oracle
from tests.golden.cases import BY_NAME

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

PER_GEMM = 1 | 8                       # bit 0: one launch per GEMM; bit 3: the team engines also at <= 80 rows
WHOLE = (1 << 5) | (1 << 1) | 8        # whole-tile teams, one row tile per step: h2_stack_kernel whatever the shape
DEFAULT = 8                            # the form rule picks the persistent kernel

_MODELS = {}


def _model(flagset, V):
    """Depth-2 model of a flag set at V views with the deterministic weights of the goldens (seed 11), built once per module."""
    if (flagset, V) not in _MODELS:
        flags = dict(BY_NAME[flagset + "_v4_b8_l2"]["flags"], num_views=V)
        sd = {k: torch.from_numpy(v) for k, v in detrng.make_state_dict(mpl_oracle.param_shapes(flags), seed=11).items()}
        m = MultiView_MPL(**flags)
        m.load_state_dict(sd, strict=True)
        _MODELS[(flagset, V)] = m.to(DEV).eval()
    return _MODELS[(flagset, V)]


def _big_inputs(B, V, seed):
    p, r, c = detrng.make_inputs(B, V, seed=seed)
    mk = lambda lst: [torch.from_numpy(x).to(DEV) for x in lst]
    return mk(p), mk(r), mk(c)


def _poses_by_mode(m, B, V, prec, modes):
    lib = cabi.load()
    P, R, Cn = _big_inputs(B, V, 4321)
    outs = {}
    m.set_matmul_precision(prec)
    try:
        with torch.no_grad():
            for tag, mode in modes:
                cabi.check(lib.mpl_x3_stack_mode(mode), "stack mode")
                outs[tag] = m(P, rays=R, centers=Cn).clone()
                torch.cuda.synchronize()
                outs[tag + ":form"] = lib.mpl_block_stack_last_form()
    finally:
        cabi.check(lib.mpl_x3_stack_mode(0), "stack mode")
        m.set_matmul_precision("fp32")
    assert not cabi.device_error()
    return outs


@pytest.mark.parametrize("flagset,V,B,prec", [
    ("chosen", 4, 16, "fp32"),         # one row tile
    ("chosen", 4, 17, "fp32"),         # ragged second tile
    ("chosen", 4, 40, "fp32"),         # several teams
    ("chosen", 3, 8, "fp32"),          # LDS attention epilogue: the qkv phase must not prefetch into the ring it reuses
    ("chosen", 8, 8, "fp32"),          # register attention of eight views
    ("full", 4, 16, "fp32"),           # D = 1088: the other slot rotations
    ("chosen", 8, 8, "bf16"),          # NP = 1: a stage is a pair of k-tiles, the k-tile count is padded
])
def test_prefetching_chain_is_bitwise_the_per_gemm_form(flagset, V, B, prec):
    m = _model(flagset, V)
    outs = _poses_by_mode(m, B, V, prec, (("gemm", PER_GEMM), ("whole", WHOLE), ("default", DEFAULT), ("whole2", WHOLE)))
    assert outs["gemm:form"] == cabi.FORM_PER_GEMM and outs["whole:form"] == cabi.FORM_TEAMS, outs
    assert torch.isfinite(outs["gemm"]).all()
    for tag in ("whole", "default", "whole2"):
        d = float((outs["gemm"] - outs[tag]).abs().max())
        print("%s V=%d B=%d %s: %s vs per-GEMM max |d| = %.3e" % (flagset, V, B, prec, tag, d))
    for tag in ("whole", "default", "whole2"):
        assert torch.equal(outs["gemm"], outs[tag]), "%s differs from the per-GEMM form: max |d| = %.3e" % (
            tag, float((outs["gemm"] - outs[tag]).abs().max()))


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_a_team_that_walks_two_tiles_prefetches_across_the_tile_boundary(prec):
    """4120 rows = 65 row tiles for the 64 teams of a 256-CU device at D = 544 (fewer compute units: more tiles per team): team 0
    walks tiles 0 and 64, and the last phase of the first prefetches the qkv weights of the second."""
    lib = cabi.load()
    V, B = 4, 1030
    n_tiles, cap = (B * V + 63) // 64, torch.cuda.get_device_properties(0).multi_processor_count // 4
    assert n_tiles > min(cap, 1024 // 4), "every team owns one tile: the case does not cross a tile boundary on this device"
    m = _model("chosen", V)
    outs = _poses_by_mode(m, B, V, prec, (("gemm", PER_GEMM), ("whole", WHOLE)))
    assert outs["whole:form"] == cabi.FORM_TEAMS, outs
    assert torch.isfinite(outs["gemm"]).all()
    d = float((outs["gemm"] - outs["whole"]).abs().max())
    print("two tiles per team, %s: max |d| = %.3e" % (prec, d))
    assert torch.equal(outs["gemm"], outs["whole"]), "max |d| = %.3e" % d
