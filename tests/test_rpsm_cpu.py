"""The RPSM restatement (tests/rpsm_cases.py) against the reference-generated golden, the conditions its cases are built under, the
grid order, the closed-form crop transform, and the envelope of openmpl_amd.rpsm, which raises before anything is loaded."""
import os
import re

import numpy as np
import pytest
import torch

from tests import rpsm_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("tag", ["g4", "g8", "g8_dist"])
def test_restatement_matches_the_reference_golden(tag):
    """bins equal, poses within 1e-9 world units (millimetres here); the 16^3 case, 20 s of numpy, is held to the same when the golden
    is made (make_golden_rpsm.py asserts it) and checked below through its recorded margins"""
    g = rc.golden()
    inp, ref, attempt = rc.case(tag)
    assert attempt == int(g[tag + "_attempt"])
    assert np.array_equal(ref["bins"], g[tag + "_bins"])
    diff = np.abs(ref["poses"] - g[tag + "_poses"]).max()
    print("%s: poses differ from the reference's by at most %.2e" % (tag, diff))
    assert diff <= 1e-9
    first = rc.grid(inp["kw"]["grid_size"], inp["root_center"][0].astype(np.float64), inp["kw"]["first_nbins"])
    u = rc.unary(inp["hm"][0][:, [0, 9]], [first], inp["center"][0], inp["scale"][0], inp["cams"], inp["image_size"], inp["dist"])
    rel = np.abs(u - g[tag + "_unary_0_9"]).max() / np.abs(g[tag + "_unary_0_9"]).max()
    print("%s: unary terms differ from the reference's by at most %.2e of their maximum" % (tag, rel))
    assert rel <= 1e-12


def test_the_recorded_16_cubed_case_met_both_conditions():
    g = rc.golden()
    a, b = g["g16_margins"]
    print("16^3: boundary distance %.2e, on-path margin %.2e" % (a, b))
    assert a >= rc.MARGIN_A and b >= rc.MARGIN_B
    assert g["g16_bins"].shape == (2, 11, 17) and g["g16_poses"].shape == (2, 17, 3)
    assert rc.boundary_distance(rc.attempt_inputs("g16", int(g["g16_attempt"]))) == a


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_conditions_hold_for_every_gpu_case(name):
    inp, ref, attempt = rc.case(name)                      # raises when no seed meets them
    a, b = rc.boundary_distance(inp), ref["margin"]
    print("%s: attempt %d, boundary distance %.2e, on-path margin %.2e" % (name, attempt, a, b))
    assert a >= rc.MARGIN_A and b >= rc.MARGIN_B
    assert ref["bins"].shape == (inp["hm"].shape[0], 1 + inp["kw"]["recur_depth"], len(inp["parents"]))


@pytest.mark.parametrize("name", ["n2", "n3", "n5", "single"])
def test_small_grids_land_within_a_first_round_cell(name):
    """a grid coarser than the tolerance allows forbids every pair and degenerates to bin 0: the small bin counts get a small box"""
    inp, ref, _ = rc.case(name)
    step = inp["kw"]["grid_size"] / (inp["kw"]["first_nbins"] - 1)
    err = np.abs(ref["first"] - inp["truth"]).max()
    print("%s: first round within %.2f cells of the pose" % (name, err / step))
    assert err <= step
    assert (ref["energy"] > 0).all()                       # not the degenerate answer: some pair was allowed on every edge


def test_the_default_case_finds_the_pose():
    inp, ref, _ = rc.case("n8")
    err = np.linalg.norm(ref["poses"] - inp["truth"], axis=-1)
    print("8^3, depth 10: mean joint error %.1f mm, worst %.1f mm" % (err.mean(), err.max()))
    assert err.max() < 0.5 * np.sqrt(3.0) * 2000.0 / 7


def test_grid_index_order():
    """y is the slowest axis and z the fastest: bin (iy*n + ix)*n + iz is (l[ix] + cx, l[iy] + cy, l[iz] + cz)"""
    n, size, c = 4, 600.0, np.array([10.0, 200.0, 3000.0])
    g = rc.grid(size, c, n)
    l = np.linspace(-size / 2, size / 2, n)
    for iy in range(n):
        for ix in range(n):
            for iz in range(n):
                assert np.array_equal(g[(iy * n + ix) * n + iz], [l[ix] + c[0], l[iy] + c[1], l[iz] + c[2]])
    assert l[-1] == size / 2 and l[1] == 1 * (size / (n - 1)) + -size / 2


def test_closed_form_crop_against_the_affine_solve():
    """get_affine_transform(center, scale, 0, image_size) as the reference builds it (float32 anchor points, then the float64 solve of
    the stub cv2.getAffineTransform of the golden scripts), applied to points, against the closed form"""
    worst = 0.0
    for seed in range(4):
        inp = rc.inputs(seed=seed, V=4)
        for v in range(4):
            center, scale = inp["center"][0, v], inp["scale"][0, v]
            iw, ih = inp["image_size"]
            src_w = np.float64(scale[0]) * 200.0
            src = np.zeros((3, 2), np.float32)
            dst = np.zeros((3, 2), np.float32)
            src[0] = center
            src[1] = center + np.array([0.0, src_w * -0.5])
            dst[0] = [iw * 0.5, ih * 0.5]
            dst[1] = np.array([iw * 0.5, ih * 0.5]) + np.array([0.0, iw * -0.5], np.float32)
            src[2] = src[1] + np.array([-(src[0] - src[1])[1], (src[0] - src[1])[0]], np.float32)
            dst[2] = dst[1] + np.array([-(dst[0] - dst[1])[1], (dst[0] - dst[1])[0]], np.float32)
            M = np.linalg.solve(np.concatenate([src.astype(np.float64), np.ones((3, 1))], axis=1), dst.astype(np.float64)).T
            px = np.asarray(center, np.float64) + rc.detrng.uniform(seed, "crop.%d" % v, (50, 2), -400.0, 400.0)
            via = (np.concatenate([px, np.ones((50, 1))], axis=1) @ M.T) * np.array([64.0, 64.0]) / np.array([iw, ih])
            worst = max(worst, np.abs(via - rc.crop_cells(px, center, scale[0], (iw, ih), 64, 64)).max())
    print("closed form vs affine solve: at most %.2e cells" % worst)
    assert worst <= 1e-10


def _cpu_args(J=17, B=1, V=2, H=8, W=8):
    return dict(heatmaps=torch.zeros(B, V, J, H, W), center=torch.zeros(B, V, 2), scale=torch.ones(B, V, 2), cams=torch.zeros(V, 16, dtype=torch.float64),
                image_size=(256.0, 256.0), root_center=torch.zeros(B, 3), limb_length=torch.ones(J))


@pytest.mark.parametrize("change", [dict(first_nbins=1), dict(first_nbins=17), dict(first_nbins=8.5), dict(recur_nbins=1), dict(recur_nbins=5),
                                    dict(recur_depth=-1), dict(recur_depth=17), dict(parents=[0] * 17), dict(parents=[-1] * 17),
                                    dict(parents=[-1, 2, 1] + [0] * 14), dict(parents=[-1, 0, 17] + [0] * 14), dict(parents=[-1, 0]),
                                    dict(grid_size=0.0), dict(tolerance=-1.0), dict(image_size=(0.0, 256.0)),
                                    dict(limb_length=torch.ones(16)), dict(root_center=torch.zeros(2, 3)), dict(distortion=torch.zeros(2, 4, dtype=torch.float64)),
                                    dict(cams=torch.zeros(2, 16)), dict(heatmaps=torch.zeros(1, 2, 17, 8, 8, dtype=torch.float64)),
                                    dict(heatmaps=torch.zeros(1, 2, 17, 1, 8)), dict(heatmaps=torch.zeros(2, 17, 8, 8))],
                         ids=lambda c: "%s=%s" % next(iter((k, getattr(v, "shape", v)) for k, v in c.items())))
def test_envelope_violations_raise_before_the_library_is_loaded(change, monkeypatch):
    import openmpl_amd
    from openmpl_amd import cabi

    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(cabi, "load", no_load)
    args = _cpu_args()
    args.update(change)
    with pytest.raises(ValueError):
        openmpl_amd.rpsm(**args)


def test_more_joints_or_views_than_the_envelope():
    import openmpl_amd
    args = _cpu_args(J=65)
    with pytest.raises(ValueError):
        openmpl_amd.rpsm(parents=[-1] + [0] * 64, **args)
    args = _cpu_args(J=3, V=33)
    with pytest.raises(ValueError):
        openmpl_amd.rpsm(parents=[-1, 0, 1], **args)
    with pytest.raises(ValueError):                      # the default tree is the 17-joint body
        openmpl_amd.rpsm(**_cpu_args(J=3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        openmpl_amd.rpsm(**_cpu_args())


def test_the_module_is_the_function_and_documents_its_launches():
    import openmpl_amd
    from openmpl_amd import cabi
    from openmpl_amd import rpsm as mod
    assert callable(openmpl_amd.rpsm) and openmpl_amd.rpsm is mod and mod.RPSMResult._fields == ("poses", "bins", "energy")
    assert mod.HUMAN_BODY_PARENTS == rc.BODY
    assert mod.launches() == 7 and mod.launches([-1]) == 2 and mod.launches([-1, 0, 1]) == 4 and mod.launches([-1, 0, 0, 0, 0]) == 3
    assert "7 for the default tree" in mod.rpsm.__doc__
    assert "mpl_rpsm" in cabi.EXPORTS and "mpl_rpsm_workspace_bytes" in cabi.EXPORTS
    header = open(os.path.join(ROOT, "include", "mpl_hip.h")).read()
    assert re.search(r"int mpl_rpsm\(", header) and re.search(r"size_t mpl_rpsm_workspace_bytes\(", header)
    assert "rpsm.hip" in __import__("openmpl_amd.build", fromlist=["SOURCES"]).SOURCES
