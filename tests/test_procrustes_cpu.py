"""Procrustes alignment, CPU side: the float64 restatement of tests/procrustes_cases.py pinned on the golden that the reference's
own PoseUtils.procrustes produced (tests/golden/make_golden_procrustes.py), what the restatement claims about itself, the raising
rules of the public surface (checked before anything touches a device) and the C ABI bookkeeping.  The GPU tests compare the
kernel with the golden and the restatement.

Restatement against golden: both are float64 on the same inputs, so what is left is the round-off of two SVDs and of the
reference's d = 1 - S^2.  Measured here (numpy 1.x / OpenBLAS, printed by the tests): at most 3.1e-13 max-scaled over every field,
case and mode (it is d, where the golden's 1 - S^2 cancels), and 0 on the evaluator's "aligned" fields, which score Z after its
rounding to float32; the gates are those figures x 10, not below 1e-12.
"""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from tests import evaluate_cases as ec
from tests import procrustes_cases as pc

GATE = max(10 * 3.1e-13, 1e-12)
GATE_EVAL = max(10 * 0.0, 1e-12)
KEYS = dict(aligned="Z", d="d", rotation="rotation", scale="scale", translation="translation")


def golden_fields(g, J, scaling, reflection):
    """the stored results of one case and mode as the restatement names them.  J = 3 under 'best': three points are coplanar and
    numpy's sign is arbitrary there; the proper rotation (the documented rule) is what reflection=False stored, with the same d,
    Z and scale (asserted by the generator)."""
    tag = "j%d_%s" % (J, pc.mode_tag(scaling, reflection))
    out = {k: g["%s_%s" % (tag, v)] for k, v in KEYS.items()}
    if J == 3 and reflection == "best":
        proper = "j%d_%s" % (J, pc.mode_tag(scaling, False))
        out["rotation"], out["translation"] = g[proper + "_rotation"], g[proper + "_translation"]
    return out


@pytest.mark.parametrize("J", [3, 4, 17])
def test_restatement_matches_the_reference_golden(J):
    g = pc.golden()
    pred, target = g["j%d_pred" % J], g["j%d_target" % J]
    assert pred.dtype == np.float32 and pred.shape == (6, J, 3)
    worst = 0.0
    for scaling, reflection in pc.MODES:
        res = pc.align(pred, target, scaling=scaling, reflection=reflection)
        ref = golden_fields(g, J, scaling, reflection)
        for k in pc.FIELDS:
            mx, nw = pc.rel_errors(res[k], ref[k])
            worst = max(worst, mx)
            print("J %d %s %s: max-scaled %.3e norm-wise %.3e" % (J, pc.mode_tag(scaling, reflection), k, mx, nw))
            assert mx <= GATE, (J, scaling, reflection, k, mx)
        det = np.linalg.det(res["rotation"])
        if reflection == "best":
            assert (det < 0).tolist() == ([False] * 6 if J == 3 else [b in (1, 4) for b in range(6)])
        else:
            assert ((det < 0) == bool(reflection)).all()
    print("J %d: worst max-scaled %.3e (gate %.1e)" % (J, worst, GATE))


def eval_aligned(batches, mode, joints=None, n_groups=1, output_in_meter=False, not_consider_kp=None, scale=(1, 1, 1), offset=(0, 0, 0)):
    """the "aligned" entry of PoseEvaluator.compute(): the restatement's Z (rounded to float32, as the kernel stores it) scored by
    the absolute pass of tests.evaluate_cases.evaluate against the de-normalised targets"""
    cat = {k: np.concatenate([b[k] for b in batches]) for k in ("output", "target", "conf_3d", "group") if batches[0].get(k) is not None}
    J = cat["output"].shape[1]
    u = np.arange(J) if joints is None else np.asarray([int(k) % J for k in joints])
    Z = pc.align(cat["output"], cat["target"], conf=cat.get("conf_3d"), joints=joints, scaling=mode == "similarity", scale=scale,
                 offset=offset)["aligned"].astype(np.float32)
    sc, of = np.asarray(scale, dtype=np.float32), np.asarray(offset, dtype=np.float32)
    conf = cat["conf_3d"].reshape(Z.shape[0], -1)[:, u] if "conf_3d" in cat else None
    return ec.evaluate(Z[:, u, :], (cat["target"] * sc + of)[:, u, :], conf, False, output_in_meter, not_consider_kp, cat.get("group"),
                       n_groups)


def test_evaluator_fields_of_the_restatement_match_the_golden():
    """the golden's Z scored by evaluate() against the restatement's Z scored the same way"""
    g = pc.golden()
    worst = 0.0
    for J in (4, 17):
        pred, target = g["j%d_pred" % J], g["j%d_target" % J]
        for mode, tag in (("similarity", "s"), ("rigid", "r")):
            mine = eval_aligned([dict(output=pred, target=target)], mode)
            ref = ec.evaluate(g["j%d_%s_best_Z" % (J, tag)].astype(np.float32), target, None, False, False)
            for f in ec.FIELDS:
                mx, _ = pc.rel_errors(mine[f], ref[f])
                worst = max(worst, mx)
                print("J %d %s %s: max-scaled %.3e" % (J, mode, f, mx))
                assert mx <= GATE_EVAL, (J, mode, f, mx)
            assert mine["n_samples"] == 6
    print("worst %.3e (gate %.1e)" % (worst, GATE_EVAL))


def small_rotation(axis, angle):
    k = np.zeros((3, 3))
    k[(axis + 1) % 3, (axis + 2) % 3], k[(axis + 2) % 3, (axis + 1) % 3] = -1.0, 1.0
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)


@pytest.mark.parametrize("scaling", [True, False])
def test_restatement_minimises_the_residual(scaling):
    """no small rotation on top of R lowers d (scale and translation re-fitted as the reference fits them)"""
    case = pc.similarity_case(8, 17, seed=2, mirror=(3,))
    conf = np.ones((8, 17), np.float32)
    conf[2, 5:] = 0.0                                   # 5 joints take part
    res = pc.align(case["pred"], case["target"], conf=conf, scaling=scaling, reflection=False)
    for b in range(8):
        take = np.nonzero(conf[b] > 0)[0]
        A, Bp = case["target"][b].astype(np.float64)[take], case["pred"][b].astype(np.float64)[take]
        A0, B0 = A - A.mean(0), Bp - Bp.mean(0)
        ssX = (A0 ** 2).sum()

        def d_of(R):
            BR = B0 @ R
            s = (A0 * BR).sum() / (BR ** 2).sum() if scaling else 1.0
            return ((s * BR - A0) ** 2).sum() / ssX

        base = d_of(res["rotation"][b])
        assert abs(base - res["d"][b]) <= 1e-12 * max(base, 1e-3)
        for axis in range(3):
            for angle in (1e-6, -1e-6, 1e-3, -1e-3, 0.1, -0.1):
                assert d_of(res["rotation"][b] @ small_rotation(axis, angle)) >= base * (1 - 1e-12), (b, axis, angle)


def test_restatement_rules_for_participation_and_degenerate_poses():
    case = pc.similarity_case(6, 17, seed=3)
    pred, target = case["pred"].copy(), case["target"].copy()
    conf = np.ones((6, 17), np.float32)
    conf[0, 3:] = 0.0                                   # exactly 3 joints: fine
    conf[1, 2:] = 0.0                                   # 2 joints: NaN
    conf[2, 4], conf[2, 5], conf[2, 6] = np.nan, np.inf, -1.0
    target[3] = target[3, :1]                           # all joints equal
    pred[4] = np.float32([1.5, -2.25, 0.5]) + np.arange(17, dtype=np.float32)[:, None] * np.float32([0.25, 0.5, -0.125])      # collinear, exactly
    res = pc.align(pred, target, conf=conf)
    bad = [1, 3, 4]
    for k in pc.FIELDS:
        isn = np.isnan(res[k]).reshape(6, -1)
        assert isn[bad].all() and not isn[[0, 2, 5]].any(), k
    dropped = conf.copy()
    dropped[2, 4:7] = 0.0
    again = pc.align(pred, target, conf=dropped)
    for k in pc.FIELDS:
        np.testing.assert_array_equal(res[k], again[k])
    # a selection is the same as the confidences that leave those joints (Z still holds every joint)
    sel = [16, 2, 9, 4]
    c = np.zeros((6, 17), np.float32)
    c[:, sel] = 1.0
    a, b = pc.align(pred, target, joints=sel), pc.align(pred, target, conf=c)
    for k in pc.FIELDS:
        np.testing.assert_allclose(a[k], b[k], rtol=1e-10, atol=1e-12, equal_nan=True)
    # coplanar target: the proper rotation under 'best', whatever numpy's sign
    flat = target.copy()
    flat[..., 2] = 0.0
    r = pc.align(pred[[0, 2, 5]], flat[[0, 2, 5]])
    np.testing.assert_allclose(np.linalg.det(r["rotation"]), 1.0, rtol=1e-12)
    # de-normalisation happens before the fit, on both tensors
    sc, of = (2.0, 3.0, 0.5), (0.1, 0.0, -0.2)
    x = pc.align(pred, target, scale=sc, offset=of)
    y = pc.align(pred.astype(np.float64) * sc + of, target.astype(np.float64) * sc + of)
    np.testing.assert_allclose(x["aligned"], y["aligned"], rtol=1e-6, atol=1e-6, equal_nan=True)


def test_procrustes_align_is_exported_and_checks_its_arguments_before_any_device():
    import openmpl_amd
    from openmpl_amd import procrustes
    assert openmpl_amd.procrustes_align is procrustes.procrustes_align
    align = openmpl_amd.procrustes_align
    B, J = 4, 17
    x = torch.zeros(B, J, 3)
    with pytest.raises(RuntimeError, match="no CPU path: pred"):
        align(x, x)
    with pytest.raises(RuntimeError, match=r"pred: expected shape \(B,J,3\)"):
        align(x[..., :2], x)
    with pytest.raises(RuntimeError, match="target: expected shape"):
        align(x, x[:, :16])
    with pytest.raises(RuntimeError, match="conf: expected shape"):
        align(x, x, conf=torch.ones(B, J - 1))
    with pytest.raises(RuntimeError, match=r"float32 tensors required \(pred"):
        align(x.double(), x)
    with pytest.raises(RuntimeError, match=r"float32 tensors required \(target"):
        align(x, x.half())
    with pytest.raises(RuntimeError, match=r"float32 tensors required \(conf"):
        align(x, x, conf=torch.ones(B, J, dtype=torch.float64))
    for bad in ("worst", None, 1, 0):
        with pytest.raises(ValueError, match="reflection"):
            align(x, x, reflection=bad)
    with pytest.raises(IndexError, match="joint index 17"):
        align(x, x, joints=[0, 17])
    with pytest.raises(IndexError, match="joint index -18"):
        align(x, x, joints=[-18])
    with pytest.raises(RuntimeError, match="3 values"):
        align(x, x, scale=(1.0, 2.0))
    with pytest.raises(RuntimeError, match="no CPU path: pred"):
        align(x, x, joints=[-1, 0, 5], conf=torch.ones(B, J, 1), reflection=True, scaling=False)      # all legal but the device


def test_pose_evaluator_rejects_other_aligned_values():
    from openmpl_amd import PoseEvaluator
    from openmpl_amd.evaluate import ALIGNED
    assert sorted(k for k in ALIGNED if k) == ["rigid", "similarity"] and None in ALIGNED
    for bad in ("affine", True, 1, ""):
        with pytest.raises(ValueError, match="aligned must be"):
            PoseEvaluator(17, aligned=bad)


def test_symbol_is_in_the_header_and_the_binding_with_matching_arity():
    import os
    from openmpl_amd import cabi
    assert "mpl_procrustes_align" in cabi.EXPORTS and cabi.ABI_VERSION == 14
    assert (cabi.REFLECT_BEST, cabi.REFLECT_OFF, cabi.REFLECT_ON) == (0, 1, 2)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mpl_hip.h")).read()
    m = re.search(r"\bint mpl_procrustes_align\(([^;]*)\);", header)
    assert m, "mpl_procrustes_align is not declared in include/mpl_hip.h"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert len(params) == 17 and params[0] == "const float *pred" and params[-1] == "void *stream"
    lib = cabi.load()
    assert len(lib.mpl_procrustes_align.argtypes) == len(params)
    assert lib.mpl_procrustes_align.restype is C.c_int
    # the refusals need no device: they come before any launch
    f3 = (C.c_float * 3)(1, 1, 1)
    one = C.c_void_p(8)         # never dereferenced by a refused call
    assert lib.mpl_procrustes_align(None, one, None, None, 0, f3, f3, 1, 0, 4, 17, one, one, None, None, None, None) == -1
    assert lib.mpl_procrustes_align(one, one, None, None, 0, None, None, 1, 3, 4, 17, one, one, None, None, None, None) == -1
    assert lib.mpl_procrustes_align(one, one, None, None, 0, None, None, 1, 0, 4, 17, None, None, one, None, None, None) == -1
    assert lib.mpl_procrustes_align(one, one, None, (C.c_int * 2)(0, 17), 2, None, None, 1, 0, 4, 17, one, one, None, None, None, None) == -1
    assert lib.mpl_procrustes_align(one, one, None, None, 0, None, None, 1, 0, 0, 17, one, one, None, None, None, None) == -1
    assert lib.mpl_procrustes_align(one, one, None, None, 0, None, None, 1, 0, 4, 65, one, one, None, None, None, None) == -2
    assert lib.mpl_procrustes_align(one, one, None, (C.c_int * 65)(), 65, None, None, 1, 0, 4, 17, one, one, None, None, None, None) == -2
    assert lib.mpl_procrustes_align(one, one, None, None, 0, None, None, 1, 0, 1 << 26, 17, one, one, None, None, None, None) == -2
