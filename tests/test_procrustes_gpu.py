"""Procrustes alignment on the GPU (openmpl_amd/procrustes.py, csrc/procrustes.hip, PoseEvaluator(aligned=...)) against the
reference's golden and the float64 restatement of tests/procrustes_cases.py.

Bound everywhere: the parity rule of DESIGN.md section 2, max|d| <= 1e-4 max|ref| and ||d||_2 <= 1e-4 ||ref||_2.  The kernel
computes in fp64 and rounds once to fp32, so it sits near 1e-7 (measured on an MI355X: at most 5.5e-8 max-scaled against the
golden).  Repeated runs and two batchings are compared bitwise.  Outputs lie between canary regions and
start as canaries, so an element the kernel skips fails too.  The evaluator's "aligned" fields are held to rtol 1e-5 against the
restatement, the bound tests/test_evaluate_gpu.py uses for its own passes.

Before every assertion on an error the figures are printed (pytest -s shows them).
"""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

from tests import evaluate_cases as ec
from tests import procrustes_cases as pc
from tests.test_procrustes_cpu import eval_aligned, golden_fields

pytestmark = pytest.mark.gpu
TOL = 1e-4
GUARD, CANARY = 4096, -12345.0
E_INVALID, E_UNSUPPORTED = -1, -2
REFLECT = {"best": 0, False: 1, True: 2}
SHAPES = dict(aligned=lambda B, J: (B, J, 3), d=lambda B, J: (B,), rotation=lambda B, J: (B, 3, 3), scale=lambda B, J: (B,),
              translation=lambda B, J: (B, 3))


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _assert_parity(got, ref, what):
    mx, nw = pc.rel_errors(got, ref)
    print("%s: max-scaled %.3e norm-wise %.3e" % (what, mx, nw))
    assert mx <= TOL and nw <= TOL, "%s: max-scaled %.3e norm-wise %.3e (tol %.0e)" % (what, mx, nw, TOL)
    return mx


def _launches(fn):
    """(result, number of kernels launched while fn ran)."""
    from openmpl_amd import cabi
    torch.cuda.synchronize()
    cabi.profile_start()
    try:
        res = fn()
    finally:
        torch.cuda.synchronize()
        counts = cabi.profile_stop()
    return res, sum(n for _, n in counts.values())


class Guarded:
    """n floats between two canary regions, canaries themselves until written"""

    def __init__(self, *shape):
        self.n = int(np.prod(shape))
        self.all = torch.full((self.n + 2 * GUARD,), CANARY, dtype=torch.float32, device="cuda")
        self.t = self.all[GUARD:GUARD + self.n].view(*shape)

    def intact(self):
        return bool((self.all[:GUARD] == CANARY).all()) and bool((self.all[GUARD + self.n:] == CANARY).all())

    def untouched(self):
        return bool((self.all == CANARY).all())


def raw(pred, target, B, J, conf=None, sel=None, scale=None, offset=None, scaling=True, reflection="best", outputs=pc.FIELDS):
    """the C ABI on guarded outputs -> (return code, {field: Guarded}); fields not in `outputs` are passed as NULL"""
    from openmpl_amd import cabi
    out = {k: Guarded(*SHAPES[k](B, J)) for k in pc.FIELDS}
    ptr = lambda k: out[k].t.data_ptr() if k in outputs else None      # noqa: E731
    f3 = lambda v: None if v is None else (C.c_float * 3)(*v)         # noqa: E731
    rc = cabi.load().mpl_procrustes_align(pred.data_ptr(), target.data_ptr(), None if conf is None else conf.data_ptr(),
                                          None if sel is None else (C.c_int * len(sel))(*sel), 0 if sel is None else len(sel),
                                          f3(scale), f3(offset), int(scaling), REFLECT[reflection], B, J, ptr("aligned"), ptr("d"),
                                          ptr("rotation"), ptr("scale"), ptr("translation"), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out


@functools.lru_cache(maxsize=None)
def golden():
    return pc.golden()


# ----------------------------------------------------------------------------- the reference's golden
@pytest.mark.parametrize("J", [3, 4, 17])
def test_all_six_modes_match_the_reference_golden(J):
    from openmpl_amd import procrustes_align
    g = golden()
    pred, target = g["j%d_pred" % J], g["j%d_target" % J]
    worst = 0.0
    for scaling, reflection in pc.MODES:
        res = procrustes_align(_dev(pred), _dev(target), scaling=scaling, reflection=reflection)
        ref = golden_fields(g, J, scaling, reflection)
        mine = pc.align(pred, target, scaling=scaling, reflection=reflection)
        for k in pc.FIELDS:
            t = getattr(res, k)
            assert t.dtype == torch.float32 and t.is_cuda and tuple(t.shape) == SHAPES[k](6, J)
            what = "J %d %s %s" % (J, pc.mode_tag(scaling, reflection), k)
            worst = max(worst, _assert_parity(_np(t), ref[k], "golden " + what))
            _assert_parity(_np(t), mine[k], "restatement " + what)
    print("J %d: worst max-scaled error against the golden %.3e" % (J, worst))


# ----------------------------------------------------------------------------- shapes where the indexing can go wrong
def grid_case(B, J):
    """selection, confidences and per-axis de-normalisation at once.  J = 3: all joints, nothing masked (3 is the minimum)."""
    rs = np.random.RandomState(B * 100 + J)
    case = pc.similarity_case(B, J, seed=5, mirror=tuple(range(1, B, 7)))
    sel, conf, nan_poses = None, None, []
    if J > 3:
        sel = [int(k) for k in rs.permutation(J - 1)[:max(6, J - 5)]] + [-1]    # reordered, some dropped, one negative (wraps)
        conf = rs.uniform(0.1, 1.0, size=(B, J)).astype(np.float32)
        wrapped = [k % J for k in sel]
        for b in range(0, B, 3):                    # exactly 3 of the selected joints left
            conf[b, wrapped[3:]] = 0.0
            conf[b, wrapped[:3]] = 0.5
        for b in range(1, B, 5):                    # 2 left: the pose is NaN
            if b % 3 == 0:
                continue
            conf[b, wrapped[2:]] = [0.0, -1.0, np.nan, np.inf][b % 4]
            conf[b, wrapped[:2]] = 0.5
            nan_poses.append(b)
    return case, sel, conf, nan_poses


@pytest.mark.parametrize("B,J", list(itertools.product([1, 63, 64, 65, 130], [3, 17, 64])))
def test_shape_grid_against_float64(B, J):
    case, sel, conf, nan_poses = grid_case(B, J)
    sc, of = (2.0, 3.0, 0.5), (0.1, 0.0, -0.2)
    scaling, reflection = [(True, "best"), (False, False), (True, True)][(B + J) % 3]
    wrapped = None if sel is None else [k % J for k in sel]
    rc, out = raw(_dev(case["pred"]), _dev(case["target"]), B, J, _dev(conf), wrapped, sc, of, scaling, reflection)
    assert rc == 0 and all(o.intact() for o in out.values())
    ref = pc.align(case["pred"], case["target"], conf=conf, joints=sel, scaling=scaling, reflection=reflection, scale=sc, offset=of)
    for k in pc.FIELDS:
        _assert_parity(_np(out[k].t), ref[k], "B %d J %d %s" % (B, J, k))
    isn = np.isnan(_np(out["d"].t))
    if J > 3:
        assert set(nan_poses) <= set(np.nonzero(isn)[0].tolist()) and (len(nan_poses) > 0 or B == 1)
    else:
        assert not isn.any()
    # the poses a confidence made NaN leave the others as they are without it: bitwise
    if nan_poses:
        fine = conf.copy()
        fine[nan_poses] = 1.0
        rc, out2 = raw(_dev(case["pred"]), _dev(case["target"]), B, J, _dev(fine), wrapped, sc, of, scaling, reflection)
        keep = np.ones(B, bool)
        keep[nan_poses] = False
        for k in pc.FIELDS:
            assert rc == 0 and np.array_equal(_np(out[k].t)[keep], _np(out2[k].t)[keep], equal_nan=True), k
            assert not np.isnan(_np(out2[k].t)[nan_poses]).any(), k


def test_python_entry_point_returns_what_the_c_abi_writes_in_one_launch():
    from openmpl_amd import procrustes_align
    B, J = 65, 17
    case, sel, conf, _ = grid_case(B, J)
    p, t, c = _dev(case["pred"]), _dev(case["target"]), _dev(conf)
    res, n = _launches(lambda: procrustes_align(p, t, conf=c, joints=sel, scaling=False, reflection=True, scale=2.0, offset=(1, 2, 3)))
    assert n == 1 and res._fields == pc.FIELDS
    rc, out = raw(p, t, B, J, c, [k % J for k in sel], (2.0, 2.0, 2.0), (1.0, 2.0, 3.0), False, True)
    for k in pc.FIELDS:
        assert rc == 0 and np.array_equal(_np(getattr(res, k)), _np(out[k].t), equal_nan=True), k
    r3, _ = _launches(lambda: procrustes_align(p, t, conf=c.reshape(B, J, 1), joints=sel, scaling=False, reflection=True, scale=2.0,
                                               offset=(1, 2, 3)))
    assert np.array_equal(_np(r3.aligned), _np(res.aligned), equal_nan=True)
    with pytest.raises(NotImplementedError):
        procrustes_align(torch.zeros(2, 65, 3, device="cuda"), torch.zeros(2, 65, 3, device="cuda"))
    with pytest.raises(RuntimeError, match="no CPU path: target"):
        procrustes_align(p, t.cpu())


# ----------------------------------------------------------------------------- a constructed exact case
def test_exact_similarities_are_recovered_with_a_vanishing_residual():
    """predictions that are fp32-rounded similarities of the targets: what is left of d is the rounding of the predictions, at
    most 2^-24 of a coordinate (up to 3 here: a pose about 1 m across at the origin, scaled by up to 2 and shifted by up to 1)
    over the spread of the pose (0.29 per axis and joint, times the scale): d <= (2^-24 * 3 / 0.29)^2 ~ 4e-13"""
    from openmpl_amd import procrustes_align
    B, J = 65, 17
    case = pc.similarity_case(B, J, seed=9, exact=True, mirror=(2, 40), room=0.0)
    res = procrustes_align(_dev(case["pred"]), _dev(case["target"]))
    d = _np(res.d)
    ref = pc.align(case["pred"], case["target"])
    print("exact fit: d kernel max %.3e restatement max %.3e" % (d.max(), ref["d"].max()))
    assert (d >= 0).all() and d.max() <= 1e-12
    _assert_parity(d, ref["d"], "exact fit: d")
    # aligned = s_fit * pred R_fit + t_fit undoes pred = s * target R + t
    _assert_parity(_np(res.scale), 1.0 / case["s"], "exact fit: scale")
    _assert_parity(_np(res.rotation), np.transpose(case["R"], (0, 2, 1)), "exact fit: rotation")
    _assert_parity(_np(res.aligned), case["target"], "exact fit: aligned")
    used = _np(res.scale)[:, None, None] * np.einsum("bjx,bxy->bjy", case["pred"].astype(np.float64), _np(res.rotation).astype(np.float64)) \
        + _np(res.translation)[:, None, :]
    _assert_parity(_np(res.aligned), used, "exact fit: the reported transform is the one used")
    det = np.linalg.det(_np(res.rotation).astype(np.float64))
    assert sorted(np.nonzero(det < 0)[0].tolist()) == [2, 40]
    rigid = procrustes_align(_dev(case["pred"]), _dev(case["target"]), scaling=False)
    assert np.array_equal(_np(rigid.scale), np.ones(B, np.float32))
    _assert_parity(_np(rigid.rotation), ref["rotation"], "rigid: the rotation does not depend on scaling")


# ----------------------------------------------------------------------------- invariants
def test_rotations_are_orthogonal_and_the_reflection_modes_decide_the_determinant():
    from openmpl_amd import procrustes_align
    B, J = 130, 17
    case = pc.similarity_case(B, J, seed=11, noise=0.3, mirror=tuple(range(0, B, 3)))
    p, t = _dev(case["pred"]), _dev(case["target"])
    for reflection in ("best", False, True):
        R = _np(procrustes_align(p, t, reflection=reflection).rotation).astype(np.float64)
        err = np.abs(np.einsum("bxy,bxz->byz", R, R) - np.eye(3)).max()
        det = np.linalg.det(R)
        print("reflection %s: |R^T R - I| max %.3e, | |det| - 1 | max %.3e" % (reflection, err, np.abs(np.abs(det) - 1).max()))
        assert err <= 1e-6 and np.abs(np.abs(det) - 1).max() <= 1e-6
        if reflection == "best":
            assert (det < 0).any() and (det > 0).any()
        else:
            assert ((det < 0) == reflection).all()
    # a coplanar target (z = 0): the proper rotation under 'best', d as the restatement says
    flat = case["target"].copy()
    flat[..., 2] = 0.0
    res = procrustes_align(p, _dev(flat))
    det = np.linalg.det(_np(res.rotation).astype(np.float64))
    assert np.abs(det - 1).max() <= 1e-6
    ref = pc.align(case["pred"], flat)
    _assert_parity(_np(res.d), ref["d"], "coplanar target: d")
    _assert_parity(_np(res.rotation), ref["rotation"], "coplanar target: rotation")
    _assert_parity(_np(res.aligned), ref["aligned"], "coplanar target: aligned")


# ----------------------------------------------------------------------------- degenerate poses
def test_degenerate_poses_are_nan_their_neighbours_unchanged_and_no_device_error():
    import openmpl_amd
    from openmpl_amd import procrustes_align
    B, J = 64, 17          # one workgroup
    case = pc.similarity_case(B, J, seed=12)
    base = procrustes_align(_dev(case["pred"]), _dev(case["target"]))
    pred, target = case["pred"].copy(), case["target"].copy()
    pred[5] = np.float32([1.5, -2.25, 0.5]) + np.arange(J, dtype=np.float32)[:, None] * np.float32([0.25, 0.5, -0.125])     # collinear
    target[20] = target[20, :1]                        # all joints equal
    pred[33] = pred[33, :1]
    pred[41, 7, 1] = np.nan                            # NaN input
    target[63, 0, 0] = np.inf
    bad = [5, 20, 33, 41, 63]
    rc, out = raw(_dev(pred), _dev(target), B, J)
    assert rc == 0 and all(o.intact() for o in out.values())
    keep = np.ones(B, bool)
    keep[bad] = False
    for k in pc.FIELDS:
        got = _np(out[k].t)
        assert np.isnan(got[bad]).all(), k
        assert np.array_equal(got[keep], _np(getattr(base, k))[keep]), k          # bitwise
    ref = pc.align(pred, target)
    assert np.array_equal(np.isnan(ref["d"]), ~keep)
    openmpl_amd.check_device()                         # a degenerate pose is no device error


# ----------------------------------------------------------------------------- determinism
def test_two_runs_and_two_batchings_are_bitwise_equal():
    from openmpl_amd import procrustes_align
    B, J = 130, 17
    case, sel, conf, _ = grid_case(B, J)

    def run(lo, hi):
        r = procrustes_align(_dev(case["pred"][lo:hi]), _dev(case["target"][lo:hi]), conf=_dev(conf[lo:hi]), joints=sel, scale=(2.0, 3.0, 0.5))
        return [_np(x) for x in r]

    a, b = run(0, B), run(0, B)
    halves = [np.concatenate(p) for p in zip(run(0, 64), run(64, B))]
    for x, y, z in zip(a, b, halves):
        assert np.array_equal(x, y, equal_nan=True) and np.array_equal(x, z, equal_nan=True)


# ----------------------------------------------------------------------------- optional outputs, refusals
def test_every_legal_subset_of_the_optional_outputs_leaves_the_others_alone():
    B, J = 65, 17
    case = pc.similarity_case(B, J, seed=13)
    p, t = _dev(case["pred"]), _dev(case["target"])
    rc, full = raw(p, t, B, J)
    assert rc == 0
    optional = ("d", "rotation", "scale", "translation")
    for r in range(len(optional) + 1):
        for subset in itertools.combinations(optional, r):
            for with_aligned in (True, False):
                outputs = subset + (("aligned",) if with_aligned else ())
                rc, out = raw(p, t, B, J, outputs=outputs)
                if not with_aligned and "d" not in subset:
                    assert rc == E_INVALID and all(o.untouched() for o in out.values()), outputs       # aligned may be NULL only if d is not
                    continue
                assert rc == 0, outputs
                for k in pc.FIELDS:
                    if k in outputs:
                        assert out[k].intact() and np.array_equal(_np(out[k].t), _np(full[k].t)), (outputs, k)
                    else:
                        assert out[k].untouched(), (outputs, k)


def test_refusals_launch_nothing_and_leave_the_outputs_alone():
    B = 3
    wide = pc.similarity_case(B, 65, seed=14)
    p, t = _dev(wide["pred"]), _dev(wide["target"])
    (rc, out), n = _launches(lambda: raw(p, t, B, 65))
    assert rc == E_UNSUPPORTED and n == 0 and all(o.untouched() for o in out.values())
    (rc, out), n = _launches(lambda: raw(p, t, B, 17, sel=[0] * 65))
    assert rc == E_UNSUPPORTED and n == 0 and all(o.untouched() for o in out.values())
    (rc, out), n = _launches(lambda: raw(p, t, B, 17, sel=[0, 5, 17]))
    assert rc == E_INVALID and n == 0 and all(o.untouched() for o in out.values())
    (rc, out), n = _launches(lambda: raw(p, t, 0, 17))
    assert rc == E_INVALID and n == 0 and all(o.untouched() for o in out.values())


# ----------------------------------------------------------------------------- the evaluator
def eval_run(J=17, N=150, n_groups=4, seed=21):
    """three ragged batches with groups, conf_3d, degenerate poses among them"""
    rs = np.random.RandomState(seed)
    case = pc.similarity_case(N, J, seed=seed, noise=0.2, mirror=(3, 77))
    conf = np.where(rs.rand(N, J) < 0.1, 0.0, 1.0).astype(np.float32)
    conf[10, 2:] = 0.0                                 # the selection below keeps fewer than 3 of joints 0 and 1: a NaN pose
    arrays = dict(output=case["pred"], target=case["target"], conf_3d=conf, group=rs.randint(-1, n_groups + 2, size=N).astype(np.int32))
    return ec.cut(arrays, [64, 65, N - 129])


def feed(ev, batches, **kw):
    for b in batches:
        ev.update(_dev(b["output"]), _dev(b["target"]), conf_3d=_dev(b.get("conf_3d")), group=_dev(b.get("group")), **kw)
    return ev


EVAL_KW = dict(joints=[0, 16, 3, 5, 8, -4, 11, 1], n_groups=4, output_in_meter=True, not_consider_kp=[2, -1])


@pytest.mark.parametrize("mode", ["similarity", "rigid"])
def test_evaluator_aligned_pass_matches_the_restatement_and_leaves_the_rest_bitwise(mode):
    from openmpl_amd import PoseEvaluator
    batches = eval_run()
    sc, of = (2.0, 3.0, 0.5), (0.1, 0.0, -0.2)
    mk = lambda aligned: PoseEvaluator(17, joints=EVAL_KW["joints"], groups=3, output_in_meter=True, not_consider_kp=EVAL_KW["not_consider_kp"],  # noqa: E731
                                       aligned=aligned)
    res = feed(mk(mode), batches, scale=sc, offset=of).compute()
    plain = feed(mk(None), batches, scale=sc, offset=of).compute()
    assert "aligned" not in plain
    ec.assert_same(res, plain, rtol=0)                          # loss, "absolute", "relative": bitwise
    ec.assert_same(res, ec.run(batches, scale=sc, offset=of, **EVAL_KW), rtol=1e-5)
    ref = eval_aligned(batches, mode, scale=sc, offset=of, **EVAL_KW)
    got = res["aligned"]
    print("%s: PA-MPJPE %.6g restatement %.6g, MPJPE %.6g" % (mode, got["mpjpe"], ref["mpjpe"], res["absolute"]["mpjpe"]))
    assert got["mpjpe"] < res["absolute"]["mpjpe"]
    assert sorted(got["per_group"]) == sorted(ref["per_group"]) == [1, 2, 3]
    for a, b, what in [(got, ref, "all")] + [(got["per_group"][k], ref["per_group"][k], "group %d" % k) for k in ref["per_group"]]:
        assert a["n_samples"] == b["n_samples"], what
        for f in ec.FIELDS:
            np.testing.assert_allclose(a[f], b[f], rtol=1e-5, equal_nan=True, err_msg="%s %s %s" % (mode, what, f))
    # identity de-normalisation takes the path without the de-normalised copy of the targets
    res1 = feed(mk(mode), batches).compute()
    ref1 = eval_aligned(batches, mode, **EVAL_KW)
    for f in ec.FIELDS:
        np.testing.assert_allclose(res1["aligned"][f], ref1[f], rtol=1e-5, equal_nan=True, err_msg=f)


def test_evaluator_update_does_not_synchronise_counts_its_launches_and_reset_clears_both_states():
    from openmpl_amd import PoseEvaluator
    batches = eval_run()
    dev = [{k: _dev(v) for k, v in b.items()} for b in batches]
    sc, of = (2.0, 3.0, 0.5), (0.1, 0.0, -0.2)

    def one(ev, b, **kw):
        ev.update(b["output"], b["target"], conf_3d=b["conf_3d"], group=b["group"], **kw)

    plain, pa = PoseEvaluator(17, groups=3), PoseEvaluator(17, groups=3, aligned="similarity")
    one(plain, dev[0]), one(pa, dev[0])                         # first calls: the library is loaded, the allocator warm
    _, n_plain = _launches(lambda: one(plain, dev[1], scale=sc, offset=of))
    _, n_pa = _launches(lambda: one(pa, dev[1], scale=sc, offset=of))
    print("kernels of the library per update(): %d without, %d with aligned" % (n_plain, n_pa))
    assert n_plain == 2                                        # accumulate + fold, as before this option existed
    assert n_pa == 2 * n_plain + 1                             # + one alignment + the second state's accumulate and fold
    # no host synchronisation: torch refuses every synchronising call of its own while the mode is "error", and the stream is
    # still busy with the work queued in front when update() returns
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        one(pa, dev[2], scale=sc, offset=of)
        one(pa, dev[2])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    before = pa.compute()
    assert before["aligned"]["n_samples"] == before["n_samples"] == 64 + 65 + 2 * 21
    pa.reset()
    empty = pa.compute()
    assert empty["n_samples"] == 0 and empty["aligned"]["n_samples"] == 0 and empty["aligned"]["per_group"] == {}
    again = feed(pa, batches, scale=sc, offset=of).compute()
    fresh = feed(PoseEvaluator(17, groups=3, aligned="similarity"), batches, scale=sc, offset=of).compute()
    ec.assert_same(again, fresh, rtol=0)
    for f in ec.FIELDS:
        assert np.array_equal(again["aligned"][f], fresh["aligned"][f], equal_nan=True), f


def test_evaluator_aligns_the_final_poses_of_the_kadkhod_tuple():
    from openmpl_amd import PoseEvaluator
    case = pc.similarity_case(40, 17, seed=23, noise=0.2)
    out, tgt = _dev(case["pred"]), _dev(case["target"])
    x1, x2 = out + 0.5, out - 0.25
    a = PoseEvaluator(17, criterion="mpjpe_kadkhoda", aligned="rigid")
    a.update((out, [x1, x2]), tgt)
    b = PoseEvaluator(17, aligned="rigid")
    b.update(out, tgt)
    ra, rb = a.compute()["aligned"], b.compute()["aligned"]
    for f in ec.FIELDS:
        assert np.array_equal(ra[f], rb[f]), f
