"""Run-level evaluator on the GPU (openmpl_amd/evaluate.py, csrc/evaluate.hip) against the reference's goldens and the float64
restatement of tests/evaluate_cases.py.

Bounds: rtol=2e-5, atol=1e-6 against the goldens (the kernel bound of test_metrics.py; the goldens carry numpy's float32 means),
rtol=1e-5 against the restatement (that file's large-batch bound), rtol=1e-6 between two batchings of one run (fp64 sums,
re-associated), bitwise between two identical runs.

The device-error rule (a batch that arrives while the device's error word is set poisons the state, a poisoned state reports NaN,
compute() raises through cabi.raise_if_device_error) is NOT exercised here: no test may provoke a device error.
MPJPE with LOSS.WEIGHT_AXIS exists in the reference for batches of 1 or J samples only (loss.py:56 broadcasts (B,J,1) * (B,J)),
so that criterion is fed in the fixture's own cut instead of 1 / 7 / 64 / all.
"""
import functools

import numpy as np
import pytest
import torch

from tests import evaluate_cases as ec

pytestmark = pytest.mark.gpu
SIZES = (1, 7, 64, 0)          # 0: all at once


def dev(b):
    t = {}
    for k, v in b.items():
        t[k] = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in v] if k == "x12" else torch.from_numpy(np.ascontiguousarray(v)).cuda()
    return t


def feed(ev, batches, **kw):
    for b in batches:
        t = dev(b)
        out = (t["output"], t["x12"]) if "x12" in t else t["output"]
        ev.update(out, t["target"], weight=t.get("weight"), conf_3d=t.get("conf_3d"), group=t.get("group"), **kw)
    return ev


def evaluator(kw, J=17, cls=None, **more):
    from openmpl_amd import PoseEvaluator
    return (cls or PoseEvaluator)(J, joints=kw["joints"], groups=kw["n_groups"] - 1, output_in_meter=kw["output_in_meter"],
                                  not_consider_kp=kw["not_consider_kp"], **more)


@functools.lru_cache(maxsize=None)
def golden_case(tag):
    g, arrays, kw = ec.golden_run(tag)
    return g, arrays, kw, ec.run(ec.cut(arrays, 0), **kw)


@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_evaluator_matches_reference_goldens_in_every_batching(tag):
    g, arrays, kw, ref = golden_case(tag)
    first = None
    for size in SIZES:
        ev = evaluator(kw)
        res = feed(ev, ec.cut(arrays, size), scale=kw["scale"], offset=kw["offset"]).compute()
        ec.check_against_golden(res, g, rtol=2e-5, atol=1e-6)
        ec.assert_same(res, ref, rtol=1e-5)
        assert res["n_samples"] == g["out"].shape[0] and not res["poisoned"]
        if first is None:
            first = res
        else:
            ec.assert_same(res, first, rtol=1e-6)          # another batching of the same samples


@pytest.mark.parametrize("name", sorted(ec.E_CRITERIA))
def test_evaluator_criteria_match_reference_goldens(name):
    from openmpl_amd import PoseEvaluator
    g = ec.golden("e")
    crit, wa = ec.E_CRITERIA[name]
    arrays, V = ec.golden_e_arrays(g), int(g["n_views"])
    axis = g["weight_axis"].tolist() if wa else None
    for size in ([g["splits_wa"].tolist()] if name == "mpjpe_wa" else list(SIZES) + [g["splits"].tolist()]):
        batches = ec.cut(arrays, size)
        res = feed(PoseEvaluator(17, criterion=crit, weight_axis=axis), batches, n_views=V).compute()
        ref = ec.run(batches, crit, axis, n_views=V)
        np.testing.assert_allclose(res["loss"], g["loss_" + name], rtol=2e-5, atol=1e-6)
        np.testing.assert_allclose(res["loss_axis"], g["axis_" + name], rtol=2e-5, atol=1e-6)
        ec.assert_same(res, ref, rtol=1e-5)
    if name == "mpjpe_wa":      # a batch the reference cannot broadcast raises what torch raises there, before any launch
        with pytest.raises(RuntimeError, match="non-singleton dimension"):
            feed(PoseEvaluator(17, criterion=crit, weight_axis=axis), ec.cut(arrays, [7, 113]))


def random_run(J, N, n_groups, seed, gone=0.05):
    rs = np.random.RandomState(seed)
    out = rs.randn(N, J, 3).astype(np.float32)
    tgt = (out + 0.1 * rs.randn(N, J, 3)).astype(np.float32)
    conf = np.where(rs.rand(N, J) < gone, 0.0, 1.0).astype(np.float32)
    arrays = dict(output=out, target=tgt, conf_3d=conf, weight=rs.rand(N, J).astype(np.float32))
    if n_groups > 1:
        arrays["group"] = rs.randint(-1, n_groups + 2, size=N).astype(np.int32)      # ids outside 1..n_groups-1 count in group 0 only
    return arrays


@pytest.mark.parametrize("J,N,n_groups,nck,size", [(1, 50, 1, None, 0), (18, 131, 3, [17, -18], 64), (64, 97, 32, [40, 63], 0),
                                                   (17, 1, 1, None, 0), (17, 1, 32, [0], 0), (17, 8192, 17, None, 0)])
def test_evaluator_shape_edges_against_restatement(J, N, n_groups, nck, size):
    """J = 1 / 18 / 64 (the two geometries of pose_metrics_kernel and the largest J), joints 40 and 63 in not_consider_kp, a batch
    of 1, 8192 samples in one call (many workgroups, the fixed-order fold), n_groups = 1 and the cap."""
    from openmpl_amd import PoseEvaluator, cabi
    assert cabi.EVAL_MAX_GROUPS == 32
    arrays = random_run(J, N, n_groups, seed=J + N)
    sel = None if J != 18 else list(range(17, -1, -1))
    kw = dict(joints=sel, n_groups=n_groups, output_in_meter=J == 64, not_consider_kp=nck, scale=(2.0, 3.0, 0.5), offset=(0.1, 0.0, -0.2))
    batches = ec.cut(arrays, size)
    ev = PoseEvaluator(J, criterion="weighted_mpjpe", joints=sel, groups=n_groups - 1, output_in_meter=J == 64, not_consider_kp=nck)
    res = feed(ev, batches, scale=kw["scale"], offset=kw["offset"], n_views=2).compute()
    ref = ec.run(batches, "weighted_mpjpe", n_views=2, **kw)
    ec.assert_same(res, ref, rtol=1e-5)
    if n_groups > 1:
        assert all(1 <= k < n_groups for k in res["absolute"]["per_group"])
    with pytest.raises(NotImplementedError):
        PoseEvaluator(J, groups=cabi.EVAL_MAX_GROUPS)          # one group beyond the cap


def test_evaluator_is_deterministic_and_reset_starts_over():
    g, arrays, kw, _ = golden_case("c")
    runs = []
    for size in (7, 7, 64):
        runs.append(feed(evaluator(kw), ec.cut(arrays, size), scale=kw["scale"], offset=kw["offset"]).compute())
    ec.assert_same(runs[0], runs[1], rtol=0)                  # bitwise
    ec.assert_same(runs[0], runs[2], rtol=1e-6)               # re-associated fp64 sums
    big = random_run(17, 8192, 17, seed=3)
    a = feed(evaluator(dict(kw, joints=None)), ec.cut(big, 0)).compute()
    b = feed(evaluator(dict(kw, joints=None)), ec.cut(big, 0)).compute()
    ec.assert_same(a, b, rtol=0)


def test_update_launches_two_kernels_and_stays_inside_its_buffers():
    from openmpl_amd import PoseEvaluator, cabi
    g, arrays, kw, _ = golden_case("b")
    N, J, K = g["out"].shape[0], 17, 320

    class Guarded(PoseEvaluator):          # the same buffers with a canary region behind the state and behind the kept poses
        def _alloc(self, nbytes):
            n, m = nbytes // 8, 2 * K * J * 3
            self.state_all = torch.full((n + 4096,), 1234.5, dtype=torch.float64, device=self.device)
            self.keep_all = torch.full((m + 4096,), -7.0, dtype=torch.float32, device=self.device)
            self._state = self.state_all[:n]
            self._keep = self.keep_all[:m].view(2, K, J, 3)

    ev = evaluator(kw, cls=Guarded, keep_poses=K)
    batches = ec.cut(arrays, 64)
    first = dev(batches[0])
    torch.cuda.synchronize()
    cabi.profile_start()
    ev.update(first["output"], first["target"], conf_3d=first["conf_3d"], scale=kw["scale"], offset=kw["offset"])
    prof = cabi.profile_stop()
    assert 1 <= sum(n for _, n in prof.values()) <= 2, prof
    feed(ev, batches[1:], scale=kw["scale"], offset=kw["offset"])
    res = ev.compute()
    assert bool((ev.state_all[-4096:] == 1234.5).all()) and bool((ev.keep_all[-4096:] == -7.0).all())
    assert bool((ev._keep[:, N:] == -7.0).all())              # rows past the run are untouched, of both buffers
    pred, tgt = ev.poses()
    sc, of = np.asarray(kw["scale"], dtype=np.float32), np.asarray(kw["offset"], dtype=np.float32)
    assert pred.shape == (N, J, 3) and pred.is_cuda
    np.testing.assert_allclose(pred.cpu().numpy(), g["out"] * sc + of, rtol=1e-6, atol=1e-7)       # before the joint selection
    np.testing.assert_allclose(tgt.cpu().numpy(), g["tgt"] * sc + of, rtol=1e-6, atol=1e-7)
    with pytest.raises(RuntimeError, match="keep_poses"):
        ev.update(first["output"], first["target"], conf_3d=first["conf_3d"])
    ev.reset()
    again = feed(ev, batches, scale=kw["scale"], offset=kw["offset"]).compute()
    ec.assert_same(again, res, rtol=0)                        # reset() + the same run: bitwise the first report
    assert bool((ev.state_all[-4096:] == 1234.5).all()) and bool((ev.keep_all[-4096:] == -7.0).all())


def test_evaluator_agrees_with_pose_metrics():
    from openmpl_amd import PoseEvaluator
    from openmpl_amd.metrics import pose_metrics
    a = random_run(17, 256, 1, seed=9)
    out, tgt = torch.from_numpy(a["output"]).cuda(), torch.from_numpy(a["target"]).cuda()
    ev = PoseEvaluator(17)
    ev.update(out, tgt)
    res = ev.compute()
    m = {k: v.cpu().numpy() for k, v in pose_metrics(out, tgt).items()}
    for mine, theirs in ((res["loss"], "loss"), (res["loss_axis"], "loss_axis"), (res["absolute"]["pjpe"], "pjpe_abs"),
                         (res["absolute"]["mpjpe"], "mpjpe_abs"), (res["relative"]["pjpe"], "pjpe_rel"),
                         (res["relative"]["mpjpe"], "mpjpe_rel"), (res["absolute"]["dist"], "dist"),
                         (res["absolute"]["dist_mean"], "dist_mean")):
        np.testing.assert_allclose(mine, m[theirs], rtol=1e-6, err_msg=theirs)
    wide = torch.zeros(4, 64, 3, device="cuda")
    with pytest.raises(NotImplementedError):
        pose_metrics(wide, wide, not_consider_kp=[40])        # the 32-bit mask of the per-batch kernel is as it was


def test_evaluator_errors_are_loud_and_launch_nothing():
    from openmpl_amd import PoseEvaluator, cabi
    ev = PoseEvaluator(17, groups=3)
    out = torch.zeros(5, 17, 3, device="cuda")
    gid = torch.ones(5, dtype=torch.int32, device="cuda")
    with pytest.raises(IndexError):
        PoseEvaluator(17, joints=[0, 17])
    with pytest.raises(IndexError):
        PoseEvaluator(17, joints=[3, 1], not_consider_kp=[2])           # not_consider_kp indexes the SELECTED joints
    torch.cuda.synchronize()
    cabi.profile_start()
    with pytest.raises(RuntimeError, match="no CPU path"):
        ev.update(out.cpu(), out.cpu(), group=gid)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ev.update(out, out.cpu(), group=gid)
    with pytest.raises(RuntimeError, match="float32"):
        ev.update(out.double(), out.double(), group=gid)
    with pytest.raises(RuntimeError, match="shape"):
        ev.update(out, out[:4], group=gid)
    with pytest.raises(RuntimeError):
        ev.update(out[:, :16], out[:, :16], group=gid)
    with pytest.raises(RuntimeError, match="shape"):
        ev.update(out, out, conf_3d=torch.ones(5, 16, device="cuda"), group=gid)
    with pytest.raises(RuntimeError, match="int32"):
        ev.update(out, out, group=gid.long())
    with pytest.raises(RuntimeError, match="shape"):
        ev.update(out, out, group=gid[:4])
    with pytest.raises(RuntimeError, match="group ids"):
        ev.update(out, out)
    with pytest.raises(RuntimeError, match="tuple"):
        PoseEvaluator(17, criterion="mpjpe_kadkhoda").update(out, out)
    prof = cabi.profile_stop()
    assert sum(n for _, n in prof.values()) == 0, prof
    assert ev.compute()["n_samples"] == 0
