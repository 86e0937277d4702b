"""Triangulation and epipolar consistency on the GPU (openmpl_amd/geometry.py, csrc/geometry.hip) against the reference's golden
and the float64 restatement of tests/geometry_cases.py.

Bound everywhere: the parity rule of DESIGN.md section 2, max|d| <= 1e-4 max|ref| and ||d||_2 <= 1e-4 ||ref||_2 (the kernels
compute in fp64 and round once to fp32, so they sit near 1e-7; against the golden the fp32 rounding of the rays adds ~3e-6, which
the restatement measures on the CPU in tests/test_geometry_cpu.py).  Weights are compared exactly, repeated runs bitwise.
Outputs of the shape grid lie between canary regions and start as canaries, so an element a kernel skips fails too.

Before every assertion on an error the figures are printed (pytest -s shows them).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import evaluate_cases as ec
from tests import geometry_cases as gc

pytestmark = pytest.mark.gpu
TOL = 1e-4
GUARD, CANARY = 4096, -12345.0
E_UNSUPPORTED = -2


def _dev(arrays):
    return None if arrays is None else [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _np(t):
    return t.detach().cpu().numpy()


def _assert_parity(got, ref, what):
    mx, nw = gc.rel_errors(got, ref)
    print("%s: max-scaled %.3e norm-wise %.3e" % (what, mx, nw))
    assert mx <= TOL and nw <= TOL, "%s: max-scaled %.3e norm-wise %.3e (tol %.0e)" % (what, mx, nw, TOL)


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


def _table(tensors, n=None):
    from openmpl_amd import cabi
    if tensors is None:
        return None
    ptrs = [t.data_ptr() for t in tensors]
    ptrs += [ptrs[-1]] * ((n or len(ptrs)) - len(ptrs))
    return (cabi._fp * len(ptrs))(*ptrs)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def raw_triangulate(rays, centers, conf, B, V, J, stride=1):
    """the C ABI on guarded outputs -> (return code, points, residual)"""
    from openmpl_amd import cabi
    pts, res = Guarded(B, J, 3), Guarded(B, J)
    rc = cabi.load().mpl_triangulate_rays(_table(rays, V), _table(centers, V), _table(conf, V), stride, B, V, J, pts.t.data_ptr(),
                                          res.t.data_ptr(), _stream())
    torch.cuda.synchronize()
    return rc, pts, res


def raw_epipolar(rays, centers, conf, B, V, J, stride=1, weight=None, threshold=0.0):
    from openmpl_amd import cabi
    err, wout = Guarded(B, V, J), Guarded(B, V, J)
    rc = cabi.load().mpl_epipolar_errors(_table(rays, V), _table(centers, V), _table(conf, V), stride, B, V, J, err.t.data_ptr(),
                                         None if weight is None else weight.data_ptr(), float(threshold),
                                         None if weight is None else wout.t.data_ptr(), _stream())
    torch.cuda.synchronize()
    return rc, err, wout


def conf_forms(case, seed):
    """the three ways a confidence reaches the kernels -> (name, device list or None, stride, numpy list for the restatement)"""
    V = len(case["rays"])
    flat = [case["conf"][v] for v in range(V)]
    rs = np.random.RandomState(seed)
    poses = [np.concatenate([rs.randn(*c.shape, 2).astype(np.float32) * 50, c[..., None]], axis=-1) for c in flat]   # x, y, conf
    return (("none", None, 1, None), ("(B,J)", _dev(flat), 1, flat), ("(B,J,3)", _dev(poses), 3, poses))


# ----------------------------------------------------------------------------- the reference's golden
@functools.lru_cache(maxsize=None)
def golden():
    return gc.golden()


@pytest.mark.parametrize("tag", ["v2", "v3", "v4"])
def test_epipolar_errors_and_weights_match_the_reference_golden(tag):
    from openmpl_amd import consistency_weights, epipolar_errors
    c = gc.golden_case(golden(), tag)
    V = len(c["rays"])
    rays, centers = _dev(c["rays"]), _dev(c["centers"])
    flat = [c["conf"][v] for v in range(V)]
    poses = [np.concatenate([np.zeros(f.shape + (2,), np.float32), f[..., None]], axis=-1) for f in flat]
    weight = [c["weight"][v] for v in range(V)]
    first = None
    for name, conf in (("(B,J)", _dev(flat)), ("(B,J,3)", _dev(poses))):
        err = epipolar_errors(rays, centers, conf)
        assert err.shape == c["err"].shape and err.dtype == torch.float32 and err.is_cuda
        _assert_parity(_np(err), c["err"], "golden %s conf %s" % (tag, name))
        _assert_parity(_np(err), gc.epipolar(c["rays"], c["centers"], flat), "restatement %s conf %s" % (tag, name))
        w = consistency_weights(rays, centers, conf, _dev(weight), threshold=c["threshold"])
        assert len(w) == V and all(tuple(x.shape) == weight[0].shape for x in w)
        for v in range(V):
            assert np.array_equal(_np(w[v]), c["weights_out"][v]), "%s view %d" % (tag, v)
        first = _np(err) if first is None else first
        assert np.array_equal(first, _np(err))                  # both confidence forms read the same numbers
    # without confidences every view's total is unscaled: the mean of the recorded pair distances
    plain = gc.epipolar(c["rays"], c["centers"])
    _assert_parity(_np(epipolar_errors(rays, centers)), plain, "golden %s no conf" % tag)
    p, acc = 0, np.zeros_like(plain)
    for i in range(V):
        for k in range(i + 1, V):
            acc[:, i] += c["pairs"][p]
            acc[:, k] += c["pairs"][p]
            p += 1
    _assert_parity(_np(epipolar_errors(rays, centers)), acc / (V - 1), "golden %s recorded pair distances" % tag)


# ----------------------------------------------------------------------------- shapes where the indexing can go wrong
# V in {2, 3, 5, 32}, J in {1, 17, 64}, B in {1, 3, 63, 65, 257}: B * J below (1, 51, 63), on (64) and above (65, 192, ...) one
# 64-item epipolar workgroup and one 256-item triangulation workgroup (257, 1071, 4160, 16448)
SHAPES = [(2, 1, 1), (2, 17, 3), (2, 64, 1), (2, 64, 257), (3, 1, 63), (3, 1, 65), (3, 17, 257), (5, 17, 63), (5, 64, 3), (5, 1, 257),
          (32, 17, 3), (32, 1, 63), (32, 64, 65)]


@pytest.mark.parametrize("V,J,B", SHAPES)
def test_both_kernels_against_float64_at_every_confidence_form(V, J, B):
    case = gc.ring_case(B, V, J, seed=3)
    rays, centers = _dev(case["rays"]), _dev(case["centers"])
    weight = torch.from_numpy(np.random.RandomState(5).rand(B, V, J).astype(np.float32)).cuda()
    for name, conf, stride, conf_np in conf_forms(case, seed=V + J + B):
        what = "V%d J%d B%d conf %s" % (V, J, B, name)
        rc, pts, res = raw_triangulate(rays, centers, conf, B, V, J, stride)
        assert rc == 0 and pts.intact() and res.intact(), what
        x_ref, r_ref = gc.triangulate(case["rays"], case["centers"], conf_np)
        _assert_parity(_np(pts.t), x_ref, "points " + what)
        _assert_parity(_np(res.t), r_ref, "residual " + what)
        e_ref = gc.epipolar(case["rays"], case["centers"], conf_np)
        thr = float(np.median(e_ref))
        rc, err, wout = raw_epipolar(rays, centers, conf, B, V, J, stride, weight, thr)
        assert rc == 0 and err.intact() and wout.intact(), what
        _assert_parity(_np(err.t), e_ref, "epipolar " + what)
        far = np.abs(e_ref - thr) > 1e-3 * thr                                   # entries no rounding can move across
        w_ref = np.where(e_ref > thr, 0.0, _np(weight))
        assert np.array_equal(_np(wout.t)[far], w_ref[far].astype(np.float32)), what
        rc, err2, wout2 = raw_epipolar(rays, centers, conf, B, V, J, stride)      # no epilogue: the weights stay out of it
        assert rc == 0 and wout2.untouched() and np.array_equal(_np(err2.t), _np(err.t)), what


def test_python_entry_points_return_what_the_c_abi_writes():
    from openmpl_amd import consistency_weights, epipolar_errors, triangulate_rays
    B, V, J = 65, 5, 17
    case = gc.ring_case(B, V, J, seed=4)
    rays, centers = _dev(case["rays"]), _dev(case["centers"])
    for name, conf, stride, _ in conf_forms(case, seed=1):
        (pts, res), n = _launches(lambda: triangulate_rays(rays, centers, conf))
        assert n == 1 and tuple(pts.shape) == (B, J, 3) and tuple(res.shape) == (B, J)
        _, p2, r2 = raw_triangulate(rays, centers, conf, B, V, J, stride)
        assert np.array_equal(_np(pts), _np(p2.t)) and np.array_equal(_np(res), _np(r2.t)), name
        err, n = _launches(lambda: epipolar_errors(rays, centers, conf))
        assert n == 1 and tuple(err.shape) == (B, V, J)
        _, e2, _ = raw_epipolar(rays, centers, conf, B, V, J, stride)
        assert np.array_equal(_np(err), _np(e2.t)), name
    weight = [torch.rand(B, J, device="cuda") for _ in range(V)]
    w, n = _launches(lambda: consistency_weights(rays, centers, None, weight, threshold=0.02))
    assert n == 1
    plain = _np(epipolar_errors(rays, centers))
    far = np.abs(plain - 0.02) > 1e-3 * 0.02
    assert (plain > 0.02).any() and (plain < 0.02).any()
    for v in range(V):
        assert np.array_equal(_np(w[v])[far[:, v]], np.where(plain[:, v] > 0.02, 0, _np(weight[v]))[far[:, v]])


# ----------------------------------------------------------------------------- a constructed exact case
def test_lines_through_a_known_point_and_one_line_moved_by_a_known_offset():
    from openmpl_amd import epipolar_errors, triangulate_rays
    B, V, J = 3, 5, 17
    case = gc.ring_case(B, V, J, seed=6, exact=True)
    x_ref, r_ref = gc.triangulate(case["rays"], case["centers"])
    pts, res = triangulate_rays(_dev(case["rays"]), _dev(case["centers"]))
    _assert_parity(_np(pts), case["points"], "exact case: the known point")
    _assert_parity(_np(pts), x_ref, "exact case: points")
    # the residual is what the fp32 rounding of the inputs leaves: eps32 / 2 per coordinate of a ray point (|coordinate| < 8 m)
    # on a line whose point sits 1 .. 2 m from the centre, seen at up to 8 m -- and the float64 restatement measures it on the
    # same fp32 inputs: the kernel may not exceed that figure by more than its own fp32 output rounding
    lever = 8.0
    bound = np.sqrt(3.0) * 2.0 ** -24 * 8.0 * lever
    print("exact case: residual kernel max %.3e restatement max %.3e construction bound %.3e" % (_np(res).max(), r_ref.max(), bound))
    assert 0 < r_ref.max() <= bound
    assert _np(res).max() <= r_ref.max() * (1 + 2.0 ** -23)
    _assert_parity(_np(res), r_ref, "exact case: residual")

    # view 2's line moved by delta: every pair (2, k) is now |delta . n_2k| apart, n_2k the unit normal of both directions
    delta = np.array([0.03, -0.02, 0.05])
    moved = dict(rays=[r.copy() for r in case["rays"]], centers=[c.copy() for c in case["centers"]])
    moved["rays"][2] = (moved["rays"][2].astype(np.float64) + delta).astype(np.float32)
    moved["centers"][2] = (moved["centers"][2].astype(np.float64) + delta).astype(np.float32)
    c, d = gc.lines(case["rays"], case["centers"])
    expect = np.zeros((B, J))
    for k in range(V):
        if k != 2:
            n = np.cross(d[2], d[k])
            expect += np.abs(np.sum(delta * n, axis=-1)) / np.linalg.norm(n, axis=-1)
    expect /= V - 1
    e_ref = gc.epipolar(moved["rays"], moved["centers"])
    np.testing.assert_allclose(e_ref[:, 2], expect, rtol=1e-4)                   # the restatement says what geometry says
    err = epipolar_errors(_dev(moved["rays"]), _dev(moved["centers"]))
    _assert_parity(_np(err), e_ref, "moved line: epipolar errors")
    _assert_parity(_np(err)[:, 2], expect, "moved line: view 2 against |delta . n|")
    x_m, r_m = gc.triangulate(moved["rays"], moved["centers"])
    assert r_m.min() > 100 * r_ref.max()                                         # the residual sees the offset
    pts_m, res_m = triangulate_rays(_dev(moved["rays"]), _dev(moved["centers"]))
    _assert_parity(_np(pts_m), x_m, "moved line: points")
    _assert_parity(_np(res_m), r_m, "moved line: residual")


# ----------------------------------------------------------------------------- degenerate joints
def _nan_joints(pts, res):
    assert np.array_equal(np.isnan(pts).any(axis=-1), np.isnan(pts).all(axis=-1))
    assert np.array_equal(np.isnan(pts).all(axis=-1), np.isnan(res))
    return set(zip(*np.nonzero(np.isnan(res))))


def test_degenerate_joints_are_nan_and_their_neighbours_unchanged():
    from openmpl_amd import triangulate_rays
    B, V, J = 3, 3, 17
    case = gc.ring_case(B, V, J, seed=7)
    rays, centers = _dev(case["rays"]), _dev(case["centers"])
    base = [case["conf"][v].copy() for v in range(V)]
    p0, r0 = (_np(t) for t in triangulate_rays(rays, centers, _dev(base)))
    assert not _nan_joints(p0, r0)

    conf = [c.copy() for c in base]
    conf[1][1, 5] = conf[2][1, 5] = 0.0                       # one participating view
    for v in range(V):
        conf[v][2, 0] = 0.0                                   # all confidences 0
    conf[1][0, 16] = np.nan                                   # a NaN confidence drops that view only
    conf[2][0, 3] = -1.0                                      # so does a negative one
    conf[0][0, 4] = np.inf                                    # and an infinite one
    p1, r1 = (_np(t) for t in triangulate_rays(rays, centers, _dev(conf)))
    assert _nan_joints(p1, r1) == {(1, 5), (2, 0)}
    same = np.ones((B, J), bool)
    for at in ((1, 5), (2, 0), (0, 16), (0, 3), (0, 4)):
        same[at] = False
    assert np.array_equal(p1[same], p0[same]) and np.array_equal(r1[same], r0[same])      # bitwise
    x_ref, r_ref = gc.triangulate(case["rays"], case["centers"], conf)
    _assert_parity(p1, x_ref, "degenerate joints: points")
    _assert_parity(r1, r_ref, "degenerate joints: residual")
    dropped = [c.copy() for c in conf]
    dropped[1][0, 16] = dropped[2][0, 3] = dropped[0][0, 4] = 0.0
    p2, r2 = (_np(t) for t in triangulate_rays(rays, centers, _dev(dropped)))
    assert np.array_equal(p2, p1, equal_nan=True) and np.array_equal(r2, r1, equal_nan=True)
    assert np.isfinite(p1[0, 16]).all() and not np.array_equal(p1[0, 16], p0[0, 16])

    # two identical lines: sample 1 sees both views from ONE centre (its other joints meet at that centre: finite), and joint 7
    # of view 1 looks exactly along view 0's line
    two = gc.ring_case(B, 2, J, seed=8)
    two["centers"][1][1] = two["centers"][0][1]
    pa, ra = (_np(t) for t in triangulate_rays(_dev(two["rays"]), _dev(two["centers"])))
    assert not _nan_joints(pa, ra)
    two["rays"][1][1, 7] = two["rays"][0][1, 7]
    pb, rb = (_np(t) for t in triangulate_rays(_dev(two["rays"]), _dev(two["centers"])))
    assert _nan_joints(pb, rb) == {(1, 7)}
    same = np.ones((B, J), bool)
    same[1, 7] = False
    assert np.array_equal(pb[same], pa[same]) and np.array_equal(rb[same], ra[same])
    _assert_parity(pb, gc.triangulate(two["rays"], two["centers"])[0], "identical lines: points")


def test_parallel_pair_takes_the_point_to_line_distance():
    from openmpl_amd import epipolar_errors
    B, V, J = 2, 3, 17
    case = gc.ring_case(B, V, J, seed=9)
    d = np.array([0.5, 1.0, 0.25])                           # dyadic numbers: r - c is exact, the cross product exactly 0
    c0, c1 = np.array([1.5, -2.25, 0.5]), np.array([-3.0, 1.75, 2.5])
    case["centers"][0][0, 0], case["centers"][1][0, 0] = c0, c1
    case["rays"][0][0, 3], case["rays"][1][0, 3] = c0 + d, c1 - 2 * d
    c, dd = gc.lines(case["rays"], case["centers"])
    pair = gc.pair_distance(c[0], dd[0], c[1], dd[1])
    expect = np.linalg.norm(np.cross(c1 - c0, d)) / np.linalg.norm(d)
    assert abs(pair[0, 3] - expect) <= 1e-12 * expect and expect > 1.0
    e_ref = gc.epipolar(case["rays"], case["centers"])
    err = _np(epipolar_errors(_dev(case["rays"]), _dev(case["centers"])))
    assert np.isfinite(err).all()
    _assert_parity(err, e_ref, "parallel pair: epipolar errors")
    other = gc.pair_distance(c[0], dd[0], c[2], dd[2])[0, 3]
    print("parallel pair: kernel %.9g expected %.9g" % (err[0, 0, 3], (expect + other) / 2))
    assert abs(err[0, 0, 3] - (expect + other) / 2) <= TOL * (expect + other) / 2


# ----------------------------------------------------------------------------- determinism
def test_two_runs_and_two_batchings_are_bitwise_equal():
    from openmpl_amd import consistency_weights, epipolar_errors, triangulate_rays
    B, V, J = 130, 4, 17
    case = gc.ring_case(B, V, J, seed=10)
    conf = [case["conf"][v] for v in range(V)]
    weight = [np.random.RandomState(v).rand(B, J).astype(np.float32) for v in range(V)]

    def run(lo, hi):
        cut = lambda lst: _dev([a[lo:hi] for a in lst])      # noqa: E731
        r, c, cf = cut(case["rays"]), cut(case["centers"]), cut(conf)
        pts, res = triangulate_rays(r, c, cf)
        w = consistency_weights(r, c, cf, cut(weight), threshold=0.02)
        return [_np(pts), _np(res), _np(epipolar_errors(r, c, cf))] + [_np(x) for x in w]

    a, b = run(0, B), run(0, B)
    halves = [np.concatenate(p) for p in zip(run(0, 65), run(65, B))]
    for x, y, z in zip(a, b, halves):
        assert np.array_equal(x, y) and np.array_equal(x, z)


# ----------------------------------------------------------------------------- into the evaluator
def test_pose_evaluator_scores_the_triangulated_points():
    from openmpl_amd import PoseEvaluator, triangulate_rays
    B, V, J = 65, 4, 17
    case = gc.ring_case(B, V, J, seed=11, noise=0.05)
    conf = [case["conf"][v] for v in range(V)]
    target = case["points"].astype(np.float32)
    pts, _ = triangulate_rays(_dev(case["rays"]), _dev(case["centers"]), _dev(conf))
    ev = PoseEvaluator(J)
    ev.update(pts, torch.from_numpy(target).cuda())
    res = ev.compute()
    x_ref, _ = gc.triangulate(case["rays"], case["centers"], conf)
    ref = ec.run([dict(output=x_ref.astype(np.float32), target=target)])
    print("evaluator on triangulated points: mpjpe %.6g restatement %.6g" % (res["absolute"]["mpjpe"], ref["absolute"]["mpjpe"]))
    ec.assert_same(res, ref, rtol=1e-5)                      # the restatement bound of tests/test_evaluate_gpu.py
    assert 0.01 < res["absolute"]["mpjpe"] < 0.2             # centimetres of detection noise, in metres


# ----------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing_and_leave_the_outputs_alone():
    from openmpl_amd import cabi, epipolar_errors
    lib = cabi.load()
    B, J = 3, 17
    case = gc.ring_case(B, 2, J, seed=12)
    rays, centers = _dev(case["rays"]), _dev(case["centers"])
    wide = gc.ring_case(B, 2, 65, seed=12)
    wrays, wcenters = _dev(wide["rays"]), _dev(wide["centers"])

    def refused(fn, *args):
        (rc, *outs), n = _launches(lambda: fn(*args))
        assert rc == E_UNSUPPORTED and n == 0 and all(o.untouched() for o in outs)

    refused(raw_epipolar, rays, centers, None, B, 1, J)                          # one view has no pair
    refused(raw_epipolar, rays, centers, None, B, cabi.MPL_MAX_VIEWS + 1, J)     # the tables are padded to 33 entries
    refused(raw_triangulate, rays, centers, None, B, cabi.MPL_MAX_VIEWS + 1, J)
    refused(raw_epipolar, wrays, wcenters, None, B, 2, 65)
    refused(raw_triangulate, wrays, wcenters, None, B, 2, 65)
    # bad arguments are MPL_E_INVALID, also before any launch
    out = Guarded(B, J, 3)

    def invalid():
        t = _table(rays)
        return [lib.mpl_triangulate_rays(None, _table(centers), None, 1, B, 2, J, out.t.data_ptr(), out.t.data_ptr(), _stream()),
                lib.mpl_triangulate_rays(t, _table(centers), None, 1, 0, 2, J, out.t.data_ptr(), out.t.data_ptr(), _stream()),
                lib.mpl_triangulate_rays(t, _table(centers), None, 1, B, 2, J, None, out.t.data_ptr(), _stream()),
                lib.mpl_triangulate_rays(t, _table(centers), _table(rays), 2, B, 2, J, out.t.data_ptr(), out.t.data_ptr(), _stream()),
                lib.mpl_epipolar_errors(t, _table(centers), None, 1, B, 2, J, out.t.data_ptr(), out.t.data_ptr(), C.c_float(1.0), None,
                                        _stream()),
                lib.mpl_epipolar_errors(t, (cabi._fp * 2)(centers[0].data_ptr(), None), None, 1, B, 2, J, out.t.data_ptr(), None,
                                        C.c_float(1.0), None, _stream())]

    codes, n = _launches(invalid)
    assert codes == [-1] * 6 and n == 0 and out.untouched()
    # the Python layer refuses the same shapes, and CPU tensors, without a launch
    def python_side():
        with pytest.raises(NotImplementedError):
            epipolar_errors(rays[:1], centers[:1])
        with pytest.raises(NotImplementedError):
            epipolar_errors(wrays, wcenters)
        with pytest.raises(RuntimeError, match=r"rays\[1\]"):
            epipolar_errors([rays[0], rays[1].cpu()], centers)
        with pytest.raises(RuntimeError, match=r"centers\[0\]"):
            epipolar_errors(rays, [centers[0].double(), centers[1]])

    _, n = _launches(python_side)
    assert n == 0
