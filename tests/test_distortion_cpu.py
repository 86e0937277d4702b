"""The lens model (csrc/views.hpp) without a GPU: the float64 restatement against the reference-generated golden, its Newton
inverse, the scene builder of the GPU tests, and the new C prototypes against their bindings and their refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from openmpl_amd import cabi
from tests import distortion_cases as dc

G = dc.golden()
SHAPES = [(1, 1, 1), (3, 4, 17), (2, 32, 3), (5, 2, 64)]
HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mpl_hip.h")).read()


def test_golden_is_small():
    assert os.path.getsize(os.path.join(dc.GOLD, "distortion.npz")) < 100 * 1024
    assert G["points"].shape == (4, 17, 3) and G["cams"].shape == (3, 16)


@pytest.mark.parametrize("name", ["zeros", "h36m", "strong"])
def test_projection_matches_reference_golden(name):
    assert np.array_equal(G[name + "_dist"], dc.table(name, 3))
    px, depth = dc.project(G["points"], G["cams"], G[name + "_dist"])
    np.testing.assert_allclose(px, G[name + "_pixels"], rtol=1e-12, atol=0)
    assert depth.min() > 0.5
    if name != "zeros":            # the case does what it is there for: the lens moves pixels by more than a pixel
        assert np.abs(G[name + "_pixels"] - G["zeros_pixels"]).max() > 1.0


@pytest.mark.parametrize("name", ["zeros", "h36m", "strong"])
def test_inverse_takes_the_golden_back_to_the_pinhole(name):
    u = dc.undistort_pixels(G[name + "_pixels"], G["cams"], G[name + "_dist"])
    assert u["valid"].all()
    err = np.abs(u["pixels"] - G["zeros_pixels"]).max()
    print("%s: undistorted golden against the pinhole golden: %.3e px, at most %d iterations" % (name, err, u["iterations"].max()))
    assert err <= 1e-9
    assert u["iterations"].max() <= 8
    # and the forward polynomial on the pinhole pixels gives the distorted ones
    np.testing.assert_allclose(dc.distort_pixels(G["zeros_pixels"], G["cams"], G[name + "_dist"]), G[name + "_pixels"], rtol=0, atol=1e-9)


@pytest.mark.parametrize("B,V,J", SHAPES)
@pytest.mark.parametrize("name", dc.SETS)
def test_every_valid_item_converges_quickly(B, V, J, name):
    c = dc.case(B, V, J, name)
    u = c["restated"]
    assert c["skipped"] == 0 and u["valid"].all() and c["valid"].all()
    assert u["iterations"].max() <= 8 and u["min_det"].min() >= dc.DET_MIN
    # the inverse is one: through the lens again it lands on the pixel it came from
    back = dc.distort_pixels(u["pixels"], c["cams"], c["dist"])
    assert np.abs(back - c["pixels"].astype(np.float64)).max() <= 1e-9


@pytest.mark.parametrize("B,V,J,every", [(1, 1, 1, 1), (3, 4, 17, 5), (2, 32, 3, 5), (5, 2, 64, 5)])
@pytest.mark.parametrize("name", ["cmu", "strong", "per_view"])
def test_deliberately_invalid_items_are_reported_invalid(B, V, J, every, name):
    if (B, V, J) == (1, 1, 1) and name == "per_view":
        name = "strong"                      # view 0 of per_view has no fold
    c = dc.case(B, V, J, name, invalid_every=every)
    u = c["restated"]
    assert c["skipped"] == 0 and (~c["valid"]).any()
    assert np.array_equal(u["valid"], c["valid"])
    assert np.isnan(u["pixels"][~c["valid"]]).all() and np.isfinite(u["pixels"][c["valid"]]).all()
    if c["valid"].any():
        assert u["iterations"][c["valid"]].max() <= 8
    # prepare: an invalid joint keeps its pinhole ray and gets confidence 0
    conf = np.full((B, V, J), 0.75)
    r = dc.prepare(c["pixels"], conf, c["cams"], c["dist"], (1000.0, 1000.0))
    pin = dc.prepare(c["pixels"], conf, c["cams"], dc.table("zeros", V), (1000.0, 1000.0))
    bad_v = np.transpose(~c["valid"], (1, 0, 2))
    assert (r["poses"][..., 2][bad_v] == 0).all() and (r["poses"][..., 2][~bad_v] == 0.75).all()
    assert np.array_equal(r["rays"][bad_v], pin["rays"][bad_v])
    assert np.array_equal(r["poses"][..., :2], pin["poses"][..., :2])


def test_a_case_that_comes_near_a_fold_is_rejected():
    """the builder does not skip: a valid item whose Jacobian gets small makes the whole case fail"""
    yd = 0.9995 * dc.reach(dc.STRONG)
    _, _, valid, _, min_det = dc.undistort(np.array([yd]), np.array([0.0]), np.array(dc.STRONG))
    assert valid[0] and 0 < min_det[0] < dc.DET_MIN
    # and the point of the issue: beyond the fold is refused by det J <= 0
    _, _, valid, iters, min_det = dc.undistort(np.array([0.92]), np.array([0.0]), np.array(dc.STRONG))
    assert not valid[0] and min_det[0] <= 0 and iters[0] <= dc.MAX_ITER


def test_zero_coefficients_return_the_input_bits():
    c = dc.case(3, 4, 17, "zeros")
    px = c["pixels"].astype(np.float64)
    u = dc.undistort_pixels(px, c["cams"], c["dist"])
    assert u["valid"].all() and np.array_equal(u["pixels"], px)
    assert np.array_equal(dc.distort_pixels(px, c["cams"], c["dist"]), px)
    y = np.array([-0.7, 0.0, 0.3, 1e-300, 12.5])
    y0, y1, valid, iters, _ = dc.undistort(y, y[::-1].copy(), np.zeros(5))
    assert valid.all() and np.array_equal(y0, y) and np.array_equal(y1, y[::-1]) and (iters == 1).all()
    # prepare with zeros is the pinhole: the restatement of synth_cases
    from tests import synth_cases as sc
    r = dc.prepare(px, None, c["cams"], c["dist"], (1000.0, 1000.0))
    pts, cams = sc.scene(3, 4, 17, seed=3, focal=dc.FOCAL)
    ref = sc.synthesize(pts, cams, (1000.0, 1000.0), clip=False)
    np.testing.assert_allclose(r["rays"], ref["rays"], rtol=0, atol=2e-7)       # the pixels went through float32 here


def _params(name):
    m = re.search(r"\bint %s\(([^;]*)\);" % name, HEADER)
    assert m, "%s is not declared in include/mpl_hip.h" % name
    return [p.strip() for p in m.group(1).replace("\n", " ").split(",")]


def _ctype(param):
    """the ctypes type a C parameter of mpl_hip.h binds to"""
    if "*" in param:
        if re.match(r"float \*const \*", param):
            return C.POINTER(cabi._fp)
        if param.startswith("const mpl_synth_options *"):
            return C.POINTER(cabi.SynthOptions)
        return cabi._fp
    return {"int": C.c_int, "float": C.c_float, "double": C.c_double, "long long": C.c_longlong}[param.rsplit(" ", 1)[0]]


def test_header_prototypes_and_bindings_agree():
    lib = cabi.load()
    for name, n in (("mpl_undistort_points", 10), ("mpl_prepare_inputs_ex", 15), ("mpl_synthesize_views_ex", 20)):
        params = _params(name)
        fn = getattr(lib, name)
        assert len(params) == n and params[-1] == "void *stream" and fn.restype is C.c_int
        assert [_ctype(p) for p in params] == list(fn.argtypes), name
        assert name in cabi.EXPORTS
    # the _ex calls are their namesakes plus dist_dev right behind cams_dev
    for name, at in (("mpl_prepare_inputs", 3), ("mpl_synthesize_views", 2)):
        base, ex = _params(name), _params(name + "_ex")
        assert ex[:at] + ex[at + 1:] == base and ex[at] == "const double *dist_dev" and ex[at - 1] == "const double *cams_dev"
    codes = dict((n, int(v)) for n, v in re.findall(r"#define MPL_DISTORT_([A-Z_]+) (\d+)", HEADER))
    assert codes == {"REMOVE": cabi.DISTORT_REMOVE, "APPLY": cabi.DISTORT_APPLY}
    assert re.search(r"#define MPL_HIP_ABI_VERSION 14\b", HEADER) and cabi.ABI_VERSION == 14
    assert "distortion.hip" in __import__("openmpl_amd.build", fromlist=["SOURCES"]).SOURCES


def test_refusals_need_no_device():
    lib = cabi.load()
    p = lambda a: None if a is None else C.c_void_p(a)            # never dereferenced by a refused call

    def undistort(px=8, cams=8, dist=8, B=2, V=3, J=17, direction=cabi.DISTORT_REMOVE, out=8, valid=8):
        return lib.mpl_undistort_points(p(px), p(cams), p(dist), B, V, J, direction, p(out), p(valid), None)
    assert undistort(px=None) == -1 and undistort(cams=None) == -1 and undistort(dist=None) == -1 and undistort(out=None) == -1
    assert undistort(B=0) == -1 and undistort(V=0) == -1 and undistort(J=-1) == -1 and undistort(V=33) == -1
    assert undistort(direction=2) == -1 and undistort(direction=-1) == -1

    views = (cabi._fp * 33)(*([8] * 33))

    def prepare(px=8, cams=8, dist=8, B=2, V=3, J=17, w=1000.0, h=1000.0, tables=views):
        return lib.mpl_prepare_inputs_ex(p(px), None, p(cams), p(dist), B, V, J, w, h, 1, 1, tables, tables, tables, None)
    assert prepare(px=None) == -1 and prepare(cams=None) == -1 and prepare(tables=None) == -1
    assert prepare(B=0) == -1 and prepare(V=0) == -1 and prepare(J=0) == -1 and prepare(V=33) == -1
    assert prepare(w=0.0) == -1 and prepare(h=-1.0) == -1
    assert prepare(tables=(cabi._fp * 3)(None, 8, 8)) == -1

    def synth(opt, poses3d=8, cams=8, dist=8, B=2, V=3, J=17, out=8):
        return lib.mpl_synthesize_views_ex(p(poses3d), p(cams), p(dist), opt, None, None, None, None, None, B, V, J, None, None, None,
                                           p(out), None, None, None, None)

    def options(**kw):
        o = cabi.SynthOptions()
        o.img_w, o.img_h = 1000.0, 1000.0
        o.target_scale[:] = [1.0] * 3
        for k, v in kw.items():
            setattr(o, k, v)
        return C.byref(o)
    assert synth(options(), poses3d=None) == -1 and synth(options(), cams=None) == -1 and synth(None) == -1
    assert synth(options(), out=None) == -1
    assert synth(options(), B=0) == -1 and synth(options(), V=0) == -1 and synth(options(), J=0) == -1 and synth(options(), V=33) == -1
    assert synth(options(img_w=0.0)) == -1 and synth(options(penalize=4)) == -1


def test_pack_distortion_reads_the_reference_camera_dicts():
    from openmpl_amd.inputs import pack_distortion
    cams = [dict(fx=1.0, k=np.array([[0.1], [0.2], [0.3]]), p=np.array([[0.4], [0.5]])), dict(fx=1.0), dict(k=[1, 2, 3], p=(4, 5))]
    t = pack_distortion(cams, "cpu")
    assert t.dtype.is_floating_point and t.element_size() == 8 and tuple(t.shape) == (3, 5)
    assert t.tolist() == [[0.1, 0.2, 0.3, 0.4, 0.5], [0.0] * 5, [1.0, 2.0, 3.0, 4.0, 5.0]]
    with pytest.raises(RuntimeError, match="3 values"):
        pack_distortion([dict(k=[1, 2], p=[1, 2])], "cpu")
