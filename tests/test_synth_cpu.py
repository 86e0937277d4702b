"""Synthesis of model inputs from 3D poses (openmpl_amd/synth.py): the float64 restatement against the reference-generated golden,
the properties of its counter-based streams, and the C prototype against its binding.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from openmpl_amd import cabi, detrng
from tests import synth_cases as sc

G = sc.golden()
COMBOS = [(t, p, c) for t in sc.TAGS for p in sc.PENALTIES for c in (True, False)]


@pytest.mark.parametrize("tag,penalize,clip", COMBOS)
def test_restatement_matches_reference_golden(tag, penalize, clip):
    poses3d, cams, wh, kw = sc.golden_case(G, tag, penalize)
    ref = sc.synthesize(poses3d, cams, wh, clip=clip, **kw)
    want = sc.golden_outputs(G, tag, penalize, clip)
    got = {k: ref[k].astype(np.float32) for k in ("poses", "rays", "pixels", "pixels_clean", "target", "centers")}
    sc.assert_matches(got, {k: v.astype(np.float64) for k, v in want.items()})
    assert ref["margin"].min() > 1e-6          # no stored item sits on a decision (the image borders are 1e-3 px away by construction)


def test_golden_is_small():
    assert os.path.getsize(os.path.join(sc.GOLD, "synth.npz")) < 200 * 1024


def _own(B0, B1, seed=3, first_index=0):
    poses3d, cams = sc.scene(12, 4, 17, seed=2, focal=2400.0)
    return sc.synthesize(poses3d[B0:B1], cams, (1000.0, 1000.0), seed=seed, first_index=first_index + B0, rotate=True,
                         room=(-0.4, 0.4, -0.3, 0.3), noise_level=6.0, penalize="exp_error", penalize_a=0.95, penalize_b=0.04,
                         clip=False, missing_level=0.2, target_scale=(2.0, 2.0, 1.0), target_offset=(0.0, 0.1, 1.0))


def test_own_streams_do_not_depend_on_batching():
    whole = _own(0, 12)
    parts = [_own(0, 4), _own(4, 8), _own(8, 12)]
    for k in ("poses", "rays", "centers"):
        assert np.array_equal(whole[k], np.concatenate([p[k] for p in parts], axis=1)), k
    for k in ("target", "pixels", "pixels_clean", "depth", "conf"):
        assert np.array_equal(whole[k], np.concatenate([p[k] for p in parts], axis=0)), k
    assert not np.array_equal(whole["pixels"], _own(0, 12, seed=4)["pixels"])
    assert (whole["conf"] == 0).any() and (whole["conf"] > 0).any()


def test_uniform_draws_are_detrng_uniform01():
    n = 5000
    for name, lane in (("synth.missing", 0), ("synth.noise", 1), ("synth.room", 1)):
        assert np.array_equal(sc.draw(7, name, lane, np.arange(n)), detrng.uniform01(7, name, n, lane=lane))
    # any counter, in any order and shape
    idx = np.array([[4999, 0], [17, 1234]])
    assert np.array_equal(sc.draw(7, "synth.rot", 0, idx), detrng.uniform01(7, "synth.rot", n)[idx])


def test_normal_pair_moments():
    N = 100000
    n = sc.normal_pair(11, np.arange(N))
    assert n.shape == (N, 2) and np.isfinite(n).all()
    for k in range(2):
        assert abs(n[:, k].mean()) < 4 / np.sqrt(N)
        assert abs(n[:, k].var() - 1.0) < 4 * np.sqrt(2.0 / N)


def test_behind_the_camera_is_dropped_before_the_noise():
    poses3d, cams = sc.scene(2, 2, 5, seed=1)
    poses3d[0, 0] = cams[0, 13:16] - 2.0 * cams[0, 10:13]          # two units behind camera 0
    for clip in (True, False):
        r = sc.synthesize(poses3d, cams, (1000.0, 1000.0), noise_level=5.0, penalize="linear", penalize_a=0.1, penalize_b=1.0, clip=clip)
        assert r["depth"][0, 0, 0] < 0 and r["conf"][0, 0, 0] == 0
        assert not r["pixels"][0, 0, 0].any() and not r["pixels_clean"][0, 0, 0].any()


def test_header_prototype_and_binding_agree():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mpl_hip.h")).read()
    m = re.search(r"\bint mpl_synthesize_views\(([^;]*)\);", header)
    assert m, "mpl_synthesize_views is not declared in include/mpl_hip.h"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert len(params) == 19 and params[0] == "const float *poses3d" and params[-1] == "void *stream"
    lib = cabi.load()
    assert len(lib.mpl_synthesize_views.argtypes) == len(params)
    assert lib.mpl_synthesize_views.restype is C.c_int
    codes = dict((n.lower(), int(v)) for n, v in re.findall(r"#define MPL_SYNTH_PENALIZE_([A-Z_]+) (\d+)", header))
    assert codes == cabi.SYNTH_PENALIZE
    # the options struct: field for field
    body = re.search(r"typedef struct mpl_synth_options \{(.*?)\} mpl_synth_options;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.sub(r"\[\d+\]", "", n.strip()) for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [f[0] for f in cabi.SynthOptions._fields_]
    assert C.sizeof(cabi.SynthOptions) == 6 * 4 + 10 * 8 + 6 * 8 + 7 * 8
    assert re.search(r"#define MPL_HIP_ABI_VERSION 14\b", header) and cabi.ABI_VERSION == 14

    # the refusals need no device: they come before any launch
    def call(opt, poses3d=8, cams=8, B=2, V=3, J=17, out=8, views=None):
        p = lambda a: None if a is None else C.c_void_p(a)            # never dereferenced by a refused call
        return lib.mpl_synthesize_views(p(poses3d), p(cams), opt, None, None, None, None, None, B, V, J, views, views, views, p(out), None,
                                        None, None, None)

    def options(**kw):
        o = cabi.SynthOptions()
        o.img_w, o.img_h = 1000.0, 1000.0
        o.target_scale[:] = [1.0] * 3
        for k, v in kw.items():
            setattr(o, k, v)
        return C.byref(o)
    assert call(options(), poses3d=None) == -1 and call(options(), cams=None) == -1 and call(None) == -1
    assert call(options(), out=None) == -1
    assert call(options(), B=0) == -1 and call(options(), V=0) == -1 and call(options(), J=0) == -1 and call(options(), V=33) == -1
    assert call(options(img_w=0.0)) == -1 and call(options(img_h=-1.0)) == -1
    assert call(options(penalize=4)) == -1 and call(options(penalize=-1)) == -1
    o = cabi.SynthOptions()
    o.img_w, o.img_h = 1000.0, 1000.0
    o.target_scale[:] = [1.0, 0.0, 1.0]
    assert call(C.byref(o)) == -1
    null_views = (cabi._fp * 3)(None, 8, 8)
    assert call(options(), views=null_views) == -1
