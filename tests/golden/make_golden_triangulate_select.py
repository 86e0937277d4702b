"""Golden view selections for triangulate_rays_robust from the REFERENCE's own triangulate_poses (build container only).

MHP/multiviews/triangulate.py is loaded in place and triangulate_poses called as it stands.  It imports pymvg, which is not
installed: stand-ins for pymvg.camera_model and pymvg.multi_camera_system are put into sys.modules, whose find3d records the names
of the cameras it is handed ('camera_<view>') -- the selection of lines :94-102 is all that is taken from the call.

The reference never resets conf_threshold between the joints of one pose: a joint that lowered it hands the lower value on to the
joints after it.  triangulate_rays_robust starts every joint at conf_threshold (a joint's result does not depend on its
neighbours), so the function is called once per joint, on a one-joint pose.

Per V = 2, 4, 8: confs (V,J) float32 -- the kernel reads float32 -- on and off the 0.05 lattice the thresholds walk, with joints
where 0, 1 and 2 or more views pass at 0.85, one that needs the descent past 0 (where the reference starts selecting
zero-confidence views), one below -1, one with all confidences equal, a NaN; the start thresholds; sel (S,V,J) bool.
    python tests/golden/make_golden_triangulate_select.py
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle.ref_import import REFERENCE_ROOT  # noqa: E402

HANDED = []


class CameraModel:
    def __init__(self, name):
        self.name = name

    @classmethod
    def load_camera_from_M(cls, M, name=None, distortion_coefficients=None):
        return cls(name)


class MultiCameraSystem:
    def __init__(self, cameras):
        self.names = [c.name for c in cameras]

    def find3d(self, points_2d_set):
        assert all(name in self.names for name, _ in points_2d_set)
        HANDED.append([name for name, _ in points_2d_set])
        return np.zeros(3)


for mod, cls in (("pymvg.camera_model", CameraModel), ("pymvg.multi_camera_system", MultiCameraSystem)):
    m = types.ModuleType(mod)
    setattr(m, cls.__name__, cls)
    sys.modules[mod] = m
sys.modules["pymvg"] = types.ModuleType("pymvg")
sys.path.insert(0, os.path.join(REFERENCE_ROOT, "MHP"))
spec = importlib.util.spec_from_file_location("_ref_triangulate", os.path.join(REFERENCE_ROOT, "MHP", "multiviews", "triangulate.py"))
tri = importlib.util.module_from_spec(spec)
spec.loader.exec_module(tri)

STARTS = np.array([0.85, 0.5, 0.3, 0.0])
CAMERA = dict(R=np.eye(3), T=np.zeros((3, 1)), fx=1000.0, fy=1000.0, cx=500.0, cy=500.0, k=np.zeros((3, 1)), p=np.zeros((2, 1)))


def columns(V, rs):
    lattice = lambda n: (0.05 * rs.randint(0, 21, size=n)).astype(np.float32)      # noqa: E731
    cols = [np.full(V, 0.5), np.full(V, 0.0), np.full(V, 0.2), np.full(V, 0.85),    # all equal: below, at 0, on the lattice
            np.full(V, -5.0),                                                        # nothing passes above -1: the empty set
            np.r_[0.9, np.zeros(V - 1)],                                             # one passes; the second only below 0
            np.r_[0.9, np.full(V - 1, -0.3)],                                        # ... further down
            np.r_[0.9, 0.86, np.full(V - 2, 0.1)][:V],                               # two pass at 0.85
            np.r_[0.9, 0.84, np.full(V - 2, 0.1)][:V],                               # one passes at 0.85
            np.r_[0.8, 0.8, np.full(V - 2, 0.75)][:V],                               # float32 0.8 against 0.85 - 0.05
            np.r_[np.nan, 0.6, np.full(V - 2, 0.55)][:V],                            # a NaN never passes
            np.r_[np.inf, 0.1, np.full(V - 2, 0.05)][:V]]
    cols += [lattice(V) for _ in range(6)] + [rs.uniform(0.0, 1.0, size=V) for _ in range(6)]
    return np.stack([np.asarray(c, dtype=np.float32) for c in cols], axis=1)       # (V,J)


out = {}
for V in (2, 4, 8):
    confs = columns(V, np.random.RandomState(40 + V))
    J = confs.shape[1]
    sel = np.zeros((len(STARTS), V, J), bool)
    for s, start in enumerate(STARTS):
        for j in range(J):
            del HANDED[:]
            tri.triangulate_poses([CAMERA] * V, np.zeros((V, 1, 2)), confs[:, j:j + 1].astype(np.float64), conf_threshold=float(start))
            assert len(HANDED) == 1
            sel[s, [int(name.split("_")[1]) for name in HANDED[0]], j] = True
    with np.errstate(invalid="ignore"):
        passing = (confs > 0.85).sum(axis=0)
    assert {0, 1}.issubset(set(passing.tolist())) and (passing >= 2).any()
    tag = "v%d" % V
    out.update({tag + "_confs": confs, tag + "_starts": STARTS, tag + "_sel": sel})
    print(tag, "joints %d, selected per (start, joint):" % J, sel.sum(axis=1).tolist())
np.savez_compressed(os.path.join(HERE, "triangulate_select.npz"), **out)
