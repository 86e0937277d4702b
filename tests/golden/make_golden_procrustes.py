"""Golden vectors for the Procrustes kernel (openmpl_amd/procrustes.py) from the REFERENCE's own code (build container only).

lib/utils/pose_utils.py is loaded in place (sklearn, which it imports for another function, is stubbed when absent).  Per case
(J = 3, 4, 17 joints, 6 poses): targets a pose about 1 m across somewhere in a room, predictions a random similarity of the target
plus 5 % noise, both float32 from detrng; poses 1 and 4 of every case are mirrored, so that reflection='best' returns det R = -1
there (asserted).  PoseUtils().procrustes(A, B, scaling, reflection) is called per pose on float64 casts of those float32 inputs,
under all six (scaling on / off) x (reflection best / False / True), and d, Z, rotation, scale and translation are stored.

No stored pose is near a decision edge: |det R| is 1, and s[1] / s[0], s[2] / s[0] of A0n^T B0n are at least 1e-3 (the kernel's
collinear / coplanar thresholds are 1e-12).  J = 3 is the exception that cannot be otherwise: three centred points span a plane, so
s[2] is round-off (asserted: s[2] / s[0] <= 1e-14, as far below the threshold as the others are above it).  There both signs of
the third singular pair fit equally well -- d, Z and scale are the same for both (asserted) -- and which one 'best' returns is up
to numpy's SVD; the forced modes are decided by the sign of det R alone and stay unique.  The tests compare the kernel's 'best'
at J = 3 (the proper rotation, its documented coplanar rule) with the rotation and translation stored for reflection=False.
    python tests/golden/make_golden_procrustes.py
"""
import importlib.util
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from openmpl_amd import detrng  # noqa: E402
from oracle.ref_import import REFERENCE_ROOT  # noqa: E402

try:
    import sklearn.preprocessing  # noqa: F401
except ImportError:      # pose_utils.py:9 imports `normalize` for estimate_camera only
    sk, pre = types.ModuleType("sklearn"), types.ModuleType("sklearn.preprocessing")
    pre.normalize = lambda x: x / np.linalg.norm(x, axis=1, keepdims=True)
    sk.preprocessing = pre
    sys.modules["sklearn"], sys.modules["sklearn.preprocessing"] = sk, pre

warnings.simplefilter("ignore", SyntaxWarning)        # `reflection is not 'best'` (:111)
spec = importlib.util.spec_from_file_location("_ref_pose_utils", os.path.join(REFERENCE_ROOT, "MPL", "lib", "utils", "pose_utils.py"))
pose_utils = importlib.util.module_from_spec(spec)
spec.loader.exec_module(pose_utils)
procrustes = pose_utils.PoseUtils().procrustes

SEED, B, MIRRORED = 31, 6, (1, 4)
MODES = [(scaling, reflection) for scaling in (True, False) for reflection in ("best", False, True)]
TAGS = {"best": "best", False: "off", True: "on"}


def rotations(tag):
    """B proper rotations from detrng (Gram-Schmidt of a random matrix)"""
    m = detrng.normal(SEED, "rot." + tag, (B, 3, 3), 0.0, 1.0).astype(np.float64)
    out = []
    for b in range(B):
        q, r = np.linalg.qr(m[b])
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, 2] *= -1
        out.append(q)
    return np.stack(out)


out = {}
for J in (3, 4, 17):
    tag = "j%d" % J
    tgt = (detrng.uniform(SEED, "tgt." + tag, (B, J, 3), -0.5, 0.5).astype(np.float64)
           + detrng.uniform(SEED, "room." + tag, (B, 1, 3), -2.0, 2.0)).astype(np.float32)
    s = detrng.uniform(SEED, "scale." + tag, (B,), 0.5, 2.0).astype(np.float64)
    R = rotations(tag)
    for b in MIRRORED:
        R[b] = R[b] @ np.diag([1.0, 1.0, -1.0])
    t = detrng.uniform(SEED, "shift." + tag, (B, 3), -1.0, 1.0).astype(np.float64)
    pred = s[:, None, None] * np.einsum("bjx,bxy->bjy", tgt.astype(np.float64), R) + t[:, None, :]
    pred = (pred + 0.05 * s[:, None, None] * 0.3 * detrng.normal(SEED, "noise." + tag, (B, J, 3), 0.0, 1.0)).astype(np.float32)
    out[tag + "_pred"], out[tag + "_target"] = pred, tgt

    # the decision edges, on the matrix the reference decomposes
    for b in range(B):
        A0, B0 = tgt[b].astype(np.float64), pred[b].astype(np.float64)
        A0, B0 = A0 - A0.mean(0), B0 - B0.mean(0)
        sv = np.linalg.svd(np.dot((A0 / np.sqrt((A0 ** 2).sum())).T, B0 / np.sqrt((B0 ** 2).sum())), compute_uv=False)
        assert sv[1] / sv[0] >= 1e-3 and (sv[2] / sv[0] >= 1e-3 if J > 3 else sv[2] / sv[0] <= 1e-14), (tag, b, sv)

    for scaling, reflection in MODES:
        m = "%s_%s_%s" % (tag, "s" if scaling else "r", TAGS[reflection])
        d, Z, rot, sc, tr = np.zeros(B), np.zeros((B, J, 3)), np.zeros((B, 3, 3)), np.zeros(B), np.zeros((B, 3))
        for b in range(B):
            d[b], Z[b], tf = procrustes(tgt[b].astype(np.float64), pred[b].astype(np.float64), scaling=scaling, reflection=reflection)
            rot[b], sc[b], tr[b] = tf["rotation"], tf["scale"], tf["translation"]
        det = np.linalg.det(rot)
        assert np.abs(np.abs(det) - 1).max() < 1e-9, (m, det)
        if reflection == "best":
            if J > 3:
                assert sorted(np.nonzero(det < 0)[0].tolist()) == list(MIRRORED), (m, det)
            best = (d, Z, sc)
        else:
            if J == 3:      # three points: the reflected and the proper fit are the same fit
                assert all(np.abs(x - y).max() <= 1e-12 * np.abs(y).max() for x, y in zip((d, Z, sc), best)), m
            assert ((det < 0) == bool(reflection)).all(), (m, det)
        # Z is the transform the reference reports
        assert np.abs(Z - (sc[:, None, None] * np.einsum("bjx,bxy->bjy", pred.astype(np.float64), rot) + tr[:, None, :])).max() < 1e-12
        out.update({m + "_d": d, m + "_Z": Z, m + "_rotation": rot, m + "_scale": sc, m + "_translation": tr})
        print(m, "d %.3e .. %.3e  det %s" % (d.min(), d.max(), "".join("+" if x > 0 else "-" for x in det)))
np.savez_compressed(os.path.join(HERE, "procrustes.npz"), **out)
