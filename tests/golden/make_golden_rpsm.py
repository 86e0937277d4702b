"""Golden vectors for the recursive pictorial structure model (openmpl_amd/rpsm.py) from the REFERENCE's own functions (build
container only): compute_grid, compute_unary_term, compute_pairwise_constrain, infer and rpsm of lib/multiviews/pictorial.py with
HumanBody of body.py and project_pose of cameras.py, loaded in place, on the cases of tests/rpsm_cases.GOLDEN_CASES.

numexpr and OpenCV are not installed where this runs: `numexpr` is stubbed with an empty module (pictorial.py only imports it), and
the stub `cv2` provides getAffineTransform as the float64 solve of the three point pairs that make_golden_heatmaps.py uses.  The
pairwise dictionary of the first round is built vectorised from the reference's own grid with the reference's rule (the norm of the
difference, | d - limb | <= tolerance; its Python double loop over 4096^2 pairs would take hours), as scipy csr matrices, which infer
accepts; on the 4^3 case it is checked entry by entry against compute_pairwise_constrain itself.  The bins, which rpsm does not
return, are recorded at its calls of infer.  Only results are stored: the inputs are regenerated from seeds at test time (the attempt
that met conditions (a) and (b) of rpsm_cases is stored with them).  python tests/golden/make_golden_rpsm.py"""
import os
import sys
import time
import types

import numpy as np
import scipy.sparse

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import rpsm_cases as rc  # noqa: E402


def get_affine_transform(src, dst):
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    assert src.shape == (3, 2) and dst.shape == (3, 2)
    return np.linalg.solve(np.concatenate([src, np.ones((3, 1))], axis=1), dst).T        # (2,3): dst = M [x, y, 1]


cv2 = types.ModuleType("cv2")
cv2.getAffineTransform = get_affine_transform
sys.modules["cv2"] = cv2
sys.modules["numexpr"] = types.ModuleType("numexpr")

LIB = "/root/reference/MPL/lib"
sys.path.insert(0, LIB)
from multiviews import pictorial  # noqa: E402
from multiviews.body import HumanBody  # noqa: E402

seen = []
ref_infer = pictorial.infer


def recording_infer(unary, pairwise, body, config):
    out = ref_infer(unary, pairwise, body, config)
    seen.append([idx for _, idx in out])
    return out


pictorial.infer = recording_infer


def ref_cams(inp):
    cams = []
    for v, c in enumerate(inp["cams"]):
        d = np.zeros(5) if inp["dist"] is None else inp["dist"][v]
        cams.append(dict(R=c[4:13].reshape(3, 3), T=c[13:16].reshape(3, 1), fx=c[0:1], fy=c[1:2], cx=c[2:3], cy=c[3:4],
                         k=d[:3].reshape(3, 1), p=d[3:].reshape(2, 1)))
    return cams


def first_pairwise(grid, limb, tol, body):
    gx = grid[:, None, :] - grid[None, :, :]
    d = np.sqrt((gx ** 2).sum(-1))
    del gx
    return {(n["idx"], c): scipy.sparse.csr_matrix((np.abs(d - float(limb[(n["idx"], c)])) <= tol).astype(np.float64))
            for n in body.skeleton for c in n["children"]}


out = {}
body = HumanBody()
for tag in rc.GOLDEN_CASES:
    t0 = time.time()
    inp, ref, attempt = rc.case(tag)                     # conditions (a) and (b) hold on the restatement
    kw = inp["kw"]
    cfg = types.SimpleNamespace(
        NETWORK=types.SimpleNamespace(IMAGE_SIZE=np.array(inp["image_size"]), HEATMAP_SIZE=np.array(inp["hm"].shape[-2:][::-1])),
        PICT_STRUCT=types.SimpleNamespace(FIRST_NBINS=kw["first_nbins"], RECUR_NBINS=kw["recur_nbins"], RECUR_DEPTH=kw["recur_depth"],
                                          GRID_SIZE=kw["grid_size"], LIMB_LENGTH_TOLERANCE=kw["tolerance"]),
        DATASET=types.SimpleNamespace(ROOTIDX=0))
    B = inp["hm"].shape[0]
    poses, bins = [], []
    for b in range(B):
        limb = {(q, j): float(inp["limb"].reshape(-1, 17)[min(b, inp["limb"].ndim - 1) * 0 + (b if inp["limb"].ndim == 2 else 0), j])
                for j, q in enumerate(inp["parents"]) if q != -1}
        boxes = [dict(center=inp["center"][b, v], scale=inp["scale"][b, v]) for v in range(inp["hm"].shape[1])]
        hm = inp["hm"][b].astype(np.float64)
        centre = inp["root_center"][b].astype(np.float64)
        grid = pictorial.compute_grid(kw["grid_size"], centre, kw["first_nbins"])
        assert np.array_equal(grid, rc.grid(kw["grid_size"], centre, kw["first_nbins"]))
        pairwise = first_pairwise(grid, limb, kw["tolerance"], body)
        if tag == "g4" and b == 0:
            own = pictorial.compute_pairwise_constrain(body.skeleton, limb, [grid] * 17, kw["tolerance"])
            assert all(np.array_equal(own[k], pairwise[k].toarray()) for k in own) and len(own) == 16
            u = pictorial.compute_unary_term(hm, [grid], boxes, ref_cams(inp), cfg.NETWORK.IMAGE_SIZE)
            mine = rc.unary(inp["hm"][b], [grid], inp["center"][b], inp["scale"][b], inp["cams"], inp["image_size"], inp["dist"])
            print(tag, "unary: restatement vs reference, worst relative difference %.2e" % np.max(np.abs(mine - np.array(u)) / np.abs(np.array(u)).max()))
        if b == 0:
            u = pictorial.compute_unary_term(hm[:, [0, 9]], [grid], boxes, ref_cams(inp), cfg.NETWORK.IMAGE_SIZE)
            out[tag + "_unary_0_9"] = np.stack(u)
        del seen[:]
        pose = pictorial.rpsm(ref_cams(inp), hm, boxes, centre, limb, pairwise, cfg)
        assert len(seen) == 1 + kw["recur_depth"]
        poses.append(pose)
        bins.append(np.array(seen, np.int32))
    poses, bins = np.stack(poses), np.stack(bins)
    same = np.array_equal(bins, ref["bins"])
    print("%s: attempt %d, %d pose(s), %.1f s; bins equal the restatement's: %s; poses differ by at most %.2e; margin (a) %.2e, (b) %.2e"
          % (tag, attempt, B, time.time() - t0, same, np.abs(poses - ref["poses"]).max(), rc.boundary_distance(inp), ref["margin"]))
    assert same and np.abs(poses - ref["poses"]).max() <= 1e-9
    out[tag + "_poses"], out[tag + "_bins"], out[tag + "_attempt"] = poses, bins, np.array(attempt)
    out[tag + "_energy"] = ref["energy"]                 # the restatement's (the reference does not return it)
    out[tag + "_margins"] = np.array([rc.boundary_distance(inp), ref["margin"]])
path = os.path.join(HERE, "rpsm.npz")
np.savez_compressed(path, **out)
print(path, os.path.getsize(path), "bytes")
