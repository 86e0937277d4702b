"""Float64 restatement of openmpl_amd/synth.py (csrc/synth.hip) and the scenes of its tests (TEST INFRASTRUCTURE ONLY).

numpy float64 on the float32 inputs the kernel reads, nothing rounded: the tests round once to float32 where they compare.  It is
pinned by tests/golden/synth.npz, which the reference's own rotate_pose, world_to_cam, cam_to_image, normalize_screen_coordinates
and create_3d_ray_coords produced (tests/golden/make_golden_synth.py).  The random streams are those of openmpl_amd.detrng:
draw i of a stream is _mix(key + (i + 1) * GOLD) >> 11, scaled to [0,1); the normal pair is Box-Muller on two lanes.
"""
import os

import numpy as np

from openmpl_amd import detrng

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TAGS = ("h36m", "cmu", "raw")
PENALTIES = ("none", "exp_error", "linear", "exp_sqrt")
Z_MIN = 1e-9             # a joint at z_cam <= Z_MIN: confidence 0, pixel (0,0), steps 3 to 5 skipped


def draw(seed, name, lane, idx):
    """element idx (any integer array) of the stream (seed, name, lane): detrng.uniform01 at arbitrary counters"""
    key = detrng._stream_key(seed, name, lane)
    idx = np.asarray(idx).astype(np.uint64)
    with np.errstate(over="ignore"):
        z = detrng._mix(key + (idx + np.uint64(1)) * detrng._GOLD)
    return (z >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def normal_pair(seed, idx):
    """Box-Muller on lanes 0 / 1 of "synth.noise" -> (..., 2)"""
    u1, u2 = 1.0 - draw(seed, "synth.noise", 0, idx), draw(seed, "synth.noise", 1, idx)
    r, t = np.sqrt(-2.0 * np.log(u1)), 2.0 * np.pi * u2
    return np.stack([r * np.cos(t), r * np.sin(t)], axis=-1)


def penalty(mode, d, a, b):
    if mode == "exp_error":
        return a * np.exp(-b * d)
    if mode == "linear":
        return a * d + b
    if mode == "exp_sqrt":
        return np.exp(-d / 2.0)
    assert mode == "none", mode
    return np.ones_like(d)


def synthesize(poses3d, cams, image_size, seed=0, first_index=0, rotate=False, room=None, noise_level=0.0, penalize="none",
               penalize_a=1.0, penalize_b=0.0, clip=True, missing_level=0.0, conf=None, normalize_inputs=True, normalize_cameras=True,
               target_scale=None, target_offset=None, rotation_deg=None, translation=None, noise=None, missing_u=None):
    """-> dict of float64 arrays: poses, rays (V,B,J,3), centers (V,B,1,3), target (B,J,3), pixels, pixels_clean (B,V,J,2), depth,
    conf (B,V,J), and margin (B,V,J): how far the item is from the nearest decision it takes (pixels for the image borders)."""
    X = np.asarray(poses3d, dtype=np.float64).copy()
    cams = np.asarray(cams, dtype=np.float64)
    B, J, _ = X.shape
    V = cams.shape[0]
    w, h = float(image_size[0]), float(image_size[1])
    gpose = first_index + np.arange(B)
    # 1. placement
    if rotation_deg is not None or rotate:
        deg = np.asarray(rotation_deg, dtype=np.float64) if rotation_deg is not None else draw(seed, "synth.rot", 0, gpose) * 360.0
        a = deg * (np.pi / 180.0)
        ca, sa = np.cos(a)[:, None], np.sin(a)[:, None]
        X[..., 0], X[..., 1] = X[..., 0] * ca - X[..., 1] * sa, X[..., 0] * sa + X[..., 1] * ca
    if translation is not None:
        X = X + np.asarray(translation, dtype=np.float64)[:, None, :]
    elif room is not None:
        X[..., 0] += (draw(seed, "synth.room", 0, gpose) * (room[1] - room[0]) + room[0])[:, None]
        X[..., 1] += (draw(seed, "synth.room", 1, gpose) * (room[3] - room[2]) + room[2])[:, None]
    # 2. projection
    fx, fy, cx, cy = (cams[:, k][None, :, None] for k in range(4))
    R, t = cams[:, 4:13].reshape(V, 3, 3), cams[:, 13:16]
    xc = np.einsum("vxy,bvjy->bvjx", R, X[:, None, :, :] - t[None, :, None, :])
    zc = xc[..., 2]
    front = zc > Z_MIN
    with np.errstate(divide="ignore", invalid="ignore"):
        x = np.where(front, fx * xc[..., 0] / zc + cx, 0.0)
        y = np.where(front, fy * xc[..., 1] / zc + cy, 0.0)
    cf = np.where(front, np.ones((B, V, J)) if conf is None else np.asarray(conf, dtype=np.float64).reshape(B, V, J), 0.0)
    clean = np.stack([x, y], axis=-1)
    margin = np.abs(zc - Z_MIN)
    gitem = (gpose[:, None, None] * V + np.arange(V)[None, :, None]) * J + np.arange(J)[None, None, :]
    # 3. noise and penalty
    if noise_level != 0.0:
        n = (np.asarray(noise, dtype=np.float64) if noise is not None else normal_pair(seed, gitem)) * noise_level
        xn, yn = x + n[..., 0], y + n[..., 1]
        cfn = cf * penalty(penalize, np.sqrt(n[..., 0] ** 2 + n[..., 1] ** 2), penalize_a, penalize_b)
    else:
        xn, yn, cfn = x, y, cf
    for c, edges in ((xn, (0.0, w - 1.0, w)), (yn, (0.0, h - 1.0, h))):
        for e in edges:
            margin = np.minimum(margin, np.where(front, np.abs(c - e), np.inf))
    # 4. visibility
    if clip:
        inside = (0 < xn) & (xn < w - 1) & (0 < yn) & (yn < h - 1)
        cfv = np.where(inside, cfn, 0.0)
        xv, yv = np.clip(xn, 0, w - 1), np.clip(yn, 0, h - 1)
    else:
        margin = np.minimum(margin, np.where(front & (cfn != 0), np.abs(cfn), np.inf))
        out = (np.minimum(xn, yn) < 0) | (xn >= w) | (yn >= h)
        cfv = np.where((cfn > 0) & out, 0.0, cfn)
        xv, yv = np.where(cfv > 0, xn, 0.0), np.where(cfv > 0, yn, 0.0)
    # 5. missing joints
    if missing_level > 0.0:
        u = np.asarray(missing_u, dtype=np.float64) if missing_u is not None else draw(seed, "synth.missing", 0, gitem)
        margin = np.minimum(margin, np.where(front, np.abs(u - missing_level) * 1e3, np.inf))     # 1e-9 in u counts as 1e-6 px
        keep = np.where(u < missing_level, 0.0, 1.0)
        cfv, xv, yv = cfv * keep, xv * keep, yv * keep
    x, y, cf = np.where(front, xv, 0.0), np.where(front, yv, 0.0), np.where(front, cfv, 0.0)
    pixels = np.stack([x, y], axis=-1)
    # 6. normalisation, rays, centres (the arithmetic of prepare_inputs)
    if normalize_inputs:
        x, y = (x / w) * 2.0 - 1.0, (y / w) * 2.0 - h / w
        if normalize_cameras:
            cx, cy = (cx / w) * 2.0 - 1.0, (cy / w) * 2.0 - h / w
            fx, fy = fx / w * 2.0, fy / w * 2.0
    u = np.stack([(x - cx) / fx, (y - cy) / fy, np.ones_like(x)], axis=-1)                    # (B,V,J,3)
    rays = np.einsum("vyx,bvjy->vbjx", R, u) + t[:, None, None, :]                             # R^T u + t
    poses = np.transpose(np.stack([x, y, cf], axis=-1), (1, 0, 2, 3))
    centers = np.broadcast_to(t[:, None, None, :], (V, B, 1, 3)).copy()
    # 7. target
    sc = np.ones(3) if target_scale is None else np.asarray(target_scale, dtype=np.float64)
    of = np.zeros(3) if target_offset is None else np.asarray(target_offset, dtype=np.float64)
    return dict(poses=poses, rays=rays, centers=centers, target=(X - of) / sc, placed=X, pixels=pixels, pixels_clean=clean, depth=zc,
                conf=cf, margin=margin)


# --------------------------------------------------------------------------------------------------------------- scenes
def look_at(centre, aim):
    """world->camera rotation of a camera at `centre` whose optical axis points at `aim` (z up in the world)"""
    z = (aim - centre) / np.linalg.norm(aim - centre)
    x = np.cross(z, np.array([0.0, 0.0, 1.0]))
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z])


def scene(B, V, J, seed, image_size=(1000.0, 1000.0), focal=900.0):
    """`B` poses of about 1 unit extent around (0, 0, 1) and `V` cameras on a ring of 3 .. 6 units, looking at them: poses3d (B,J,3)
    float32, cams (V,16) float64 in the layout of pack_cameras.  Everything comes from detrng."""
    poses = detrng.uniform(seed, "scene.pose.%d.%d" % (B, J), (B, J, 3), -0.5, 0.5) + np.array([0.0, 0.0, 1.0], np.float32)
    az = 2 * np.pi * (np.arange(V) + detrng.uniform(seed, "scene.az.%d" % V, (V,), 0.0, 0.5).astype(np.float64)) / max(V, 3)
    rad = detrng.uniform(seed, "scene.rad.%d" % V, (V,), 3.0, 6.0).astype(np.float64)
    hgt = detrng.uniform(seed, "scene.h.%d" % V, (V,), 0.5, 3.0).astype(np.float64)
    w, h = image_size
    cams = []
    for v in range(V):
        c = np.array([rad[v] * np.cos(az[v]), rad[v] * np.sin(az[v]), hgt[v]])
        cams.append(np.concatenate([[focal + 37.0 * (v % 5), focal - 11.0 * (v % 7), w / 2 + 13.0 * (v % 3), h / 2 - 7.0 * (v % 4)],
                                    look_at(c, np.array([0.0, 0.0, 1.0])).reshape(-1), c]))
    return poses.astype(np.float32), np.stack(cams)


def golden():
    g = np.load(os.path.join(GOLD, "synth.npz"))
    return {k: g[k] for k in g.files}


def golden_case(g, tag, penalize="none"):
    """the inputs of one case: poses3d, cams, image size, and the rest as keyword arguments of synthesize() (numpy arrays)"""
    conf = g[tag + "_conf_in"] if tag + "_conf_in" in g else None
    kw = dict(rotation_deg=g[tag + "_rotation_deg"], translation=g[tag + "_translation"], noise=g[tag + "_noise"],
              missing_u=g[tag + "_missing_u"], noise_level=float(g[tag + "_levels"][0]), missing_level=float(g[tag + "_levels"][1]),
              penalize=penalize, penalize_a=float(g[tag + "_ab_" + penalize][0]), penalize_b=float(g[tag + "_ab_" + penalize][1]),
              conf=conf, normalize_inputs=bool(g[tag + "_normalize"][0]), normalize_cameras=bool(g[tag + "_normalize"][1]),
              target_scale=g[tag + "_target_scale"], target_offset=g[tag + "_target_offset"])
    return g[tag + "_poses3d"], g[tag + "_cams"], (float(g[tag + "_wh"][0]), float(g[tag + "_wh"][1])), kw


def golden_outputs(g, tag, penalize, clip):
    """the stored outputs of one combination: arrays that do not depend on the penalty are stored once per visibility mode"""
    mode = "clip" if clip else "zero"

    def get(name):
        k = "%s_%s_%s_%s" % (tag, mode, penalize, name)
        return g[k] if k in g else g["%s_%s_none_%s" % (tag, mode, name)]
    return dict(poses=get("poses"), rays=get("rays"), pixels=get("pixels"), centers=g[tag + "_centers"], target=g[tag + "_target"],
                pixels_clean=g[tag + "_pixels_clean"])


def assert_matches(got, ref, skip=None):
    """got / ref: dicts of float32 / float64 arrays by output name; the tolerances of the issue (one fp32 rounding per side).
    skip: (B,V,J) mask of items left out (views outputs are (V,B,J,.), pixel outputs (B,V,J,.))"""
    keep_b = None if skip is None else ~skip
    keep_v = None if skip is None else ~np.transpose(skip, (1, 0, 2))
    for name, rtol, atol, keep in (("poses", 2e-7, 2e-7, keep_v), ("rays", 3e-7, 5e-7, keep_v), ("pixels", 2e-7, 2e-7, keep_b),
                                   ("pixels_clean", 2e-7, 2e-7, keep_b), ("target", 2e-7, 2e-7, None), ("depth", 2e-7, 2e-7, keep_b)):
        if name not in got or got[name] is None or name not in ref:
            continue
        a, r = np.asarray(got[name]), np.asarray(ref[name]).astype(np.float32)
        assert a.dtype == np.float32 and a.shape == r.shape, (name, a.dtype, a.shape, r.shape)
        if keep is not None:
            a, r = a[keep], r[keep]
        np.testing.assert_allclose(a, r, rtol=rtol, atol=atol, err_msg=name)
    if "centers" in got and got["centers"] is not None:
        np.testing.assert_array_equal(np.asarray(got["centers"]), np.asarray(ref["centers"]).astype(np.float32))
    if "poses" in got and got["poses"] is not None:            # a confidence the contract sets to 0 is exactly 0
        a, r = np.asarray(got["poses"])[..., 2], np.asarray(ref["poses"])[..., 2]
        if keep_v is not None:
            a, r = a[keep_v], r[keep_v]
        assert np.array_equal(a == 0, r == 0)
