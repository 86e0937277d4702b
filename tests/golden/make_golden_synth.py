"""Golden vectors for the synthesis of model inputs from 3D poses (openmpl_amd/synth.py) from the REFERENCE's own code (build
container only).  lib/utils/calib.py, lib/utils/utils_amass.py and lib/dataset/joints_dataset_mpl.py are loaded in place (stub
`cv2`); rotate_pose, world_to_cam, cam_to_image, JointsDataset.normalize_screen_coordinates and create_3d_ray_coords are called
themselves.  The steps that exist only as lines inside __getitem__ are written out below with their line numbers.

Cases: B = 5, V = 3, J = 17 at 1000x1000 normalised ("h36m"), 1920x1080 normalised ("cmu") and 1000x1000 raw ("raw"), each under
the four penalty modes and both visibility modes.  Poses and cameras come from detrng; the four random inputs (rotation,
translation, noise, missing draws) come from a seeded numpy generator, are rounded to float32 (what the kernel reads) and stored.
Arrays that turn out not to depend on the penalty are stored once per visibility mode.      python tests/golden/make_golden_synth.py
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from openmpl_amd import detrng  # noqa: E402
from oracle.ref_import import REFERENCE_ROOT  # noqa: E402
from tests import synth_cases as sc  # noqa: E402

LIB = os.path.join(REFERENCE_ROOT, "MPL", "lib")
sys.modules.setdefault("cv2", types.ModuleType("cv2"))
sys.path.insert(0, LIB)


def load(name, *path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(LIB, *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


calib = load("_ref_calib", "utils", "calib.py")
amass = load("_ref_utils_amass", "utils", "utils_amass.py")
DS = load("_ref_joints_dataset", "dataset", "joints_dataset_mpl.py").JointsDataset_MPL

B, V, J = 5, 3, 17
NOISE_LEVEL, MISSING_LEVEL = 8.0, 0.15
PEN = {"none": (1.0, 0.0), "exp_error": (0.9, 0.05), "linear": (-0.05, 1.0), "exp_sqrt": (1.0, 0.0)}
ROOM = (-0.3, 0.3, -0.2, 0.4)                      # room_min_x, room_max_x, room_min_y, room_max_y
T_SCALE, T_OFFSET = np.array([2.0, 2.5, 1.25]), np.array([0.1, -0.2, 1.0])
rs = np.random.RandomState(20240)
out = {}

for tag, (w, h), norm_in, norm_cam, focal in (("h36m", (1000, 1000), True, True, 4400.0), ("cmu", (1920, 1080), True, True, 5800.0),
                                               ("raw", (1000, 1000), False, False, 4400.0)):
    fake = types.SimpleNamespace(downsample=1, use_grid=False, use_t=True, bug_test=False, image_size=[w, h])
    poses3d = (detrng.uniform(31, "pose." + tag, (B, J, 3), -0.5, 0.5) + np.array([0.0, 0.0, 1.0], np.float32)).astype(np.float32)
    az = np.deg2rad(115.0) * (np.arange(V) + detrng.uniform(31, "az." + tag, (V,), 0.0, 0.4).astype(np.float64))
    rad = detrng.uniform(31, "rad." + tag, (V,), 3.0, 6.0).astype(np.float64)
    hgt = detrng.uniform(31, "h." + tag, (V,), 0.5, 2.5).astype(np.float64)
    cams, cam_rows = [], []
    for v in range(V):
        c = np.array([rad[v] * np.cos(az[v]), rad[v] * np.sin(az[v]), hgt[v]])
        R = sc.look_at(c, np.array([0.0, 0.1, 1.0]))
        cam = dict(fx=focal * rad[v] / 4.0 + 37 * v, fy=focal * rad[v] / 4.0 - 11 * v, cx=w / 2 + 13.0 * v, cy=h / 2 - 7.0 * v, R=R, t=c.reshape(3, 1))
        cams.append(cam)
        cam_rows.append(np.concatenate([[cam["fx"], cam["fy"], cam["cx"], cam["cy"]], R.reshape(-1), c]))
    # the four random inputs: numpy's own streams, as float32
    rotation_deg = (rs.rand(B) * 360).astype(np.float32)                                              # amass :318
    translation = np.concatenate([rs.rand(B, 1) * (ROOM[1] - ROOM[0]) + ROOM[0], rs.rand(B, 1) * (ROOM[3] - ROOM[2]) + ROOM[2],
                                  np.zeros((B, 1))], axis=1).astype(np.float32)                      # amass :339
    noise = rs.normal(0, 1, (B, V, J, 2)).astype(np.float32)                                          # :593
    missing_u = rs.uniform(0, 1, (B, V, J)).astype(np.float32)                                        # :736
    conf_in = None if tag == "h36m" else detrng.uniform(31, "conf." + tag, (B, V, J), 0.5, 1.0)       # the mmpose confidences
    assert np.abs(missing_u.astype(np.float64) - MISSING_LEVEL).min() > 1e-6

    # pose placement, multiview_amass_h36m_mpl.py:317-342
    placed = np.zeros((B, J, 3))
    for b in range(B):
        pose_3d = poses3d[b].astype(np.float64)
        pose_3d = amass.rotate_pose(pose_3d[None], np.array([rotation_deg[b]], np.float64), axis="z")[0]     # :320
        placed[b] = pose_3d + translation[b].astype(np.float64)[None]                                 # :342
    # projection, calib.py:42-77
    clean, depth = np.zeros((B, V, J, 2)), np.zeros((B, V, J))
    for v, cam in enumerate(cams):
        K = np.array([[cam["fx"], 0, cam["cx"]], [0, cam["fy"], cam["cy"]], [0, 0, 1.0]])
        pc = calib.world_to_cam(placed, cam["R"], -cam["R"] @ cam["t"])
        clean[:, v], depth[:, v] = calib.cam_to_image(pc, K), pc[..., 2]
    assert depth.min() > 0.5
    # project_points takes float32 points: the same projection of the rounded placed poses
    points = placed.astype(np.float32)
    points_px, points_depth = np.zeros((B, V, J, 2)), np.zeros((B, V, J))
    for v, cam in enumerate(cams):
        K = np.array([[cam["fx"], 0, cam["cx"]], [0, cam["fy"], cam["cy"]], [0, 0, 1.0]])
        pc = calib.world_to_cam(points.astype(np.float64), cam["R"], -cam["R"] @ cam["t"])
        points_px[:, v], points_depth[:, v] = calib.cam_to_image(pc, K), pc[..., 2]
    base = dict(poses3d=poses3d, cams=np.stack(cam_rows), wh=np.array([w, h], np.float32), normalize=np.array([norm_in, norm_cam]),
                rotation_deg=rotation_deg, translation=translation, noise=noise, missing_u=missing_u,
                target_scale=T_SCALE, target_offset=T_OFFSET, pixels_clean=clean.astype(np.float32),
                target=((placed - T_OFFSET) / T_SCALE).astype(np.float32), points=points, points_pixels=points_px.astype(np.float32),
                points_depth=points_depth.astype(np.float32))
    if conf_in is not None:
        base["conf_in"] = conf_in
    centers = np.zeros((V, B, 1, 3), np.float32)

    for clip in (True, False):
        mode = "clip" if clip else "zero"
        for pen, (pa, pb) in PEN.items():
            poses, rays, pixels = np.zeros((V, B, J, 3), np.float32), np.zeros((V, B, J, 3), np.float32), np.zeros((B, V, J, 2), np.float32)
            sides, n_missing = np.zeros(4, int), 0
            for v, cam in enumerate(cams):
                camera = dict(cam)
                if norm_in and norm_cam:                                                      # :615-623
                    cc = DS.normalize_screen_coordinates(fake, np.array([camera["cx"], camera["cy"]]), w, h)
                    camera["cx"], camera["cy"] = cc[0], cc[1]
                    fl = np.array([camera["fx"], camera["fy"]]) / w * 2
                    camera["fx"], camera["fy"] = fl[0], fl[1]
                for b in range(B):
                    joints = clean[b, v].copy()
                    joints_vis = np.repeat((np.ones(J) if conf_in is None else conf_in[b, v].astype(np.float64))[:, None], 3, axis=1)
                    # noise and penalty, :592-613
                    nz = noise[b, v].astype(np.float64) * NOISE_LEVEL                          # :593
                    joints = joints + nz                                                       # :595
                    if pen == "exp_error":
                        penalize_conf = pa * np.exp(-pb * np.sqrt((nz ** 2).sum(axis=1)))      # :601-602
                    elif pen == "linear":
                        penalize_conf = pa * np.sqrt((nz ** 2).sum(axis=1)) + pb               # :606-607
                    elif pen == "exp_sqrt":
                        penalize_conf = np.exp(-np.sqrt((nz ** 2).sum(axis=1)) / 2)            # :609
                    else:
                        penalize_conf = np.ones((J,))                                          # :611
                    joints_vis = joints_vis * penalize_conf[:, None]                           # :613
                    for e in (0, w - 1, w):
                        assert np.abs(joints[:, 0] - e).min() > 1e-3
                    for e in (0, h - 1, h):
                        assert np.abs(joints[:, 1] - e).min() > 1e-3
                    sides += [(joints[:, 0] < 0).sum(), (joints[:, 0] > w - 1).sum(), (joints[:, 1] < 0).sum(), (joints[:, 1] > h - 1).sum()]
                    # visibility under NO_AUGMENTATION, :701-727
                    if clip:
                        joints_vis[:, 0] = np.where(0 < joints[:, 0], joints_vis[:, 0], 0)     # :710-713
                        joints_vis[:, 0] = np.where(joints[:, 0] < w - 1, joints_vis[:, 0], 0)
                        joints_vis[:, 0] = np.where(0 < joints[:, 1], joints_vis[:, 0], 0)
                        joints_vis[:, 0] = np.where(joints[:, 1] < h - 1, joints_vis[:, 0], 0)
                        joints[:, 0] = np.clip(joints[:, 0], 0, w - 1)                         # :714-715
                        joints[:, 1] = np.clip(joints[:, 1], 0, h - 1)
                    else:
                        for i in range(J):                                                     # :717-727
                            if joints_vis[i, 0] > 0.0:
                                if np.min(joints[i, :2]) < 0 or joints[i, 0] >= w or joints[i, 1] >= h:
                                    joints_vis[i, :] = 0
                                    joints[i, :] = 0
                            else:
                                joints[i, :] = 0
                    # missing joints, :735-740
                    mask = np.ones_like(joints_vis)
                    mask[missing_u[b, v].astype(np.float64) < MISSING_LEVEL] = 0
                    n_missing += int((mask[:, 0] == 0).sum())
                    joints_vis = joints_vis * mask
                    joints = joints * mask[:, 0:1]
                    pixels[b, v] = joints.astype(np.float32)
                    # normalisation and rays, :762-774
                    if norm_in:
                        joints = DS.normalize_screen_coordinates(fake, joints, w, h)           # :763
                    joints_ds = joints / fake.downsample                                       # :767
                    ray = DS.create_3d_ray_coords(fake, camera, None, joints_ds=joints_ds)     # :768
                    poses[v, b] = np.concatenate([joints, joints_vis[:, 0:1]], axis=1).astype(np.float32)   # :772-774
                    rays[v, b] = ray.numpy()
                    centers[v, b, 0] = cam["t"].reshape(-1).astype(np.float32)                 # :646
            cf = poses[..., 2]
            assert (sides > 0).all() and n_missing > 0 and (cf > 0).any(), (tag, mode, pen, sides, n_missing)
            assert pen == "none" or ((cf > 0) & (cf < 1)).any()
            for name, arr in (("poses", poses), ("rays", rays), ("pixels", pixels)):
                first = base.get("%s_none_%s" % (mode, name))
                if first is None or not np.array_equal(first, arr):
                    base["%s_%s_%s" % (mode, pen, name)] = arr
            # the restatement agrees before anything is stored
            ref = sc.synthesize(poses3d, base["cams"], (w, h), rotation_deg=rotation_deg, translation=translation, noise=noise,
                                missing_u=missing_u, noise_level=NOISE_LEVEL, missing_level=MISSING_LEVEL, penalize=pen, penalize_a=pa,
                                penalize_b=pb, clip=clip, conf=conf_in, normalize_inputs=norm_in, normalize_cameras=norm_cam,
                                target_scale=T_SCALE, target_offset=T_OFFSET)
            sc.assert_matches(dict(poses=poses, rays=rays, pixels=pixels, centers=centers, target=base["target"],
                                   pixels_clean=base["pixels_clean"]), ref)
            print(tag, mode, pen, "clamped l/r/t/b", sides, "missing", n_missing, "conf>0", int((cf > 0).sum()), "conf<0", int((cf < 0).sum()))
    base["centers"] = centers
    base["levels"] = np.array([NOISE_LEVEL, MISSING_LEVEL])
    for pen, (pa, pb) in PEN.items():
        base["ab_" + pen] = np.array([pa, pb])
    out.update({tag + "_" + k: v for k, v in base.items()})

path = os.path.join(HERE, "synth.npz")
np.savez_compressed(path, **out)
print("%s: %d bytes, %d arrays" % (path, os.path.getsize(path), len(out)))
