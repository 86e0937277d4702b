"""Device time per call of refine_poses_kernel (csrc/refine_poses.hip) beside refine_points_kernel at the same sizes, and what the
bones buy on the device.

    python tools/refine_poses_prof.py [OUT.txt]        (default: profiles/refine_poses.txt of this repository)

Sizes: B = 1024, J = 17 (the human tree), V = 2, 4 and 31; detections with 2 px of noise under the H36M-like lens
(tests/refine_poses_cases.case), started from the float64 least-squares point, the bone lengths those of every true pose, the
default bone_weight.  Variants: plain / Huber (2.5 px) cost, both refiners at max_iterations = 50 so that the caps compare.
Method: that of tools/refine_prof.py -- every launch inside the library's own event brackets (mpl_profile_start / stop), 5 warm-up
rounds, then 30 rounds in which every variant is launched once, in turn; the figure is the median of a variant's launches, beside
its minimum and maximum.
Accuracy: the closed loops of tests/test_refine_poses_gpu.py on the device -- mean distance to the true points after refine_points
and after refine_poses at V = 2, 3, 4, 8 (B = 32), with the bone lengths 2 % off at V = 2, and the occlusion case (V = 4, 30 % of
the joints seen by one view, the start 0.05 units off the truth)."""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openmpl_amd import build as mpl_build, cabi, refine_points, refine_poses      # noqa: E402
from tests import refine_poses_cases as pc      # noqa: E402

DEV = "cuda:0"
WARM, ROUNDS = 5, 30
HUBER, CAP = 2.5, 50


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def one(call):
    cabi.profile_start()
    call()
    torch.cuda.synchronize()
    ms, k = cabi.profile_stop()["fuse_head"]
    assert k == 1
    return ms * 1e3


def alternated(runs):
    """-> {name: (median, min, max) us} over ROUNDS rounds of one launch each, in turn"""
    for _ in range(WARM):
        for _, call in runs:
            call()
    torch.cuda.synchronize()
    us = {name: [] for name, _ in runs}
    for _ in range(ROUNDS):
        for name, call in runs:
            us[name].append(one(call))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in us.items()}


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "refine_poses.txt")
    lines = ["refine_poses_kernel: device time per call beside refine_points_kernel",
             "library source hash %s" % mpl_build.source_hash(),
             "device %s" % torch.cuda.get_device_name(0),
             "J = 17 (human tree), 2 px of noise, H36M-like lens, start: the least-squares point; true bone lengths per pose, bone_weight "
             "1e4; Huber at %.1f px; max_iterations = %d" % (HUBER, CAP),
             "us/launch: median of %d launches inside the library's event brackets, the variants launched in turn (min .. max)" % ROUNDS, "",
             "%5s %3s %-22s | %9s | %-22s | %s" % ("B", "V", "launch", "us/launch", "(min .. max)", "trials mean / max, status 0 / 1")]
    for B, V, J in ((1024, 2, 17), (1024, 4, 17), (1024, 31, 17)):
        c = pc.case(B, V, J)
        P, X, Cm, D, L = dev(c["points0"]), dev(c["pixels"]), dev(c["cams"]), dev(c["dist"]), dev(c["limb"])
        keep = {}

        def run(name, fn, *extra, **kw):
            def call():
                keep[name] = fn(P, X, None, Cm, *extra, distortion=D, max_iterations=CAP, **kw)
            return name, call
        runs = [run("refine_poses plain", refine_poses, L), run("refine_poses Huber", refine_poses, L, huber=HUBER),
                run("refine_points plain", refine_points), run("refine_points Huber", refine_points, huber=HUBER)]
        res = alternated(runs)
        for name, _ in runs:
            med, lo, hi = res[name]
            it, st = keep[name].iterations.float(), keep[name].status
            note = "%.1f / %d, %d / %d" % (float(it.mean()), int(it.max()), int((st == 0).sum()), int((st == 1).sum()))
            lines.append("%5d %3d %-22s | %9.2f | %-22s | %s" % (B, V, name, med, "(%.2f .. %.2f)" % (lo, hi), note))
        lines.append("")
    lines += ["accuracy on the device, B = 32, J = 17, H36M-like lens, 2 px of noise, mean distance to the true points (scene units)",
              "%3s %-28s | %13s | %12s | %s" % ("V", "bone lengths", "refine_points", "refine_poses", "ratio")]
    for V, off in ((2, 0.0), (2, 0.02), (3, 0.0), (4, 0.0), (8, 0.0)):
        c = pc.case(32, V, 17, limb_error=off)
        args = (dev(c["points0"]), dev(c["pixels"]), None, dev(c["cams"]))
        a = refine_points(*args, distortion=dev(c["dist"])).points.cpu().numpy()
        b = refine_poses(*args, dev(c["limb"]), distortion=dev(c["dist"]), max_iterations=100)
        ea, eb = pc.joint_errors(a, c["truth"]).mean(), pc.joint_errors(b.points.cpu().numpy(), c["truth"]).mean()
        lines.append("%3d %-28s | %13.5f | %12.5f | %.3f   (trials up to %d, status 0: %d of 32)"
                     % (V, "true" if not off else "%.0f %% off" % (100 * off), ea, eb, eb / ea, int(b.iterations.max()), int((b.status == 0).sum())))
    c, one_view = pc.occlusion_case()
    r = refine_poses(dev(c["points0"]), dev(c["pixels"]), dev(c["conf"]), dev(c["cams"]), dev(c["limb"]), distortion=dev(c["dist"]),
                     max_iterations=100)
    e0, e1 = pc.joint_errors(c["points0"], c["truth"]), pc.joint_errors(r.points.cpu().numpy(), c["truth"])
    leaf = ~np.isin(np.arange(17), c["parents"])[None, :] & np.ones_like(one_view)
    lines += ["", "occlusion, V = 4, B = 32: %d of %d joints seen by one view, start 0.05 units off the truth" % (one_view.sum(), one_view.size),
              "one-view joints: %.5f -> %.5f (x %.3f); inner %.5f, leaves %.5f; fully seen joints: %.5f -> %.5f"
              % (e0[one_view].mean(), e1[one_view].mean(), e1[one_view].mean() / e0[one_view].mean(), e1[one_view & ~leaf].mean(),
                 e1[one_view & leaf].mean(), e0[~one_view].mean(), e1[~one_view].mean()),
              "trials up to %d, status 0 / 1: %d / %d, cost <= cost0 everywhere: %s"
              % (int(r.iterations.max()), int((r.status == 0).sum()), int((r.status == 1).sum()), bool((r.cost <= r.cost0).all()))]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
