"""Device time per call of refine_points_kernel (csrc/refine.hip) beside triangulate_robust_kernel at the same sizes, and what the
refinement buys on the device.

    python tools/refine_prof.py [OUT.txt]        (default: profiles/refine.txt of this repository)

Sizes: B = 1024, J = 17, V = 4 and V = 31, and a single frame (B = 1, V = 4); detections with 2 px of noise under the H36M-like lens
(tests/refine_cases.case), started from the float64 least-squares point.  Variants: plain / Huber (6 px) cost, the lens kernel / the
pinhole kernel (no distortion table; on the pinhole pixels of the same scene and noise), and max_iterations = 0
(reprojection_errors); beside them triangulate_rays_robust on the rays of the lens pixels, with the pair consensus (tau = 0.05
units) and without.
Method: every launch inside the library's own event brackets (mpl_profile_start / stop), 5 warm-up rounds, then 50 rounds in which
every variant is launched once, in turn -- what else the machine does in that time falls on all of them alike; the figure is the
median of a variant's 50 launches, beside its minimum and maximum.
Accuracy: mean distance to the true points before and after, on the device, at V = 3, 4, 8 (plain, 2 px of noise) and with one view
of every joint moved 40 .. 120 px off (Huber 6 px), the cases of tests/test_refine_cpu.py."""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openmpl_amd import build as mpl_build, cabi, refine_points, triangulate_rays_robust      # noqa: E402
from openmpl_amd.inputs import prepare_inputs      # noqa: E402
from tests import refine_cases as rc      # noqa: E402

DEV = "cuda:0"
WARM, ROUNDS = 5, 50
HUBER, TAU = 6.0, 0.05


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
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "refine.txt")
    lines = ["refine_points_kernel: device time per call beside triangulate_robust_kernel",
             "library source hash %s" % mpl_build.source_hash(),
             "device %s" % torch.cuda.get_device_name(0),
             "J = 17, 2 px of noise, H36M-like lens, start: the least-squares point; Huber at %.0f px; tau = %.2f" % (HUBER, TAU),
             "us/launch: median of %d launches inside the library's event brackets, the variants launched in turn (min .. max)" % ROUNDS, "",
             "%5s %3s %-37s | %9s | %-20s | %s" % ("B", "V", "launch", "us/launch", "(min .. max)", "trials mean / max, status 0 / 1")]
    for B, V, J in ((1024, 4, 17), (1024, 31, 17), (1, 4, 17)):
        c = rc.case(B, V, J, "h36m", seed=13)
        P, X, Cm, D = dev(c["points0"]), dev(c["pixels"]), dev(c["cams"]), dev(c["dist"])
        poses, rays, centers = prepare_inputs(X, None, Cm, rc.WH, False, False, distortion=D)
        c0 = rc.case(B, V, J, "zeros", seed=13)          # the same scene and noise without a lens, for the pinhole kernel
        P0, X0 = dev(c0["points0"]), dev(c0["pixels"])
        keep = {}

        def refine(name, dist, **kw):
            def call():
                keep[name] = refine_points(P if dist is not None else P0, X if dist is not None else X0, None, Cm, distortion=dist, **kw)
            return name, call
        runs = [refine("refine plain, lens", D), refine("refine Huber, lens", D, huber=HUBER),
                refine("refine plain, pinhole kernel", None), refine("refine Huber, pinhole kernel", None, huber=HUBER),
                refine("errors only (max_iterations=0), lens", D, max_iterations=0),
                ("triangulate_rays_robust, consensus", lambda: triangulate_rays_robust(rays, centers, poses, threshold=TAU)),
                ("triangulate_rays_robust, stages off", lambda: triangulate_rays_robust(rays, centers, poses))]
        res = alternated(runs)
        for name, _ in runs:
            med, lo, hi = res[name]
            note = ""
            if name in keep:
                it, st = keep[name].iterations.float(), keep[name].status
                note = "%.1f / %d, %d / %d" % (float(it.mean()), int(it.max()), int((st == 0).sum()), int((st == 1).sum()))
            lines.append("%5d %3d %-37s | %9.2f | %-20s | %s" % (B, V, name, med, "(%.2f .. %.2f)" % (lo, hi), note))
        lines.append("")
    lines += ["accuracy on the device, B = 64, J = 17, H36M-like lens, mean distance to the true points (scene units)",
              "%3s %-50s | %9s | %9s | %s" % ("V", "case", "before", "after", "after / before")]
    for V, outliers, huber in ((3, 0, None), (4, 0, None), (8, 0, None), (4, 1, HUBER), (8, 1, HUBER)):
        c = rc.case(64, V, 17, "h36m", seed=13, outliers=outliers)
        r = refine_points(dev(c["points0"]), dev(c["pixels"]), None, dev(c["cams"]), distortion=dev(c["dist"]), huber=huber)
        e0, e1 = rc.mean_error(c["points0"], c["truth"])[0], rc.mean_error(r.points.cpu().numpy(), c["truth"])[0]
        what = "2 px noise, plain" if not outliers else "one view per joint 40 .. 120 px off, Huber %.0f px" % HUBER
        lines.append("%3d %-50s | %9.5f | %9.5f | %.3f" % (V, what, e0, e1, e1 / e0))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
