"""Device time per call of refine_cameras_kernel (csrc/refine_cameras.hip) and of one bundle_adjust, and what the alternation buys on
the device.

    python tools/refine_cameras_prof.py [OUT.txt]        (default: profiles/refine_cameras.txt of this repository)

Sizes: B = 1024, J = 17, V = 4 and V = 31 -- 17408 observations per view, one workgroup per view; the true points, detections with
2 px of noise under the H36M-like lens, every camera turned by 2 degrees and moved by 0.05 units
(tests/refine_cameras_cases.case).  Variants: plain / Huber (6 px) cost, the lens kernel / the pinhole kernel (no distortion table; on
the pinhole pixels of the same scene and noise), and max_iterations = 0 (one evaluation: the score of a rig).
Method: every launch inside the library's own event brackets (mpl_profile_start / stop), 5 warm-up rounds, then 50 rounds in which
every variant is launched once, in turn -- what else the machine does in that time falls on all of them alike; the figure is the
median of a variant's 50 launches, beside its minimum and maximum.  A run's time is its trial count times the time of one evaluation
and step, so the trial counts stand beside it.
bundle_adjust(rounds=8): the closed loop of tests/test_refine_cameras_gpu.py -- (64,4,17), cameras 2 and 3 turned by 2 degrees and
moved by 0.05 units, cameras 0 and 1 fixed, from triangulate_pixels under the perturbed rig --, the device time of its 17 launches
summed, median of 20 calls, and the mean distance to the true points before and after beside the float64 restatement's."""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openmpl_amd import build as mpl_build, bundle_adjust, cabi, refine_cameras, triangulate_pixels      # noqa: E402
from tests import refine_cameras_cases as cc      # noqa: E402
from tests import refine_cases as rc      # noqa: E402

DEV = "cuda:0"
WARM, ROUNDS = 5, 50
HUBER = 6.0


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def one(call, launches=1):
    cabi.profile_start()
    call()
    torch.cuda.synchronize()
    ms, k = cabi.profile_stop()["fuse_head"]
    assert k == launches, k
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
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "refine_cameras.txt")
    lines = ["refine_cameras_kernel: device time per call; one workgroup of 512 threads per view",
             "library source hash %s" % mpl_build.source_hash(),
             "device %s" % torch.cuda.get_device_name(0),
             "J = 17, the true points, 2 px of noise, H36M-like lens, every camera 2 degrees / 0.05 units off; Huber at %.0f px" % HUBER,
             "us/launch: median of %d launches inside the library's event brackets, the variants launched in turn (min .. max)" % ROUNDS, "",
             "%5s %3s %-37s | %9s | %-22s | %s" % ("B", "V", "launch", "us/launch", "(min .. max)", "trials mean / max, status 0 / 1")]
    for B, V, J in ((1024, 4, 17), (1024, 31, 17)):
        c = cc.case(B, V, J, "h36m")
        c0 = cc.case(B, V, J, "zeros")                   # the same scene, noise and perturbation without a lens, for the pinhole kernel
        P, X, X0, Cm, D = dev(c["points"]), dev(c["pixels"]), dev(c0["pixels"]), dev(c["cams0"]), dev(c["dist"])
        keep = {}

        def refine(name, dist, **kw):
            def call():
                keep[name] = refine_cameras(P, X if dist is not None else X0, None, Cm, distortion=dist, **kw)
            return name, call
        runs = [refine("cameras plain, lens", D), refine("cameras Huber, lens", D, huber=HUBER),
                refine("cameras plain, pinhole kernel", None), refine("cameras Huber, pinhole kernel", None, huber=HUBER),
                refine("score only (max_iterations=0), lens", D, max_iterations=0),
                refine("score only, pinhole kernel", None, max_iterations=0)]
        res = alternated(runs)
        for name, _ in runs:
            med, lo, hi = res[name]
            it, st = keep[name].iterations.float(), keep[name].status
            note = "%.1f / %d, %d / %d" % (float(it.mean()), int(it.max()), int((st == 0).sum()), int((st == 1).sum()))
            lines.append("%5d %3d %-37s | %9.2f | %-22s | %s" % (B, V, name, med, "(%.2f .. %.2f)" % (lo, hi), note))
        lines.append("")

    c, cams0 = cc.closed_loop_case()
    X, Cm, D = dev(c["pixels"]), dev(cams0), dev(c["dist"])
    lin, _, _ = triangulate_pixels(X, None, Cm, rc.WH, distortion=D)
    keep = {}

    def ba():
        keep["r"] = bundle_adjust(lin, X, None, Cm, D, rounds=8, fixed=(0, 1))
    for _ in range(WARM):
        ba()
    us = [one(ba, 17) for _ in range(20)]
    r = keep["r"]
    lin64 = rc.linear_points(c["pixels"], None, cams0, c["dist"]).astype(np.float32)
    ref = cc.bundle_adjust(lin64, c["pixels"], None, cams0, c["dist"], None, 8, (0, 1))
    e0, e1 = rc.mean_error(lin.cpu().numpy(), c["truth"])[0], rc.mean_error(r.points.cpu().numpy(), c["truth"])[0]
    e_true = rc.mean_error(rc.linear_points(c["pixels"], None, c["cams"], c["dist"]), c["truth"])[0]
    cost, n = r.cost.cpu().numpy(), c["pixels"][..., 0].size
    off0 = np.linalg.norm(cams0[2:, 13:] - c["cams"][2:, 13:], axis=1)
    off1 = np.linalg.norm(r.cams.cpu().numpy()[2:, 13:] - c["cams"][2:, 13:], axis=1)
    lines += ["bundle_adjust(rounds=8, fixed=(0, 1)) at B = 64, V = 4, J = 17: cameras 2 and 3 turned by 2 degrees and moved by 0.05 units",
              "device time of the 17 launches, summed: median of 20 calls %.1f us (%.1f .. %.1f)" % (statistics.median(us), min(us), max(us)),
              "trials of the last round: cameras %s, points mean %.1f" % (r.cameras.iterations.cpu().numpy(), float(r.refined.iterations.float().mean())),
              "RMS reprojection error per round (px): %s" % " ".join("%.2f" % v for v in np.sqrt(cost / n)),
              "mean distance to the true points (scene units): %.5f -> %.5f (x %.3f); float64 restatement %.5f -> %.5f; least squares under "
              "the true rig %.5f" % (e0, e1, e1 / e0, rc.mean_error(lin64, c["truth"])[0], rc.mean_error(ref["points"], c["truth"])[0], e_true),
              "centres of cameras 2 and 3 off by %s -> %s units" % (np.round(off0, 4), np.round(off1, 4))]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
