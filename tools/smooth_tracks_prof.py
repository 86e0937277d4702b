"""Device time per call of smooth_tracks_kernel (csrc/smooth_tracks.hip), what the split of the time axis buys, and the closed loop
on the device.

    python tools/smooth_tracks_prof.py [OUT.txt]        (default: profiles/smooth_tracks.txt of this repository)

Sizes: (S, T) = (1, 4096), (64, 1024), (256, 128) segments of T frames at J = 17; tracks of tests/smooth_tracks_cases.case (sinusoids
one unit across, noise 0.01, 5 % outlier frames, random weights); smoothness 30, order 2; plain cost and Huber at 0.05 with the default
cap of 20 solves.
Method: that of tools/refine_poses_prof.py -- every launch inside the library's own event brackets (mpl_profile_start / stop), 5
warm-up rounds, then 30 rounds in which every variant is launched once, in turn; the figure is the median of a variant's launches,
beside its minimum and maximum.
The one-lane rows need a laboratory build of the library (MPL_HIPCC_FLAGS=-DMPL_LAB python -m openmpl_amd.build; the same variable
set when this tool runs): MPL_SMOOTH_F_SINGLE_LANE sends every track to the form one lane solves.  The product library refuses the
flag, and the rows are then left out.
Closed loop: tests/smooth_loop.closed_loop on the device."""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openmpl_amd import build as mpl_build, cabi, smooth_tracks      # noqa: E402
from tests import smooth_loop, smooth_tracks_cases as sc      # noqa: E402

DEV = "cuda:0"
WARM, ROUNDS = 5, 30
SMOOTHNESS, ORDER = 30.0, 2


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


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
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "smooth_tracks.txt")
    lab = "-DMPL_LAB" in os.environ.get("MPL_HIPCC_FLAGS", "")
    lines = ["smooth_tracks_kernel: device time per call, the time axis split among 64 lanes against one lane per track",
             "library source hash %s%s" % (mpl_build.source_hash(), " (laboratory build, -DMPL_LAB)" if lab else ""),
             "device %s" % torch.cuda.get_device_name(0),
             "J = 17, sinusoid tracks one unit across, noise 0.01, 5 %% outlier frames, random weights; smoothness %g, order %d; Huber at %g, "
             "max_iterations = 20" % (SMOOTHNESS, ORDER, sc.HUBER),
             "us/launch: median of %d launches inside the library's event brackets, the variants launched in turn (min .. max)" % ROUNDS, "",
             "%5s %6s %-26s | %10s | %-24s | %s" % ("S", "T", "launch", "us/launch", "(min .. max)", "solves mean / max, status 0 / 1")]
    for S, T in ((1, 4096), (64, 1024), (256, 128)):
        c = sc.case(S * T, 17, segments=(T,) * S, weights="random", outliers=True)
        P, Wt = dev(c["points"]), dev(c["weight"])
        keep = {}

        def run(name, **kw):
            def call():
                keep[name] = smooth_tracks(P, Wt, segments=c["segments"], smoothness=SMOOTHNESS, order=ORDER, **kw)
            return name, call
        runs = [run("split plain"), run("split Huber", huber=sc.HUBER)]
        if lab:
            runs += [run("one lane plain", _single_lane=True), run("one lane Huber", huber=sc.HUBER, _single_lane=True)]
        res = alternated(runs)
        for name, _ in runs:
            med, lo, hi = res[name]
            it, st = keep[name].iterations.float(), keep[name].status
            note = "%.1f / %d, %d / %d" % (float(it.mean()), int(it.max()), int((st == 0).sum()), int((st == 1).sum()))
            lines.append("%5d %6d %-26s | %10.2f | %-24s | %s" % (S, T, name, med, "(%.2f .. %.2f)" % (lo, hi), note))
        if lab:
            for mode in ("plain", "Huber"):
                same = all(torch.equal(a, b) for a, b in zip(keep["split " + mode][:3], keep["one lane " + mode][:3]))
                far = float((keep["split " + mode].points - keep["one lane " + mode].points).abs().max())
                lines.append("%12s %s: split and one-lane points %s (max |d| %.2e)" % ("", mode, "identical" if same else "differ in rounding", far))
        lines.append("")
    r = smooth_loop.closed_loop()
    lines += ["closed loop on the device: T = 256 frames, V = 4, J = 17, 2 px of noise, H36M-like lens; synthesize_views -> "
              "triangulate_pixels(refine=True) -> smooth_tracks(smoothness=%g, order=%d)" % (smooth_loop.SMOOTHNESS, smooth_loop.ORDER),
              "mean distance to the placed poses: unsmoothed %.5f, smoothed %.5f (x %.3f); float64 chain %.5f -> %.5f"
              % (r["raw"], r["device"], r["device"] / r["raw"], r["raw64"], r["float64"])]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
