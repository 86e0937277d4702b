"""Device time of the calls that take distortion=: without the argument, with zero coefficients and with the H36M-like set.

    python tools/distortion_prof.py [OUT.txt] [--package DIR]     (default: profiles/distortion.txt of this repository)

--package DIR imports openmpl_amd from another checkout (one built beside this one): a checkout from before the lens reports the
rows without distortion only, which is how the pinhole launches of two commits are compared on one machine in one session.
Sizes: B = 1024, V = 4, J = 17 (69 632 items) and the single frame B = 1 (68 items).  Heatmaps for the decode: 64 x 64, fp32.
Method: 5 warm-up launches per variant, then 50 rounds in which the variants take turns, each launch timed on its own inside the
library's event brackets (mpl_profile_start / stop: two events around every launch of the call, summed) and followed by a
synchronise; the figure is the median of the 50, the spread min .. max.  Variants: prepare_inputs; synthesize_views with everything
on (rotation, room, noise, penalty, clipping, missing joints, pixels returned); undistort_points; decode_heatmaps(cams=), fused
into its one launch without distortion, decode followed by prepare_inputs(distortion=) with it."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = [a for a in sys.argv[1:]]
PACKAGE = ROOT
if "--package" in ARGS:
    i = ARGS.index("--package")
    PACKAGE = os.path.abspath(ARGS[i + 1])
    del ARGS[i:i + 2]
sys.path.insert(0, PACKAGE)
import openmpl_amd                                                                      # noqa: E402
from openmpl_amd import build as mpl_build, cabi, decode_heatmaps, synthesize_views     # noqa: E402
from openmpl_amd import inputs as mpl_inputs                                            # noqa: E402

DEV = "cuda:0"
WARM, ROUNDS = 5, 50
V, J, H, W = 4, 17, 64, 64
WH = (1000.0, 1000.0)
H36M = (-0.2075, 0.2476, -0.0031, -0.00098, -0.00142)
HAS_LENS = hasattr(mpl_inputs, "undistort_points")
OWN = dict(rotate=True, room=(-0.4, 0.4, -0.3, 0.3), noise_level=6.0, penalize="exp_error", penalize_a=0.95, penalize_b=0.04,
           missing_level=0.2, return_pixels=True)


def bracketed(call, launches):
    cabi.profile_start()
    call()
    torch.cuda.synchronize()
    ms, k = cabi.profile_stop()["fuse_head"]
    assert k == launches, (k, launches)
    return ms * 1e3


def measure(runs):
    """runs: (name, launches, call) -> medians and spreads in us, the variants taking turns"""
    for _, n, call in runs:
        for _ in range(WARM):
            bracketed(call, n)
    us = [[] for _ in runs]
    for _ in range(ROUNDS):
        for k, (_, n, call) in enumerate(runs):
            us[k].append(bracketed(call, n))
    return [(statistics.median(u), min(u), max(u)) for u in us]


def cameras(n):
    """n cameras on a ring of 4.5 units looking at (0, 0, 1), f = 1145 on a 1000 px image: the layout of pack_cameras"""
    import numpy as np
    rows = []
    for v in range(n):
        a = 2 * np.pi * (v + 0.2) / n
        c = np.array([4.5 * np.cos(a), 4.5 * np.sin(a), 1.5 + 0.3 * v])
        z = np.array([0.0, 0.0, 1.0]) - c
        z /= np.linalg.norm(z)
        x = np.cross(z, [0.0, 0.0, 1.0])
        x /= np.linalg.norm(x)
        rows.append(np.concatenate([[1145.0, 1140.0, 505.0, 495.0], np.stack([x, np.cross(z, x), z]).reshape(-1), c]))
    return torch.from_numpy(np.stack(rows)).to(DEV)


def main():
    path = ARGS[0] if ARGS else os.path.join(ROOT, "profiles", "distortion.txt")
    cabi.load()
    lines = ["the calls that take distortion=: device time per call, V = %d, J = %d" % (V, J),
             "package %s, library source hash %s" % ("of this checkout" if PACKAGE == ROOT else "given with --package", mpl_build.source_hash()),
             "device %s" % torch.cuda.get_device_name(0),
             "time: median of %d calls, the variants taking turns, after %d warm-up calls each (min .. max), inside the library's event"
             % (ROUNDS, WARM), "brackets; a call of two launches is the sum of its two brackets", "",
             "%-6s %-34s %-12s | %26s | %s" % ("B", "call", "distortion", "us per call", "vs none")]
    cams = cameras(V)
    lens = [("none", None)]
    if HAS_LENS:
        lens += [("zeros", torch.zeros((V, 5), dtype=torch.float64, device=DEV)),
                 ("H36M-like", torch.tensor([H36M] * V, dtype=torch.float64, device=DEV))]
    kw = lambda d: {} if d is None else dict(distortion=d)
    for B in (1024, 1):
        g = torch.Generator(device=DEV)
        g.manual_seed(1)
        u = lambda *s: torch.rand(s, generator=g, device=DEV)
        points = u(B, J, 3) - 0.5 + torch.tensor([0.0, 0.0, 1.0], device=DEV)
        px = openmpl_amd.project_points(points, cams)[0]
        conf = 0.5 + 0.5 * u(B, V, J)
        hm = u(B, V, J, H, W)
        center = 500.0 + 20.0 * u(B, V, 2)
        scale = 4.0 + u(B, V, 2)
        groups = [("prepare_inputs", 1, 1, lambda d: (lambda: mpl_inputs.prepare_inputs(px, conf, cams, WH, **kw(d)))),
                  ("synthesize_views, everything on", 1, 1, lambda d: (lambda: synthesize_views(points, cams, WH, seed=3, **OWN, **kw(d)))),
                  ("decode_heatmaps(cams=)", 1, 2, lambda d: (lambda: decode_heatmaps(hm, center, scale, cams=cams, image_size=WH, **kw(d))))]
        if HAS_LENS:
            groups.insert(2, ("undistort_points", None, 1, lambda d: (lambda: mpl_inputs.undistort_points(px, cams, d))))
        for what, n_plain, n_lens, make in groups:
            sets = [(name, d) for name, d in lens if not (d is None and n_plain is None)]
            runs = [("%s" % name, n_plain if d is None else n_lens, make(d)) for name, d in sets]
            res = measure(runs)
            for (name, _, _), (med, lo, hi) in zip(runs, res):
                lines.append("%-6d %-34s %-12s | %9.2f (%.2f .. %.2f) | %.2f x" % (B, what, name, med, lo, hi, med / res[0][0]))
        del hm
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
