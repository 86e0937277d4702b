"""Device time of one synthesize_views / project_points call (csrc/synth.hip).

    python tools/synth_prof.py [OUT.txt]        (default: profiles/synth_kernel.txt of this repository)

Size: B = 1024, V = 4, J = 17 (69 632 work items) with everything switched on: rotation, room translation, detection noise with
the exp_error penalty, clipping, missing joints, both normalisations, target scaling, pixels returned.  Method: calls back to back
on one stream, 5 warm-up calls, then 5 regions of 20 calls between two events; the figure is the median region / 20, the spread is
min .. max.  A region of short kernels can be bound by the host's enqueue rate (a call allocates 3 V + 3 tensors), so the kernel is
also timed launch by launch by the library's own event brackets (mpl_profile_start / stop, median of 100 launches): the smaller of
the two is the better estimate of the kernel itself."""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openmpl_amd import build as mpl_build, cabi, project_points, synthesize_views      # noqa: E402
from tests import synth_cases as sc      # noqa: E402

DEV = "cuda:0"
WARM, REGIONS, CALLS = 5, 5, 20
B, V, J = 1024, 4, 17
WH = (1000.0, 1000.0)
ON = dict(seed=1, rotate=True, room=(-0.4, 0.4, -0.3, 0.3), noise_level=6.0, penalize="exp_error", penalize_a=0.95, penalize_b=0.04,
          clip=True, missing_level=0.2, target_scale=(2.0, 2.5, 1.25), target_offset=(0.1, -0.2, 1.0))


def regions(call):
    for _ in range(WARM):
        call()
    torch.cuda.synchronize()
    us = []
    for _ in range(REGIONS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(CALLS):
            call()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / CALLS)
    return statistics.median(us), min(us), max(us)


def bracketed(call, n=100):
    us = []
    for _ in range(n):
        cabi.profile_start()
        call()
        torch.cuda.synchronize()
        ms, k = cabi.profile_stop()["fuse_head"]
        assert k == 1
        us.append(ms * 1e3)
    return statistics.median(us)


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "synth_kernel.txt")
    cabi.load()
    poses3d, cams = sc.scene(B, V, J, seed=1, focal=2400.0)
    P, Cm = torch.from_numpy(poses3d).to(DEV), torch.from_numpy(cams).to(DEV)
    runs = [("synthesize_views all on", lambda: synthesize_views(P, Cm, WH, return_pixels=True, **ON)),
            ("synthesize_views all off", lambda: synthesize_views(P, Cm, WH, clip=False)),
            ("project_points", lambda: project_points(P, Cm))]
    lines = ["synthesize_views_kernel: device time per call at B = %d, V = %d, J = %d (%d work items)" % (B, V, J, B * V * J),
             "library source hash %s" % mpl_build.source_hash(),
             "device %s" % torch.cuda.get_device_name(0),
             "time: median of %d regions of %d calls after %d warm-up calls (min .. max) | per launch inside the library's event brackets"
             % (REGIONS, CALLS, WARM), "",
             "%-26s | %24s | %9s" % ("call", "us per call (regions)", "us/launch")]
    for name, call in runs:
        call()
        med, lo, hi = regions(call)
        lines.append("%-26s | %8.2f (%.2f .. %.2f) | %9.2f" % (name, med, lo, hi, bracketed(call)))
    # the results being timed are the right ones
    ref = sc.synthesize(poses3d, cams, WH, **ON)
    r = synthesize_views(P, Cm, WH, return_pixels=True, **ON)
    near = ref["margin"] < 1e-6
    got = dict(poses=np.stack([t.cpu().numpy() for t in r.poses]), rays=np.stack([t.cpu().numpy() for t in r.rays]),
               centers=np.stack([t.cpu().numpy() for t in r.centers]), target=r.target.cpu().numpy(), pixels=r.pixels.cpu().numpy(),
               pixels_clean=r.pixels_clean.cpu().numpy())
    sc.assert_matches(got, ref, skip=near)
    lines.append("   all on: equal to the float64 restatement at one float32 rounding; %d of %d items within 1e-6 px of a decision left out; "
                 "confidence 0 in %.1f %% of the items" % (int(near.sum()), near.size, 100.0 * float((ref["conf"] == 0).mean())))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
