"""Device time of openmpl_amd.relative_pose (csrc/relative_pose.hip) at one size.

    python tools/relative_pose_prof.py B [H]        (V = 4, J = 17, pairs (0,1) and (2,3), the H36M-like lens; H defaults to 1024)

Prints the median time of the call, by one device event pair around it (which includes the gaps between its three launches), and
of its three launches, by the library's own event brackets, over 20 runs after 3 warm-up runs.  Under a kernel trace
(rocprofv3 --kernel-trace --stats -- python tools/relative_pose_prof.py B) the trace's statistics give the time of each kernel
without the events; profiles/relative_pose.txt holds both.  The case is tests/relative_pose_cases.case: 2 px of noise and a quarter
of the detections of every view planted 40 to 120 px off."""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import openmpl_amd      # noqa: E402
from openmpl_amd import build as mpl_build, cabi      # noqa: E402
from tests import relative_pose_cases as rp      # noqa: E402

RUNS, WARM = 20, 3
PAIRS = ((0, 1), (2, 3))


def main():
    B = int(sys.argv[1])
    H = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    c = rp.case(B, 4, 17, pairs=PAIRS, outliers=0.25)
    X, Cm, D = (torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ("pixels", "cams", "dist"))
    run = lambda: openmpl_amd.relative_pose(X, None, Cm, PAIRS, D, hypotheses=H)      # noqa: E731
    call, launches = [], []
    for i in range(WARM + RUNS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = run()
        b.record()
        b.synchronize()
        cabi.profile_start()
        run()
        torch.cuda.synchronize()
        ms, n = cabi.profile_stop()["fuse_head"]
        if i >= WARM:
            call.append(a.elapsed_time(b) * 1e3)
            launches.append(ms * 1e3)
    R, t = r.rotation.cpu().numpy(), r.direction.cpu().numpy()
    deg = [rp.pose_errors(R[p], t[p], c["truth_cams"], pair) for p, pair in enumerate(PAIRS)]
    print("relative_pose (B, V, J, H) = (%d, 4, 17, %d), pairs %s, on %s, library source hash %s"
          % (B, H, PAIRS, torch.cuda.get_device_name(0), mpl_build.source_hash()))
    print("median of %d runs after %d: the call %.1f us (one event pair), its %d launches %.1f us (the library's brackets, summed)"
          % (RUNS, WARM, statistics.median(call), n, statistics.median(launches)))
    print("status %s, inliers %s of %d, winners off by %s degrees (rotation, direction)" % (r.status.tolist(), r.count.tolist(), B * 17,
                                                                                          np.round(deg, 2).tolist()))


if __name__ == "__main__":
    main()
