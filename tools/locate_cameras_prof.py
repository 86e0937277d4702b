"""Device time of openmpl_amd.locate_cameras (csrc/locate_cameras.hip) at one size.

    python tools/locate_cameras_prof.py B [H]        (V = 4, J = 17, the H36M-like lens; H defaults to 1024)

Prints the median time of the call, by one device event pair around it (which includes the gaps between its three launches), and
of its three launches, by the library's own event brackets, over 20 runs after 3 warm-up runs.  Under a kernel trace
(rocprofv3 --kernel-trace --stats -- python tools/locate_cameras_prof.py B) the trace's statistics give the time of each kernel
without the events; profiles/locate_cameras.txt holds both.  The case is tests/locate_cameras_cases.case: 2 px of noise and a quarter
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
from tests import locate_cameras_cases as lc      # noqa: E402

RUNS, WARM = 20, 3


def main():
    B = int(sys.argv[1])
    H = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    c = lc.case(B, 4, 17, outliers=0.25)
    P, X, Cm, D = (torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ("points", "pixels", "cams", "dist"))
    run = lambda: openmpl_amd.locate_cameras(P, X, None, Cm, D, hypotheses=H)      # noqa: E731
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
    deg, off = lc.pose_errors(r.cams.cpu().numpy(), c["truth_cams"])
    print("locate_cameras (B, V, J, H) = (%d, 4, 17, %d) on %s, library source hash %s" % (B, H, torch.cuda.get_device_name(0),
                                                                                           mpl_build.source_hash()))
    print("median of %d runs after %d: the call %.1f us (one event pair), its %d launches %.1f us (the library's brackets, summed)"
          % (RUNS, WARM, statistics.median(call), n, statistics.median(launches)))
    print("status %s, inliers %s of %d, winners off by %s degrees and %s units" % (r.status.tolist(), r.count.tolist(), B * 17,
                                                                                   np.round(deg, 2), np.round(off, 3)))


if __name__ == "__main__":
    main()
