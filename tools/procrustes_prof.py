"""Device time of one procrustes_align and of PoseEvaluator.update() with and without aligned=... (csrc/procrustes.hip).

    python tools/procrustes_prof.py [OUT.txt]        (default: profiles/procrustes_kernel.txt of this repository)

Sizes: B = 1024 / J = 17 and B = 256 / J = 64.  Method: calls back to back on one stream, 5 warm-up calls, then 5 regions of 20
calls between two events; the figure is the median region / 20, the spread is min .. max.  A region of short kernels can be bound
by the host's enqueue rate, so the alignment kernel is also timed launch by launch by the library's own event brackets
(mpl_profile_start / stop, median of 100 launches): the smaller of the two is the better estimate of the kernel itself."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openmpl_amd import PoseEvaluator, build as mpl_build, cabi, procrustes_align      # noqa: E402
from tests import procrustes_cases as pc      # noqa: E402

DEV = "cuda:0"
WARM, REGIONS, CALLS = 5, 5, 20


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
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "procrustes_kernel.txt")
    cabi.load()
    lines = ["procrustes_align_kernel and PoseEvaluator.update(): device time per call",
             "library source hash %s" % mpl_build.source_hash(),
             "device %s" % torch.cuda.get_device_name(0),
             "time: median of %d regions of %d calls after %d warm-up calls (min .. max) | per launch inside the library's event brackets"
             % (REGIONS, CALLS, WARM), "",
             "%-28s %5s %3s | %24s | %9s" % ("call", "B", "J", "us per call (regions)", "us/launch")]
    for B, J in ((1024, 17), (256, 64)):
        case = pc.similarity_case(B, J, seed=1)
        pred, tgt = torch.from_numpy(case["pred"]).to(DEV), torch.from_numpy(case["target"]).to(DEV)
        conf = torch.ones(B, J, device=DEV)
        runs = [("procrustes_align", lambda: procrustes_align(pred, tgt), True),
                ("procrustes_align conf+scale", lambda: procrustes_align(pred, tgt, conf=conf, scale=(2.0, 3.0, 0.5), offset=0.1), True)]
        for name, aligned in (("update()", None), ("update(aligned=similarity)", "similarity"), ("update(aligned=rigid)", "rigid")):
            ev = PoseEvaluator(J, aligned=aligned)
            runs.append((name, lambda ev=ev: ev.update(pred, tgt, conf_3d=conf), False))
            runs.append((name + " scaled", lambda ev=ev: ev.update(pred, tgt, conf_3d=conf, scale=(2.0, 3.0, 0.5), offset=0.1), False))
        for name, call, single in runs:
            call()
            med, lo, hi = regions(call)
            one = "%9.2f" % bracketed(call) if single else "%9s" % "-"
            lines.append("%-28s %5d %3d | %8.2f (%.2f .. %.2f) | %s" % (name, B, J, med, lo, hi, one))
        # the results being timed are the right ones
        ref = pc.align(case["pred"], case["target"])
        res = procrustes_align(pred, tgt)
        lines.append("   B %d J %d: max-scaled error against float64: aligned %.2e d %.2e rotation %.2e"
                     % (B, J, pc.rel_errors(res.aligned.cpu().numpy(), ref["aligned"])[0], pc.rel_errors(res.d.cpu().numpy(), ref["d"])[0],
                        pc.rel_errors(res.rotation.cpu().numpy(), ref["rotation"])[0]))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
