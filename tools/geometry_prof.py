"""Device time per call of the two geometry kernels (csrc/geometry.hip) beside their HBM floor.

    python tools/geometry_prof.py [OUT.txt]        (default: profiles/geometry_kernels.txt of this repository)

Sizes: V = 4 / B = 1024 / J = 17 and V = 31 / B = 256 / J = 17, without confidences and with the model's (B,J,3) pose tensors read
in place.  Method: the C ABI called back to back on one stream (pointer tables built once), 5 warm-up calls, then 5 regions of 20
calls between two events; the figure is the median region / 20, the spread is min .. max.  A region of short kernels can be
bound by the host's enqueue rate, so each kernel is also timed launch by launch by the library's own event brackets
(mpl_profile_start / stop, median of 100 launches): the smaller of the two is the better estimate of the kernel itself.
HBM floor: bytes the kernel must read plus bytes it must write, over the copy bandwidth measured in the same session (a 512-MiB
float32 tensor copied device to device, read + written bytes over the median of 5 copies; larger than the 256-MiB Infinity Cache).
A pose tensor read for its confidence channel counts with all 12 bytes per joint: every cache line of it is touched."""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openmpl_amd import build as mpl_build, cabi      # noqa: E402
from tests import geometry_cases as gc      # noqa: E402

DEV = "cuda:0"
WARM, REGIONS, CALLS = 5, 5, 20


def copy_bandwidth():
    src = torch.empty(128 << 20, dtype=torch.float32, device=DEV).normal_()
    dst = torch.empty_like(src)
    ms = []
    for i in range(2 + 5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(src)
        b.record()
        b.synchronize()
        if i >= 2:
            ms.append(a.elapsed_time(b))
    return 2 * src.numel() * 4 / (statistics.median(ms) * 1e-3)


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
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "geometry_kernels.txt")
    lib = cabi.load()
    bw = copy_bandwidth()
    lines = ["triangulate_rays_kernel / epipolar_errors_kernel: device time per call and HBM floor",
             "library source hash %s" % mpl_build.source_hash(),
             "device %s" % torch.cuda.get_device_name(0),
             "copy bandwidth of this session %.2f TB/s (512 MiB float32, device to device, read + written bytes)" % (bw / 1e12),
             "time: median of %d regions of %d calls after %d warm-up calls (min .. max) | per launch inside the library's event brackets"
             % (REGIONS, CALLS, WARM), "",
             "%-12s %3s %5s %3s %-8s | %22s | %9s | %9s | %s" % ("kernel", "V", "B", "J", "conf", "us per call (regions)", "us/launch", "floor us",
                                                                "best / floor")]
    st = torch.cuda.current_stream().cuda_stream
    for V, B, J in ((4, 1024, 17), (31, 256, 17)):
        case = gc.ring_case(B, V, J, seed=1)
        rays = [torch.from_numpy(a).to(DEV) for a in case["rays"]]
        centers = [torch.from_numpy(a).to(DEV) for a in case["centers"]]
        poses = [torch.from_numpy(np.concatenate([np.zeros((B, J, 2), np.float32), case["conf"][v][..., None]], axis=-1)).to(DEV)
                 for v in range(V)]
        tab = lambda lst: (cabi._fp * V)(*[t.data_ptr() for t in lst])      # noqa: E731
        tr, tc, tp = tab(rays), tab(centers), tab(poses)
        pts = torch.empty(B, J, 3, device=DEV)
        res = torch.empty(B, J, device=DEV)
        err = torch.empty(B, V, J, device=DEV)
        w_in = torch.rand(B, V, J, device=DEV)
        w_out = torch.empty_like(w_in)
        lines_in = V * B * J * 12 + V * B * 12
        for conf_name, conf, stride, conf_bytes in (("none", None, 1, 0), ("(B,J,3)", tp, 3, V * B * J * 12)):
            runs = (("triangulate", lines_in + conf_bytes + B * J * 16,
                     lambda: lib.mpl_triangulate_rays(tr, tc, conf, stride, B, V, J, pts.data_ptr(), res.data_ptr(), st)),
                    ("epipolar", lines_in + conf_bytes + B * V * J * 4,
                     lambda: lib.mpl_epipolar_errors(tr, tc, conf, stride, B, V, J, err.data_ptr(), None, 0.0, None, st)),
                    ("epipolar+w", lines_in + conf_bytes + B * V * J * 12,
                     lambda: lib.mpl_epipolar_errors(tr, tc, conf, stride, B, V, J, err.data_ptr(), w_in.data_ptr(), 0.02, w_out.data_ptr(), st)))
            for name, nbytes, call in runs:
                assert call() == 0
                med, lo, hi = regions(call)
                one = bracketed(call)
                floor = nbytes / bw * 1e6
                lines.append("%-12s %3d %5d %3d %-8s | %8.2f (%.2f .. %.2f) | %9.2f | %9.3f | %.0fx"
                             % (name, V, B, J, conf_name, med, lo, hi, one, floor, min(med, one) / floor))
        # the results being timed are the right ones
        x_ref, r_ref = gc.triangulate(case["rays"], case["centers"], [case["conf"][v] for v in range(V)])
        e_ref = gc.epipolar(case["rays"], case["centers"], [case["conf"][v] for v in range(V)])
        torch.cuda.synchronize()
        lines.append("   V %d: max-scaled error against float64: points %.2e residual %.2e epipolar %.2e"
                     % (V, gc.rel_errors(pts.cpu().numpy(), x_ref)[0], gc.rel_errors(res.cpu().numpy(), r_ref)[0],
                        gc.rel_errors(err.cpu().numpy(), e_ref)[0]))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
