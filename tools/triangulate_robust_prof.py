"""Device time per call of triangulate_robust_kernel (csrc/geometry.hip) beside the two other geometry kernels at the same size, and
the accuracy of the robust triangulation against plain least squares on cases with outliers.

    python tools/triangulate_robust_prof.py [OUT.txt]        (default: profiles/triangulate_robust.txt of this repository)

Sizes: B = 1024, J = 17, V = 4 and V = 31; both stages on (tau = 0.08 m, conf_threshold = 0.85), the confidences read in place from
the model's (B,J,3) pose tensors; V / 4 views of every item look 0.4 .. 1.0 m past their point (tests/robust_tri_cases.outlier_case).
Method: that of tools/geometry_prof.py -- the C ABI called back to back on one stream, each launch timed by the library's own
event brackets (mpl_profile_start / stop), median of 50 launches after 5 warm-up calls; beside it the median of 5 regions of 20
calls between two events, which for a short kernel is bound by the host's enqueue rate.
Accuracy: mean distance of the triangulated points to the true ones, over the joints the robust call keeps, at three small shapes
and at larger batches of the same rigs."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import geometry_prof as gp      # noqa: E402
from openmpl_amd import build as mpl_build, cabi, triangulate_rays, triangulate_rays_robust      # noqa: E402
from tests import robust_tri_cases as rc      # noqa: E402

DEV = "cuda:0"
TAU, CONF_TH = 0.08, 0.85


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "triangulate_robust.txt")
    lib = cabi.load()
    lines = ["triangulate_robust_kernel: device time per call beside triangulate_rays_kernel and epipolar_errors_kernel",
             "library source hash %s" % mpl_build.source_hash(),
             "device %s" % torch.cuda.get_device_name(0),
             "B = 1024, J = 17, confidences in (B,J,3) pose tensors, V / 4 outlier views per item, tau = %.2f, conf_threshold = %.2f"
             % (TAU, CONF_TH),
             "us/launch: median of 50 launches inside the library's event brackets | regions: median of %d regions of %d calls (min .. max)"
             % (gp.REGIONS, gp.CALLS), "",
             "%-22s %3s | %9s | %s" % ("kernel", "V", "us/launch", "us per call (regions)")]
    st = torch.cuda.current_stream().cuda_stream
    B, J = 1024, 17
    for V in (4, 31):
        case = rc.outlier_case(B, V, J, n_out=V // 4, seed=1, configs=())
        rays = [torch.from_numpy(a).to(DEV) for a in case["rays"]]
        centers = [torch.from_numpy(a).to(DEV) for a in case["centers"]]
        poses = [torch.from_numpy(np.concatenate([np.zeros((B, J, 2), np.float32), case["conf"][v][..., None]], axis=-1)).to(DEV)
                 for v in range(V)]
        tab = lambda lst: (cabi._fp * V)(*[t.data_ptr() for t in lst])      # noqa: E731
        tr, tc, tp = tab(rays), tab(centers), tab(poses)
        pts = torch.empty(B, J, 3, device=DEV)
        res = torch.empty(B, J, device=DEV)
        err = torch.empty(B, V, J, device=DEV)
        inl = torch.empty(B, V, J, device=DEV)
        runs = (("robust, both stages", lambda: lib.mpl_triangulate_robust(tr, tc, tp, 3, B, V, J, TAU, CONF_TH, 2, pts.data_ptr(),
                                                                           res.data_ptr(), inl.data_ptr(), st)),
                ("robust, consensus", lambda: lib.mpl_triangulate_robust(tr, tc, tp, 3, B, V, J, TAU, -1.0, 2, pts.data_ptr(),
                                                                         res.data_ptr(), inl.data_ptr(), st)),
                ("robust, both off", lambda: lib.mpl_triangulate_robust(tr, tc, tp, 3, B, V, J, -1.0, -1.0, 2, pts.data_ptr(),
                                                                        res.data_ptr(), inl.data_ptr(), st)),
                ("triangulate_rays", lambda: lib.mpl_triangulate_rays(tr, tc, tp, 3, B, V, J, pts.data_ptr(), res.data_ptr(), st)),
                ("epipolar_errors", lambda: lib.mpl_epipolar_errors(tr, tc, tp, 3, B, V, J, err.data_ptr(), None, 0.0, None, st)))
        for name, call in runs:
            assert call() == 0
            med, lo, hi = gp.regions(call)
            one = gp.bracketed(call, n=50)
            lines.append("%-22s %3d | %9.2f | %8.2f (%.2f .. %.2f)" % (name, V, one, med, lo, hi))
            if name == "robust, both stages":
                lines[-1] += "   inliers per item %.2f of %d" % (float(inl.sum(dim=1).mean()), V)
    lines += ["", "accuracy: 0.02 m of noise, V / 4 views of every item displaced by 0.4 .. 1.0 m, tau = %.2f m, no confidences" % TAU,
              "%3s %3s %3s | %24s | %24s | %s" % ("B", "V", "J", "least squares, mean (m)", "robust, mean error (m)", "joints kept")]
    for B, V, J in ((3, 4, 17), (2, 8, 5), (1, 31, 3), (256, 4, 17), (256, 8, 5), (64, 31, 3)):
        case = rc.outlier_case(B, V, J, n_out=V // 4, seed=1, configs=())
        rays = [torch.from_numpy(a).to(DEV) for a in case["rays"]]
        centers = [torch.from_numpy(a).to(DEV) for a in case["centers"]]
        x_ls, _ = triangulate_rays(rays, centers)
        x, _, _ = triangulate_rays_robust(rays, centers, threshold=TAU)
        e_ls = np.linalg.norm(x_ls.cpu().numpy() - case["points"], axis=-1)
        e = np.linalg.norm(x.cpu().numpy() - case["points"], axis=-1)
        ok = ~np.isnan(e)
        lines.append("%3d %3d %3d | %24.4f | %24.4f | %d of %d" % (B, V, J, e_ls.mean(), e[ok].mean(), ok.sum(), ok.size))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
