"""poses/s of models outside NUM_JOINTS 17 / DIM 32 / HEADS 8 (and of 17 / 32 / 8 on the shape-general SPT next to the tuned one).

    python tools/shape_bench.py [--batch 1024] [--views 4] [--depth 12] [--precision fp32 [bf16 ...]]

--precision takes one or more of fp32 / fp32_mfma / bf16; with several, every shape is measured under each in turn (the precisions
alternate shape by shape, so that they share the box's clock and thermal state).

One mpl_forward per step through the C ABI on the model's marshalled weights (the ctypes route of MultiView_MPL.forward), flags
CHOSEN; poses/s = median over 5 timed regions of 20 forwards each (bench.py's secondary numbers), after 10 warm-up forwards.  Each
line also gives the SPT / FPT / tail split of the kernel time (library event pairs, mpl_profile_start/stop).
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openmpl_amd import cabi, detrng                   # noqa: E402
from openmpl_amd.multiview_mpl import MultiView_MPL    # noqa: E402

SHAPES = [("j15_d32_h8", 15, 32, 8, 0), ("j20_d32_h8", 20, 32, 8, 0), ("j17_d2_h2", 17, 2, 2, 0),
          ("j17_d32_h8_tuned_spt", 17, 32, 8, 0), ("j17_d32_h8_generic_spt", 17, 32, 8, cabi.F_GENERIC_SPT)]


def measure(J, d, H, extra, B, V, L, prec, regions=5, per=20, warm=10):
    dev = torch.device("cuda:0")
    flags = dict(num_joints=J, embed_dim_ratio=d, num_heads=H, depth=L, num_views=V, pose_3d_emb_learnable=True)
    m = MultiView_MPL(**flags)
    detrng.fill_module_(m, seed=11)
    m = m.to(dev).eval().set_matmul_precision(prec)
    p, r, c = detrng.make_inputs(B, V, J, seed=1)
    poses = [torch.from_numpy(x).to(dev) for x in p]
    lib = cabi.load()
    ent = m._marshal(dev)
    cfg = cabi.Config.from_buffer_copy(ent["cfg"])
    cfg.flags |= extra
    inp = cabi.Inputs()
    inp.batch = B
    for v in range(V):
        inp.poses[v] = poses[v].data_ptr()
    ws_bytes = lib.mpl_forward_workspace_bytes(C.byref(cfg), B)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out = torch.empty((B, J, 3), device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def step():
        cabi.check(lib.mpl_forward(C.byref(cfg), C.byref(ent["weights"]), C.byref(inp), out.data_ptr(), ws.data_ptr(), ws_bytes, st),
                   "mpl_forward")

    for _ in range(warm):
        step()
    torch.cuda.synchronize()
    rates = []
    for _ in range(regions):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(per):
            step()
        e1.record()
        e1.synchronize()
        rates.append(per * B / (e0.elapsed_time(e1) * 1e-3))
    rates.sort()
    cabi.profile_start()
    for _ in range(per):
        step()
    torch.cuda.synchronize()
    prof = cabi.profile_stop()
    ms = lambda *ks: sum(prof[k][0] for k in ks) / per
    return dict(poses_per_s=round(rates[len(rates) // 2]), spt_ms=round(ms("spt"), 4),
                fpt_ms=round(ms("row_stats", "gemm", "attention"), 4), tail_ms=round(ms("fuse_head"), 4),
                form=lib.mpl_block_stack_last_form())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--precision", nargs="+", default=["fp32"], choices=("fp32", "fp32_mfma", "bf16"))
    ap.add_argument("--only", default=None, help="one shape name")
    a = ap.parse_args()
    for name, J, d, H, extra in SHAPES:
        if a.only and name != a.only:
            continue
        for prec in a.precision:
            r = measure(J, d, H, extra, a.batch, a.views, a.depth, prec)
            print(json.dumps(dict(shape=name, batch=a.batch, views=a.views, depth=a.depth, precision=prec, **r)), flush=True)


if __name__ == "__main__":
    main()
