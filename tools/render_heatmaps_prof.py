"""Device time of one render_heatmaps call (csrc/heatmap_render.hip) beside the store floor and the torch expression it replaces,
and of the sub-pixel decodes (csrc/heatmaps.hip) beside post_process=True in the same run.

    python tools/render_heatmaps_prof.py [OUT.txt]        (default: profiles/render_heatmaps.txt of this repository)

Size: B = 1024, V = 4, J = 17 maps of 64 x 64 (69 632 maps; 1.14 GB in fp32, 0.57 GB in bf16: neither fits the 256 MiB Infinity
Cache, so every launch streams to HBM), and the single-frame shape B = 1 (68 maps, 1.1 MB).
Method: 5 warm-up launches per variant, then 50 rounds in which the variants take turns, each launch timed on its own and followed
by a synchronise; the figure is the median of the 50, the spread min .. max.  render_heatmaps and decode_heatmaps are timed inside
the library's event brackets (mpl_profile_start / stop: two events around the launch), the torch calls between two events of their
own on the same stream.  Baselines of the render: Tensor.zero_() over the same bytes, the store floor, with Tensor.fill_(0.5)
beside it (the same stores of a value that is not zero); and the torch expression of tools/decode_heatmaps_prof.make_maps (exp of
a broadcast difference, then the cast), what a caller wrote before.  Bytes = the bytes of the maps.
Maps wider or higher than 64 cells take the renderer's other path, which evaluates the exponentials per cell: 128 x 128 fp32 maps
at B = 64 (4352 maps, 285 MB) are timed beside zero_() as well, so that the figures above are not read as holding for them."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openmpl_amd import build as mpl_build, cabi, decode_heatmaps, render_heatmaps      # noqa: E402

DEV = "cuda:0"
WARM, ROUNDS = 5, 50
V, J, H, W = 4, 17, 64, 64


def bracketed(call):
    cabi.profile_start()
    call()
    torch.cuda.synchronize()
    ms, k = cabi.profile_stop()["fuse_head"]
    assert k == 1
    return ms * 1e3


def evented(call):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def torch_maps(mx, my, amp, dtype):
    x, y = torch.arange(W, device=DEV).view(1, 1, 1, 1, W), torch.arange(H, device=DEV).view(1, 1, 1, H, 1)
    return (amp * torch.exp(-((x - mx) ** 2 + (y - my) ** 2) / 8.0)).to(dtype)


def measure(runs):
    """runs: (name, timer, call) -> medians and spreads in us, the variants taking turns"""
    for _, timer, call in runs:
        for _ in range(WARM):
            timer(call)
    us = [[] for _ in runs]
    for _ in range(ROUNDS):
        for k, (_, timer, call) in enumerate(runs):
            us[k].append(timer(call))
    return [(statistics.median(u), min(u), max(u)) for u in us]


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "render_heatmaps.txt")
    cabi.load()
    head = "%-6s %-5s %-34s | %26s | %6s | %s"
    lines = ["render_kernel and decode_kernel (sub-pixel): device time per launch, V = %d, J = %d, %d x %d maps" % (V, J, H, W),
             "library source hash %s" % mpl_build.source_hash(),
             "device %s" % torch.cuda.get_device_name(0),
             "time: median of %d launches, the variants taking turns, after %d warm-up launches each (min .. max); the library's calls inside"
             % (ROUNDS, WARM), "its event brackets, the torch calls between two events; TB/s = bytes of the maps / median", ""]
    render_rows, decode_rows = [head % ("B", "dtype", "call", "us per launch", "TB/s", "vs zero_()")], [head % ("B", "dtype", "call", "us per launch", "TB/s", "vs post_process")]
    for B in (1024, 1):
        for dtype, name in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
            g = torch.Generator(device=DEV)
            g.manual_seed(1)
            u = lambda *s: torch.rand(s, generator=g, device=DEV)
            cells = torch.stack([u(B, V, J) * (W - 1), u(B, V, J) * (H - 1)], -1)
            amp = 0.2 + 0.8 * u(B, V, J)
            mx, my, a5 = cells[..., 0].view(B, V, J, 1, 1), cells[..., 1].view(B, V, J, 1, 1), amp.view(B, V, J, 1, 1)
            out = torch.empty((B, V, J, H, W), dtype=dtype, device=DEV)
            nbytes = out.numel() * out.element_size()
            runs = [("Tensor.zero_()", evented, lambda: out.zero_()),
                    ("Tensor.fill_(0.5)", evented, lambda: out.fill_(0.5)),
                    ("torch expression", evented, lambda: torch_maps(mx, my, a5, dtype)),
                    ("render subpixel", bracketed, lambda: render_heatmaps(cells, amp, mode="subpixel", out=out)),
                    ("render reference", bracketed, lambda: render_heatmaps(cells, amp, mode="reference", out=out)),
                    ("render subpixel + noise 0.004", bracketed, lambda: render_heatmaps(cells, amp, mode="subpixel", noise_level=0.004, out=out))]
            res = measure(runs)
            for (what, _, _), (med, lo, hi) in zip(runs, res):
                render_rows.append("%-6d %-5s %-34s | %9.2f (%.2f .. %.2f) | %6.2f | %.2f x" % (B, name, what, med, lo, hi, nbytes / med * 1e-6, med / res[0][0]))
            # the maps being timed are the right ones: the torch expression within its own float32 error of the kernel's float64
            r = render_heatmaps(cells, amp, mode="subpixel", out=out)
            ref = torch_maps(mx, my, a5, torch.float32)
            assert float((r.heatmaps.float() - ref).abs().max()) <= (2e-6 if dtype == torch.float32 else 8e-3)
            del ref
            # the decodes, on the noisy maps of the render
            hm = render_heatmaps(cells, amp, mode="subpixel", noise_level=0.004, out=out).heatmaps
            center = 500.0 + 100.0 * torch.rand((B, V, 2), device=DEV)
            scale = 1.0 + torch.rand((B, V, 2), device=DEV)
            runs = [("decode post_process", bracketed, lambda: decode_heatmaps(hm, center, scale, post_process=True)),
                    ("decode subpixel gaussian", bracketed, lambda: decode_heatmaps(hm, center, scale, subpixel="gaussian")),
                    ("decode subpixel centroid r=2", bracketed, lambda: decode_heatmaps(hm, center, scale, subpixel="centroid", radius=2)),
                    ("decode subpixel centroid r=6", bracketed, lambda: decode_heatmaps(hm, center, scale, subpixel="centroid", radius=6))]
            res = measure(runs)
            for (what, _, _), (med, lo, hi) in zip(runs, res):
                decode_rows.append("%-6d %-5s %-34s | %9.2f (%.2f .. %.2f) | %6.2f | %.2f x" % (B, name, what, med, lo, hi, nbytes / med * 1e-6, med / res[0][0]))
            # and they decode what was rendered: the log-quadratic fit finds the interior means
            d = decode_heatmaps(hm, subpixel="gaussian")
            inside = ((cells >= 3) & (cells <= torch.tensor([W - 4.0, H - 4.0], device=DEV))).all(-1)
            err = (d.pixels - cells).abs()[inside]
            decode_rows.append("%-6d %-5s gaussian on these maps: per-axis error worst %.4f / mean %.4f cells" % (B, name, float(err.max()), float(err.mean())))
            del out, hm, r, d
            torch.cuda.empty_cache()
    # the per-cell path of maps larger than 64 x 64
    B, S = 64, 128
    g = torch.Generator(device=DEV)
    g.manual_seed(2)
    cells = torch.rand((B, V, J, 2), generator=g, device=DEV) * (S - 1)
    out = torch.empty((B, V, J, S, S), dtype=torch.float32, device=DEV)
    nbytes = out.numel() * out.element_size()
    runs = [("Tensor.zero_()", evented, lambda: out.zero_()),
            ("render subpixel", bracketed, lambda: render_heatmaps(cells, mode="subpixel", out=out)),
            ("render reference", bracketed, lambda: render_heatmaps(cells, mode="reference", out=out))]
    res = measure(runs)
    wide_rows = ["", "%d x %d maps, B = %d (the factors are evaluated per cell)" % (S, S, B)]
    for (what, _, _), (med, lo, hi) in zip(runs, res):
        wide_rows.append("%-6d %-5s %-34s | %9.2f (%.2f .. %.2f) | %6.2f | %.2f x" % (B, "fp32", what, med, lo, hi, nbytes / med * 1e-6, med / res[0][0]))
    render_rows += wide_rows
    del out
    text = "\n".join(lines + render_rows + [""] + decode_rows + ["", "in-order HBM sweep of a 1.2 GB table on this device class: 6.0 - 6.1 TB/s"]) + "\n"
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
