"""Device time of one decode_heatmaps call (csrc/heatmaps.hip) beside torch.max over the same bytes.

    python tools/decode_heatmaps_prof.py [OUT.txt]        (default: profiles/decode_heatmaps.txt of this repository)

Size: B = 1024, V = 4, J = 17 maps of 64 x 64 (69 632 maps; 1.14 GB in fp32, 0.57 GB in bf16: neither fits the 256 MiB Infinity
Cache, so every launch streams from HBM), and the single-frame shape B = 1 (68 maps, 1.1 MB, cache-resident after the warm-up).
Maps: sub-pixel Gaussians, sigma 2, amplitude 0.2 .. 1, with uniform noise, made on the device from a fixed seed.
Method: 5 warm-up launches per variant, then 50 rounds in which the variants take turns, each launch timed on its own and followed
by a synchronise; the figure is the median of the 50, the spread min .. max.  decode_heatmaps is timed inside the library's event
brackets (mpl_profile_start / stop: two events around the launch), torch.max(hm.view(-1, H * W), dim=1) between two events of its
own on the same stream.  Bytes read = the bytes of the maps; the outputs (20 bytes per map, 44 more with cameras) are left out."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openmpl_amd import build as mpl_build, cabi, decode_heatmaps      # noqa: E402
from tests import synth_cases as sc      # noqa: E402

DEV = "cuda:0"
WARM, ROUNDS = 5, 50
V, J, H, W = 4, 17, 64, 64
WH = (1000.0, 1000.0)


def make_maps(B, dtype):
    g = torch.Generator(device=DEV)
    g.manual_seed(1)
    u = lambda *s: torch.rand(s, generator=g, device=DEV)
    mx, my, amp = u(B, V, J, 1, 1) * (W - 1), u(B, V, J, 1, 1) * (H - 1), 0.2 + 0.8 * u(B, V, J, 1, 1)
    x, y = torch.arange(W, device=DEV).view(1, 1, 1, 1, W), torch.arange(H, device=DEV).view(1, 1, 1, H, 1)
    hm = amp * torch.exp(-((x - mx) ** 2 + (y - my) ** 2) / 8.0)
    hm += 0.004 * u(B, V, J, H, W)
    return hm.to(dtype)


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


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "decode_heatmaps.txt")
    cabi.load()
    cams = torch.from_numpy(sc.scene(1, V, J, seed=1)[1]).to(DEV)
    lines = ["decode_kernel: device time per launch, V = %d, J = %d, %d x %d maps" % (V, J, H, W),
             "library source hash %s" % mpl_build.source_hash(),
             "device %s" % torch.cuda.get_device_name(0),
             "time: median of %d launches, the variants taking turns, after %d warm-up launches each (min .. max); decode_heatmaps inside the"
             % (ROUNDS, WARM), "library's event brackets, torch.max between two events; TB/s = bytes of the maps / median", "",
             "%-6s %-5s %-28s | %26s | %6s | %s" % ("B", "dtype", "call", "us per launch", "TB/s", "vs torch.max")]
    for B in (1024, 1):
        for dtype, name in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
            hm = make_maps(B, dtype)
            center = 500.0 + 100.0 * torch.rand((B, V, 2), device=DEV)
            scale = 1.0 + torch.rand((B, V, 2), device=DEV)
            flat = hm.view(-1, H * W)
            runs = [("torch.max(dim=1)", evented, lambda: torch.max(flat, dim=1)),
                    ("decode plain", bracketed, lambda: decode_heatmaps(hm, center, scale)),
                    ("decode post_process", bracketed, lambda: decode_heatmaps(hm, center, scale, post_process=True)),
                    ("decode post_process + cams", bracketed, lambda: decode_heatmaps(hm, center, scale, post_process=True, cams=cams, image_size=WH))]
            for _, timer, call in runs:
                for _ in range(WARM):
                    timer(call)
            us = [[] for _ in runs]
            for _ in range(ROUNDS):
                for k, (_, timer, call) in enumerate(runs):
                    us[k].append(timer(call))
            nbytes = hm.numel() * hm.element_size()
            base = statistics.median(us[0])
            for k, (what, _, _) in enumerate(runs):
                med = statistics.median(us[k])
                lines.append("%-6d %-5s %-28s | %9.2f (%.2f .. %.2f) | %6.2f | %.2f x" % (B, name, what, med, min(us[k]), max(us[k]), nbytes / med * 1e-6, med / base))
            # the results being timed are the right ones: the peak is torch's own
            val, idx = torch.max(flat.float(), dim=1)
            r = decode_heatmaps(hm, return_coords=True)
            assert torch.equal(r.conf.view(-1), val)
            if dtype == torch.float32:            # no two equal maxima in a map: torch's index is the first one as well
                assert torch.equal(r.coords.view(-1, 2)[:, 0] + W * r.coords.view(-1, 2)[:, 1], torch.where(val > 0, idx, 0).float())
            del hm, flat, val, idx, r
            torch.cuda.empty_cache()
    lines += ["", "in-order HBM sweep of a 1.2 GB table on this device class: 6.0 - 6.1 TB/s"]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
