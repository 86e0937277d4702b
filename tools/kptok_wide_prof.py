"""Error and kernel time of the streaming attention for wide heads (csrc/token_attention_wide.hip), per stage case of
tests/test_kptok_wide_gpu.py, and the same-FLOP yardstick against the head-dim-4 kernel.

    python tools/kptok_wide_prof.py [OUT.txt]        (default: profiles/kptok_wide_attention.txt of this repository)

Times: mpl_profile_start / stop around each launch (events on the stream), median of 7 launches after 2 warm-up launches.
Yardstick: n_seq = 256, n_tok = 527, D = 32 does n_tok^2 * D multiply-adds per sequence and product whether it is 8 heads of 4
(token_attention_long_p4_kernel), 2 heads of 16 or 1 head of 32 (token_attention_wide_kernel)."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openmpl_amd import build as mpl_build, cabi      # noqa: E402
from tests.kptok_wide_cases import STAGE_CASES, attention_formula, stage_errors, stage_qkv      # noqa: E402

DEV = "cuda:0"


def timed(qkv, n_seq, n_tok, dim, H, reps=7, warm=2):
    lib = cabi.load()
    out = torch.full((n_seq * n_tok, dim), float("nan"), device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    us = []
    for i in range(warm + reps):
        cabi.profile_start()
        cabi.check(lib.mpl_token_attention(qkv.data_ptr(), n_seq, n_tok, dim, H, out.data_ptr(), st), "mpl_token_attention")
        torch.cuda.synchronize()
        ms, n = cabi.profile_stop()["attention"]
        assert n == 1
        if i >= warm:
            us.append(ms * 1e3)
    return out, statistics.median(us), min(us)


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "kptok_wide_attention.txt")
    lines = ["token_attention_wide_kernel: error against float64 and kernel time per launch",
             "library source hash %s" % mpl_build.source_hash(),
             "device %s" % torch.cuda.get_device_name(0),
             "errors: max-scaled / norm-wise (mpl_oracle.rel_errors); e32 = the float32 torch formula on the CPU; time: median (min) of 7",
             "",
             "%5s %6s %4s %3s | %-21s | %-21s | %s" % ("n_seq", "n_tok", "hd", "H", "kernel error", "e32", "us per launch")]
    for n_seq, n_tok, hd, H in STAGE_CASES:
        qkv = stage_qkv(n_seq, n_tok, hd, H)
        out, med, mn = timed(qkv.to(DEV), n_seq, n_tok, H * hd, H)
        (mx, nw), (mx32, nw32) = stage_errors(qkv, out, n_seq, n_tok, H * hd, H)
        lines.append("%5d %6d %4d %3d | %.3e / %.3e | %.3e / %.3e | %8.1f (%.1f)" % (n_seq, n_tok, hd, H, mx, nw, mx32, nw32, med, mn))
    lines += ["", "same-FLOP yardstick: n_seq 256, n_tok 527, D 32 (8.9 G multiply-adds per product and launch)"]
    g = torch.Generator().manual_seed(527)
    qkv = torch.randn(256 * 527, 96, generator=g)
    for H, kernel in ((8, "token_attention_long_p4_kernel"), (4, "token_attention_long_kernel"), (2, "token_attention_wide_kernel<16>"),
                      (1, "token_attention_wide_kernel<32>")):
        out, med, mn = timed(qkv.to(DEV), 256, 527, 32, H)
        sl = slice(0, 2 * 527)                         # two sequences against float64 (the whole batch would take the CPU minutes)
        ref = attention_formula(qkv[sl], 2, 527, 32, H, torch.float64)
        err = (out[sl].cpu().double() - ref).abs().max().item() / ref.abs().max().item()
        lines.append("H %d (hd %2d) %-34s %8.1f us (min %.1f)   max-scaled error %.2e" % (H, 32 // H, kernel, med, mn, err))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
