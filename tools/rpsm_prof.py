"""Device time of openmpl_amd.rpsm (csrc/rpsm.hip) and of its three stages, beside the first-round max-product written with torch ops.

    python tools/rpsm_prof.py [OUT.txt]        (default: profiles/rpsm.txt of this repository)

Sizes: V = 4, J = 17 (the HumanBody tree), 64x64 float32 maps, 16^3 first bins, 2^3 recursion bins, depth 10; B = 1 and B = 64
(tests/rpsm_cases.inputs).  Method: every figure is the median of 50 runs after 5 warm-up runs; a run is timed by the library's own
event brackets around each launch (mpl_profile_start / stop, summed over the launches of the stage) and, beside it, by one event
pair around the whole call, which adds the gaps between the launches.  The stages are issued alone through the `stages` mask of
mpl_rpsm: the unary launch; the level launches on energies a fresh unary launch (not timed) has just written; the final launch on
the finished tables.
Yardstick, in the same loop, alternating with the level launches: the same first-round step as a user would write it with torch on the
device -- per edge, children first, torch.where(allowed, energy[child][None, :], 0).max(dim=1), the parent's energy times the
maxima -- in float64 on the kernel's own unary terms, with the (nbins, nbins) allowed masks of all edges built beforehand and not
timed (the reference passes them in precomputed as well).  It handles one pose; a batch is that many runs in a row.
Pair tests: edges x nbins^2 per pose.  The issue rate they are set against: 256 CUs x 64 lanes x 2.4 GHz = 39.3e12 lane-instructions
per second (the FP32 vector peak of 157.3 TFLOPS in MI355X_MICROARCH.md is 2 flop x 2 packed halves of that; one fp64 instruction
takes one such slot)."""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import openmpl_amd      # noqa: E402
from openmpl_amd import build as mpl_build, cabi      # noqa: E402
from tests import rpsm_cases as rc      # noqa: E402

DEV = "cuda:0"
RUNS, WARM = 50, 5
LANE_RATE = 256 * 64 * 2.4e9


def dev(x):
    return None if x is None else torch.from_numpy(np.array(x)).to(DEV)


def event_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def bracket_us(fn):
    cabi.profile_start()
    fn()
    torch.cuda.synchronize()
    ms, k = cabi.profile_stop()["fuse_head"]
    return ms * 1e3, k


def yardstick(E0, masks, order):
    """the first round's max-product with torch ops: E0 (J,nb) float64, masks {child: (nb,nb) bool}, order [(parent, child)]"""
    E = E0.clone()
    zero = torch.zeros((), dtype=torch.float64, device=E.device)
    back = {}
    for p, c in order:
        val, idx = torch.where(masks[c], E[c][None, :], zero).max(dim=1)
        E[p] = E[p] * val
        back[c] = idx
    return E, back


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "rpsm.txt")
    lib = cabi.load()
    kw = dict(first_nbins=16, recur_nbins=2, recur_depth=10)
    lines = ["rpsm: device time per call and per stage, V = 4, J = 17, 64x64 float32 maps, 16^3 / 2^3 / depth 10",
             "library source hash %s" % mpl_build.source_hash(), "device %s" % torch.cuda.get_device_name(0),
             "median of %d runs after %d warm-up runs; brackets = the library's event pairs summed over the stage's launches, "
             "call = one event pair around the call" % (RUNS, WARM), ""]
    parents = list(rc.BODY)
    dep = rc.depths(parents)
    order = [(parents[c], c) for c in sorted(range(1, 17), key=lambda j: (-dep[parents[j]], parents[j], j))]
    for B in (1, 64):
        inp = rc.inputs(B=B, seed=14, **kw)
        args = (dev(inp["hm"]), dev(inp["center"]), dev(inp["scale"]), dev(inp["cams"]), inp["image_size"], dev(inp["root_center"]), dev(inp["limb"]))
        J, nb = 17, 16 ** 3
        ws = torch.empty(lib.mpl_rpsm_workspace_bytes(B, J, 16), dtype=torch.uint8, device=DEV)
        run = lambda stages: openmpl_amd.rpsm(*args, _stages=stages, _workspace=ws, **kw)      # noqa: E731
        res = run(cabi.RPSM_ALL)
        err = np.linalg.norm(res.poses.cpu().numpy().astype(np.float64) - inp["truth"], axis=-1)
        # the yardstick's inputs: the kernel's unary terms of pose 0 and the allowed masks of its edges
        run(cabi.RPSM_UNARY)
        torch.cuda.synchronize()
        E0 = ws[:B * J * nb * 8].view(torch.float64).view(B, J, nb)[0].clone()
        g = dev(rc.grid(2000.0, inp["root_center"][0].astype(np.float64), 16))
        d = torch.cdist(g, g)
        masks = {c: ((d - float(inp["limb"][c])).abs() <= 150.0) for _, c in order}
        del d
        E1, back = yardstick(E0, masks, order)
        run(cabi.RPSM_ALL)
        torch.cuda.synchronize()
        Ek = ws[:B * J * nb * 8].view(torch.float64).view(B, J, nb)[0]
        bk = ws[B * J * nb * 8:].view(torch.int16).view(B, J, nb)[0]
        same = all(torch.equal(back[c].to(torch.int16), bk[c]) for _, c in order)
        rel = float(((Ek[0] - E1[0]).abs() / E1[0].abs().max()).max())
        t = {k: [] for k in ("all_b", "all_c", "unary_b", "unary_c", "levels_b", "levels_c", "final_b", "final_c", "yard")}
        launches = {}
        for i in range(WARM + RUNS):
            vals = {}
            (vals["all_b"], launches["all"]), vals["all_c"] = bracket_us(lambda: run(cabi.RPSM_ALL)), event_us(lambda: run(cabi.RPSM_ALL))
            (vals["unary_b"], launches["unary"]), vals["unary_c"] = bracket_us(lambda: run(cabi.RPSM_UNARY)), event_us(lambda: run(cabi.RPSM_UNARY))
            (vals["levels_b"], launches["levels"]) = bracket_us(lambda: run(cabi.RPSM_LEVELS))
            vals["yard"] = event_us(lambda: yardstick(E0, masks, order))
            run(cabi.RPSM_UNARY)
            vals["levels_c"] = event_us(lambda: run(cabi.RPSM_LEVELS))
            (vals["final_b"], launches["final"]), vals["final_c"] = bracket_us(lambda: run(cabi.RPSM_FINAL)), event_us(lambda: run(cabi.RPSM_FINAL))
            run(cabi.RPSM_UNARY)            # the next round's level launches start from fresh unary terms again
            if i >= WARM:
                for k, v in vals.items():
                    t[k].append(v)
        m = {k: statistics.median(v) for k, v in t.items()}
        pairs = 16.0 * nb * nb * B
        lines += ["B = %d   (mean joint error of the result %.2f mm, worst %.2f mm)" % (B, err.mean(), err.max()),
                  "%-34s | %8s | %12s | %12s" % ("stage", "launches", "brackets us", "call us"),
                  "%-34s | %8d | %12.1f | %12.1f" % ("whole call", launches["all"], m["all_b"], m["all_c"]),
                  "%-34s | %8d | %12.1f | %12.1f" % ("unary, first round", launches["unary"], m["unary_b"], m["unary_c"]),
                  "%-34s | %8d | %12.1f | %12.1f" % ("max-product, first round", launches["levels"], m["levels_b"], m["levels_c"]),
                  "%-34s | %8d | %12.1f | %12.1f" % ("walk down + %d recursion rounds" % kw["recur_depth"], launches["final"], m["final_b"], m["final_c"]),
                  "%-34s | %8s | %12s | %12.1f   (one pose%s)" % ("torch yardstick, max-product", "-", "-", m["yard"],
                                                                  "" if B == 1 else "; x %d for the batch: %.1f" % (B, m["yard"] * B)),
                  "yardstick / kernel (call times, per batch): %.1f x; back-pointers equal the yardstick's: %s; root energies within %.1e"
                  % (m["yard"] * B / m["levels_c"], same, rel),
                  "pair tests: %.3g per call, %.3g per second of the level launches (brackets) = %.3f per lane-instruction slot of %.3g / s"
                  % (pairs, pairs / (m["levels_b"] * 1e-6), pairs / (m["levels_b"] * 1e-6) / LANE_RATE, LANE_RATE), ""]
        del masks, E0, E1, back, ws
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
