"""GPU test of bench.py's plain run: the result line carries the headline fields only, and --dump-outputs writes what the
timed path returned in its last step.  Both the benchmark and the direct forwards it is checked against run in fresh
child processes (this process never initialises the GPU)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import mpl_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "rccl_ranks", "config"}

# the forwards of bench.py's four resident batches, one call each, through bench.py's own model and input helpers
DIRECT = """
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
from bench import build_model, make_batch, model_flags
B, V, out = int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
dev = torch.device("cuda", 0)
m = build_model(model_flags("chosen", V, 12), dev)
m.set_matmul_precision("fp32")
with torch.no_grad():
    ys = [m(P, rays=R, centers=C).cpu().numpy() for P, R, C in (make_batch(B, V, dev, seed=1000, step=s) for s in range(4))]
np.save(out, np.stack(ys))
"""


@pytest.mark.gpu
def test_plain_bench_line_is_lean_and_dumps_the_last_timed_step(tmp_path):
    B, V, steps = 64, 4, 3
    dump = str(tmp_path / "outputs")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--batch", str(B), "--views", str(V), "--dump-outputs", dump], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-4000:]
    lines = [l for l in r.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    j = json.loads(lines[0])
    assert set(j) == HEADLINE, sorted(set(j) ^ HEADLINE)
    assert j["steps"] == steps and j["warmup"] == 1 and j["ms_per_step"] > 0 and j["value"] > 0
    assert abs(j["value"] - B / j["ms_per_step"] * 1e3) <= 1e-3 * j["value"]
    assert sorted(os.listdir(dump)) == ["poses_3d.npy"]
    got = np.load(os.path.join(dump, "poses_3d.npy"))
    assert got.dtype == np.float32 and got.shape == (B, 17, 3)

    ref_path = str(tmp_path / "direct.npy")
    r = subprocess.run([sys.executable, "-c", DIRECT, ROOT, str(B), str(V), ref_path], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-4000:]
    direct = np.load(ref_path)
    last = (steps - 1) % 4                                   # the timed steps cycle through the four batches
    for s in range(4):
        mx, nw = mpl_oracle.rel_errors(torch.from_numpy(got), torch.from_numpy(direct[s]))
        if s == last:
            assert mx < 1e-6 and nw < 1e-6, (s, mx, nw)
        else:
            assert mx > 1e-2, (s, mx, nw)
