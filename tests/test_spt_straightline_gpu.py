"""The packed SPT kernel's 16-sequence form (csrc/spt_packed.hip spt3_kernel<16>: straight-line Linear phases per wave, attention
over live query tiles only) against its own small forms, bitwise, and against float64.

Batch: B16 + 3, B16 the smallest batch for which the library's launch rule (mpl_spt_form, asked on the device at hand) puts 16
sequences into a workgroup -- V = 4 on 256 CUs: B16 = 513, B = 516.  The last workgroup of every view is ragged: it holds B % 16
live sequences (asserted to be neither 0 nor 16; 4 on 256 CUs).  The stage runs alone (mpl_spt_tokens, the entry point of
tests/test_spt_stage_gpu.py; its output is the fpt_in tap), depth 2, under three flag sets: CHOSEN,
confidence_as_attention_uncertainty_weight (the weighted application: query rows scaled by the confidences) and
multiple_spatial_blocks (one weight set per view).

  * bitwise: the rows of the whole batch equal the rows of the same sequences run in consecutive slices, each slice as large as
    the form-8, the form-4 and the form-1 class allow (the first slice of each is asserted to take that form; a shorter last
    slice takes a smaller one).  The arithmetic of a row does not depend on the form, so any difference is a fault of a form.
  * float64: the same rows against the fpt_in tap of the float64 oracle, bound max(2e-5, 4 * e32) in both measures of
    mpl_oracle.rel_errors -- the bound of tests/test_spt_stage_gpu.py for the packed forms (tests/spt_stage_cases.py).
  * short schedules, depth 1: without the weighted application the stage runs 2 block applications (the last block is applied
    twice), with it 3.  The first application finds its weights staged under the embedding, the last one stages nothing
    (app + 1 < n_apps): both edges with nothing or one application between them.  Same two checks.
"""
import ctypes as C
import functools

import pytest
import torch

from openmpl_amd import cabi
from oracle import mpl_oracle
from tests.spt_stage_cases import E32_FACTOR, SPT_BOUND, case_flags, class_ranges, make_inputs, oracle_taps
from tests.test_spt_stage_gpu import CANARY_BITS, DEV, _Engine, _model, _stream

pytestmark = pytest.mark.gpu
V = 4
CASES = [("chosen", 2), ("conf_attnw", 2), ("multi_spt", 2), ("chosen", 1), ("conf_attnw", 1)]
IDS = ["%s-L%d" % c for c in CASES]


def _run_slice(eng, dev_inputs, a, b):
    """The stage on poses a .. b - 1 -> ((b - a) * V, width) rows; the canary rows behind them must keep their bits."""
    _, B, poses, rays, centers = eng.m._check_inputs(*([x[a:b].contiguous() for x in lst] for lst in dev_inputs))
    assert B == b - a
    inp = cabi.Inputs()
    inp.batch = B
    for v in range(V):
        inp.poses[v], inp.rays[v], inp.centers[v] = poses[v].data_ptr(), rays[v].data_ptr(), centers[v].data_ptr()
    buf = torch.full((B * V + 17 * V, eng.width), float("nan"), device=DEV)
    buf[B * V:].view(torch.int32).fill_(CANARY_BITS)
    cabi.check(eng.lib.mpl_spt_tokens(C.byref(eng.cfg), C.byref(eng.ent["weights"]), C.byref(inp), buf.data_ptr(), _stream()),
               "mpl_spt_tokens")
    torch.cuda.synchronize()
    assert bool((buf[B * V:].view(torch.int32) == CANARY_BITS).all()), "rows behind B * V were written (poses %d .. %d)" % (a, b)
    assert eng.lib.mpl_device_error(0) == 0
    return buf[:B * V]


@functools.lru_cache(maxsize=None)
def _case(variant, depth):
    """Everything the checks of one case share, computed once: (engine, class ranges, B, device inputs, rows of the whole batch,
    float64 tap, float32 tap)."""
    flags = case_flags(variant, V, depth)
    m = _model(flags)
    eng = _Engine(m, "packed")
    assert eng.use_packed
    ranges = class_ranges(eng.form)
    assert (cabi.SPT_PACKED, 16) in ranges, "the 16-sequence form cannot be reached on this device: %s" % sorted(ranges)
    B = ranges[(cabi.SPT_PACKED, 16)][0] + 3
    assert eng.form(B) == (cabi.SPT_PACKED, 16) and B % 16 != 0
    inputs = make_inputs(B, flags)
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    ref64, ref32, _ = oracle_taps(sd, flags, inputs)
    dev_inputs = tuple([x.to(DEV) for x in lst] for lst in inputs)
    whole = _run_slice(eng, dev_inputs, 0, B)
    print("%s L=%d: B = %d, last workgroup holds %d sequences" % (variant, depth, B, B % 16))
    return eng, ranges, B, dev_inputs, whole, ref64, ref32


@pytest.mark.parametrize("variant,depth", CASES, ids=IDS)
def test_form16_equals_the_small_forms_bitwise(variant, depth):
    eng, ranges, B, dev_inputs, whole, _, _ = _case(variant, depth)
    assert bool(torch.isfinite(whole).all())
    for ss in (8, 4, 1):
        step = ranges[(cabi.SPT_PACKED, ss)][1]          # the largest batch of the class
        assert eng.form(min(step, B)) == (cabi.SPT_PACKED, ss), (ss, step, eng.form(min(step, B)))
        parts = [_run_slice(eng, dev_inputs, a, min(a + step, B)) for a in range(0, B, step)]
        got = torch.cat(parts)
        if not torch.equal(got, whole):
            diff = (got != whole).any(1).nonzero().flatten()
            raise AssertionError("%s L=%d: B=%d in form 16 differs bitwise from slices of %d (form %d) in %d rows (row = pose * V "
                                 "+ view), first %s" % (variant, depth, B, step, ss, diff.numel(), diff[:8].tolist()))


@pytest.mark.parametrize("variant,depth", CASES, ids=IDS)
def test_form16_against_fp64(variant, depth):
    _, _, B, _, whole, ref64, ref32 = _case(variant, depth)
    got = whole.reshape(B, -1).cpu()
    mx, nw = mpl_oracle.rel_errors(got, ref64)
    mx32, nw32 = mpl_oracle.rel_errors(ref32, ref64)
    print("%s L=%d B=%d: kernel max-scaled %.3e norm-wise %.3e | float32 oracle %.3e %.3e" % (variant, depth, B, mx, nw, mx32, nw32))
    assert bool(torch.isfinite(whole).all())
    assert mx <= max(SPT_BOUND, E32_FACTOR * mx32) and nw <= max(SPT_BOUND, E32_FACTOR * nw32), (mx, nw, mx32, nw32)
