"""A non-finite input poisons its own pose and nothing else, on every path of the forward.

Missing detections reach the model as NaN keypoints, NaN or infinite confidences and NaN rays.  The engines pack several samples
into one workgroup (16 sequences per SPT workgroup, 16 / 32 / 64-row tiles of V rows per sample in the block stack), the
split-operand engine clamps its LayerNorm outputs into the fp16 window -- which turns a NaN operand into a finite one, so that only
the fp32 residual keeps the row NaN --, and the bf16 engines, the small-batch {value, tag} engine, the joints x views grid
kernels and the three tails each have their own way from input to pose.  For every model of both tables of
tests/forward_paths.py, every channel (keypoint, confidence, ray, center) and NaN, +inf, -inf, with the first and the last
sample of the batch poisoned (and, for a NaN keypoint, an interior sample alone and every sample):

  1. the poisoned samples are NaN in every element of every output if the float64 oracle says these flags read the channel
     (tests/nonfinite_cases.py expected(); tests/test_nonfinite_cpu.py holds the survey), bitwise the clean run's otherwise:
     a finite value where the oracle has NaN fails, however plausible;
  2. every other sample is bitwise the clean run of the same model, batch and launch form;
  3. nothing is latched: the sticky device error word is clear after a synchronize, check_device() does not raise, and the clean
     forward issued next on the same model and workspace returns the clean bits (a non-finite input is the caller's data; the
     reference answers it with NaN, so does the device, and it reports nothing);
  4. the launch forms are those of the clean run, and the ones the case is there for.

No tolerance anywhere: masks and bit patterns.  Every violation of a model is collected and reported together.
"""
import ctypes as C

import pytest
import torch

from tests import nonfinite_cases as nf
from tests.forward_paths import DEV, FLAG_MODELS, FORWARD_MODELS, _fresh_model, _stack_shape

pytestmark = pytest.mark.gpu

MODELS = dict(FORWARD_MODELS, **FLAG_MODELS)
assert len(MODELS) == len(FORWARD_MODELS) + len(FLAG_MODELS)


def _batch(name, lib, cabi):
    flags, prec, small, want_stack, _, B = MODELS[name]
    if name in FLAG_MODELS or want_stack is None:
        return max(3, B)
    n_tok, D = _stack_shape(flags)
    parts = {"fp32": 2, "bf16": 1, "fp32_mfma": 0}[prec]
    sflags = 0 if small == "auto" else cabi.F_NO_SMALL_STACK
    form = getattr(cabi, "FORM_" + want_stack)
    B = next((b for b in range(3, 4097) if lib.mpl_block_stack_form(b, n_tok, D, flags["num_heads"], flags["depth"] + 1, parts, sflags) == form), None)
    assert B is not None, "%s: no batch from 3 to 4096 is sent to %s on this device" % (name, want_stack)
    return B


class _Runner:
    """one model, its clean run at batch B and the contract of one poisoned forward after another"""

    def __init__(self, name, model, B, lib, cabi):
        from openmpl_amd import detrng
        flags = MODELS[name][0]
        self.name, self.m, self.B, self.lib, self.cabi, self.flags = name, model, B, lib, cabi, flags
        p, r, c = detrng.make_inputs(B, flags["num_views"], flags["num_joints"], seed=nf.ISEED)
        self.inputs = tuple([torch.from_numpy(x).to(DEV) for x in l] for l in (p, r, c))
        self.problems = []
        self.clean, self.forms = self.forward(self.inputs)
        assert all(bool(torch.isfinite(t).all()) for t in self.clean), "%s: the clean run is not finite" % name
        assert not cabi.device_error(), "%s: the clean run latched the device error word" % name

    def forward(self, inputs):
        poses, rays, centers = inputs
        with torch.no_grad():
            out = self.m(poses, rays=rays, centers=centers)
        torch.cuda.synchronize()
        ent = self.m._hip_cache[torch.device(DEV).index]
        spw = C.c_int(0)
        forms = (self.lib.mpl_block_stack_last_form(),
                 self.lib.mpl_spt_form(C.byref(ent["cfg"]), self.B, int(ent["weights"].spt_packed), 0, C.byref(spw)))
        return [t.detach().cpu() for t in nf.flatten(out)], forms

    def poisoned(self, victims, channel, value):
        import openmpl_amd
        what = "%s B = %d: %r in %s of samples %s" % (self.name, self.B, value, channel, list(victims))
        consumed = nf.expected(self.flags, channel, value)
        got, forms = self.forward(nf.poison(self.inputs, victims, channel, value))
        verdict = nf.check(self.clean, got, victims, consumed)                                    # 1 and 2
        if verdict:
            self.problems.append("%s (the oracle: %s):\n%s" % (what, "all NaN" if consumed else "not read", verdict))
        word = self.lib.mpl_device_error(-1)                                                      # 3
        if word or self.cabi.device_error():
            self.problems.append("%s: the device error word is %d" % (what, word))
            try:
                openmpl_amd.check_device()
                self.problems.append("%s: check_device() is silent about the word" % what)
            except RuntimeError as e:
                self.problems.append("%s: check_device() raises: %s" % (what, e))
            self.cabi.clear_device_error()       # so that the clean forward below tells what the kernels left, not what the word says
        else:
            openmpl_amd.check_device()
        if forms != self.forms:                                                                   # 4
            self.problems.append("%s: launch forms %s where the clean run took %s" % (what, forms, self.forms))
        again, forms = self.forward(self.inputs)
        verdict = nf.check(self.clean, again, (), False)
        if verdict or forms != self.forms or self.cabi.device_error():
            self.problems.append("%s: the clean forward issued next (forms %s, error word %d):\n%s"
                                 % (what, forms, self.lib.mpl_device_error(-1), verdict))

    def all_cases(self):
        B = self.B
        for channel in nf.CHANNELS:
            for value in nf.VALUES:
                self.poisoned(sorted({0, B - 1}), channel, value)
        if B >= 3:
            self.poisoned([B // 2], "keypoint", float("nan"))
        self.poisoned(list(range(B)), "keypoint", float("nan"))


@pytest.mark.parametrize("name", sorted(MODELS))
def test_nonfinite_input_poisons_its_own_pose_and_nothing_else(name, capsys):
    from openmpl_amd import cabi
    flags, prec, small, want_stack, want_spt, _ = MODELS[name]
    lib = cabi.load()
    cabi.clear_device_error()
    try:
        B = _batch(name, lib, cabi)
        model = _fresh_model(flags, prec, small)
        run = _Runner(name, model, B, lib, cabi)
        stack, spt = run.forms
        if want_stack is not None:
            assert stack == getattr(cabi, "FORM_" + want_stack), "%s: the stack took form %d at B = %d" % (name, stack, B)
        assert spt in {getattr(cabi, "SPT_" + s) for s in want_spt}, "%s: the SPT stage took form %d" % (name, spt)
        run.all_cases()
        runs = [run]
        if name == "small_engine_b1":
            # the single sample of the launch is the poisoned one: the {value, tag} hand-off carries nothing but NaN values
            one = _Runner(name, model, 1, lib, cabi)
            assert one.forms[0] == cabi.FORM_SMALL, "%s: the stack took form %d at B = 1" % (name, one.forms[0])
            one.all_cases()
            runs.append(one)
        with capsys.disabled():
            for r in runs:
                print("\nnonfinite %s: B = %d, stack form %s, SPT form %d, %d violation(s)" % (name, r.B, r.forms[0], r.forms[1], len(r.problems)))
        problems = [p for r in runs for p in r.problems]
        assert not problems, "%d violation(s):\n%s" % (len(problems), "\n".join(problems))
    finally:
        cabi.clear_device_error()        # a finding here must not make every later test of the process raise
