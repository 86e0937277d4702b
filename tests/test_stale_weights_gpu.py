"""No forward ever runs on stale weights: the table of tests/stale_cases.py on the device.

The reference is a FRESH module.  After every single step (one tensor updated, one route changed, one copy made) a new
MultiView_MPL is built from a clone of the live module's state_dict(), with the same precision and engine setting, on the plain
ctypes route, and run once on the same inputs: the live module must give its poses BIT FOR BIT (routes and repeated packings are
bitwise reproducible; the control -- two fresh modules agree -- is run once per model).  For the fp32 and fp32_mfma models the
fresh module itself is anchored to the float64 oracle on that state dict at the project's 1e-4 (max-scaled and norm-wise), on the
first rows of the batch (the poses of a batch are independent in eval mode), so "fresh" cannot drift either.  Per step, too: the
poses changed in bits (or, for requires_grad_, did not), the device-error word is clear, the library reports the stack / SPT form
the model is there for, and an in-place update of a tensor the kernels read in place keeps the extension binding.

Every sequence here is a legitimate call order; nothing is provoked.  Alias writes (through .data, through a flat buffer the
parameters view) are asserted as documented: after the write AND weights_changed() the live module is the fresh one."""
import ctypes as C
import gc

import pytest
import torch

from openmpl_amd import cabi
from openmpl_amd.multiview_mpl import MultiView_MPL
from oracle import mpl_oracle
from tests import stale_cases as S
from tests.forward_paths import DEV, _fresh_model, _stack_shape

pytestmark = pytest.mark.gpu
TOL = 1e-4
ANCHOR_ROWS = 2
PARTS = 4                    # the tensors of a model are visited in this many tests (every PARTS-th tensor each)


def _batch(model):
    flags, prec, small, want_stack, _, B = S.MODELS[model]
    if B is not None:
        return B
    lib = cabi.load()
    n_tok, D = _stack_shape(flags)
    parts = {"fp32": 2, "bf16": 1, "fp32_mfma": 0}[prec]
    sflags = 0 if small == "auto" else cabi.F_NO_SMALL_STACK
    form = getattr(cabi, "FORM_" + want_stack)
    B = next((b for b in range(1, 4097) if lib.mpl_block_stack_form(b, n_tok, D, flags["num_heads"], flags["depth"] + 1, parts, sflags) == form), None)
    assert B is not None, "%s: no batch up to 4096 is sent to %s on this device" % (model, want_stack)
    return B


POOL = 8                     # fresh modules are CONSTRUCTED this many at a time, ahead of the steps that use them (see _skeleton)


def _skeleton(model):
    """A new module of the model, same precision and engine, ctypes route, weights not yet loaded, no forward run.  Constructing
    ANY module registers parameters, which moves the process-wide generation counter in front of the extension shortcut
    (multiview_mpl._STRUCT_GEN) and sends the next forward of every live module through the complete check of _marshal.  A fresh
    module constructed between the update and the live forward would therefore hide exactly the shortcut under test (it hid the
    dead binding handle of a route change when this file was first written), so the objects are made ahead, POOL at a time, the
    live modules run one forward behind that, and the state dict is loaded -- in place, no registration -- after the step."""
    flags, prec, small = S.MODELS[model][:3]
    with torch.device(DEV):
        f = MultiView_MPL(**flags)
    return f.eval().use_torch_op(False).set_matmul_precision(prec).set_small_batch_engine(small)


def _fresh_from(m, model, skeleton=None):
    """A new module with a clone of the live module's state dict: same precision and engine, ctypes route, no forward yet."""
    f = skeleton if skeleton is not None else _skeleton(model)
    f.load_state_dict({k: v.detach().clone() for k, v in m.state_dict().items()}, strict=True)
    return f


_FILLED = {}


def _live_model(model):
    """forward_paths._fresh_model(flags, precision, engine) of the model: the deterministic fill is computed once per model."""
    flags, prec, small = S.MODELS[model][:3]
    if model not in _FILLED:
        m = _fresh_model(flags, prec, small)
        _FILLED[model] = {k: v.detach().clone() for k, v in m.state_dict().items()}
        return m
    with torch.device(DEV):
        m = MultiView_MPL(**flags)
    m.load_state_dict({k: v.clone() for k, v in _FILLED[model].items()}, strict=True)
    assert m._unsupported is None, m._unsupported
    return m.eval().use_torch_op(False).set_matmul_precision(prec).set_small_batch_engine(small)


class Run:
    """One live module of a model of the table, its inputs, and the per-step check."""

    def __init__(self, model, route="auto"):
        self.model, self.rec = model, S.MODELS[model]
        flags, prec, small = self.rec[:3]
        self.lib = cabi.load()
        self.B = _batch(model)
        self.np_inputs = S.inputs(model, self.B)
        self.P, self.R, self.Cn = ([torch.from_numpy(x).to(DEV) for x in lst] for lst in self.np_inputs)
        self.anchor_inputs = tuple([x[:ANCHOR_ROWS] for x in lst] for lst in self.np_inputs)
        self.live = _live_model(model).use_torch_op(route)
        self.idx = torch.device(DEV).index
        self.prev = None
        self.pool, self.also = [], []          # fresh modules made ahead; further modules whose shortcut must stay armed
        cabi.clear_device_error()

    def fresh(self, m):
        """(a fresh module of m's state dict, whether modules had to be constructed for it just now)."""
        made = not self.pool
        if made:
            self.pool = [_skeleton(self.model) for _ in range(POOL)]
        return _fresh_from(m, self.model, self.pool.pop()), made

    def rearm(self, expect=None):
        """After modules were constructed: one forward of every live module, so that the next step meets an armed shortcut."""
        for a in [self.live] + self.also:
            again = self.forward(a)
            if a is self.live and expect is not None:
                S.assert_same_bits(again, expect, "%s: the same forward once more" % self.model)

    def forward(self, m):
        with torch.no_grad():
            return S.flat(m(self.P, rays=self.R, centers=self.Cn))

    def handle(self, m=None):
        f = (m or self.live)._fast_bind.get(self.idx)
        return None if f is None else f[0]

    def forms(self, m):
        ent = m._hip_cache[self.idx]
        spw = C.c_int(0)
        return self.lib.mpl_block_stack_last_form(), self.lib.mpl_spt_form(C.byref(ent["cfg"]), self.B, int(ent["weights"].spt_packed), 0, C.byref(spw))

    def check(self, what, changed=True, m=None):
        """Forward on the live module; hold it to a fresh module (and that one to the oracle).  changed: True -- the poses must
        differ in bits from the step before; False -- they must be the same bits; None -- not asked."""
        m = m or self.live
        what = "%s: %s" % (self.model, what)
        live = self.forward(m)
        stack, spt = self.forms(m)
        fresh_m, made = self.fresh(m)
        fresh = self.forward(fresh_m)
        S.assert_same_bits(live, fresh, what)
        assert torch.isfinite(live).all(), what
        assert not cabi.device_error(), "%s: the device-error word is set (%d)" % (what, self.lib.mpl_device_error(-1))
        want_stack, want_spt = self.rec[3], self.rec[4]
        if want_stack is not None:
            assert stack == getattr(cabi, "FORM_" + want_stack), "%s: the stack took form %d, not %s" % (what, stack, want_stack)
        if want_spt is not None:
            assert spt in {getattr(cabi, "SPT_" + s) for s in want_spt}, "%s: the SPT stage took form %d" % (what, spt)
        if self.model in S.ANCHORED:
            ref = S.oracle_poses(self.model, fresh_m.state_dict(), self.anchor_inputs)
            got = fresh[:, :ANCHOR_ROWS] if fresh.dim() == 4 else fresh[:ANCHOR_ROWS]
            mx, nw = mpl_oracle.rel_errors(got.cpu(), ref)
            assert mx <= TOL and nw <= TOL, "%s: the FRESH module is off the float64 oracle: max-scaled %.3e norm-wise %.3e" % (what, mx, nw)
        if self.prev is not None and changed is not None:
            same = torch.equal(live, self.prev)
            assert same != changed, "%s: the poses %s" % (what, "did not change in a single bit" if changed else "changed although nothing was updated")
        if made:
            self.rearm(live if m is self.live else None)
        self.prev = live
        return live

    def get(self, name):
        return S._get(self.live, name)

    def update_in_place(self, name):
        """Kind (a) with the op of the table: mul_ for "mul", add_ for "add"."""
        p = self.get(name)
        op, mag = S.mutation(name)
        with torch.no_grad():
            if op == "mul":
                p.mul_(mag)
            else:
                p.add_(S.mutated(p, op, mag) - p)


def _assert_fold_table(run):
    """tests/stale_cases.FOLDED restates which block tensors are folded; _marshal's key says what it did fold."""
    h2, bf16, spt3, d32 = run.live._hip_cache[run.idx]["dkey"][1:5]
    assert (bool(h2 or bf16 or d32), bool(spt3)) == S.FOLDED[run.model], (run.model, h2, bf16, spt3, d32)


# ================================================================================================ every tensor, one at a time
@pytest.mark.parametrize("part", range(PARTS))
@pytest.mark.parametrize("model", sorted(S.MODELS))
def test_every_tensor_one_at_a_time(model, part):
    run = Run(model)
    names = S.tensor_names(run.live)
    base = run.check("first forward")
    _assert_fold_table(run)
    if part == 0:                                                   # the control, once per model
        a, b = run.fresh(run.live)[0], run.fresh(run.live)[0]
        S.assert_same_bits(run.forward(a), run.forward(b), "%s: control, two fresh modules of one state dict" % model)
    bound = model not in S.STAGED
    assert (run.handle() is not None) == bound, "%s: %s" % (model, "no extension binding on the default route" if bound else "a staged tail bound")
    for name in names[part::PARTS]:
        cls = S.fold_class(model, name)
        orig = run.get(name).detach().clone()
        h = run.handle()
        run.update_in_place(name)
        run.check("after an in-place update of %s (%s)" % (name, cls), changed=None if S.exempt(model, name) else True)
        if bound and cls in ("inplace", "buffer"):
            assert run.handle() == h, "%s: an in-place update of %s, which the kernels read in place, cost the binding" % (model, name)
        elif bound:
            assert run.handle() != h, "%s: %s is folded into a packed operand, yet its update kept the binding" % (model, name)
        # back to the first values, in place: the first poses, bit for bit (a re-pack of the same values gives the same operand)
        with torch.no_grad():
            run.get(name).copy_(orig)
        back = run.forward(run.live)
        S.assert_same_bits(back, base, "%s: %s restored in place" % (model, name))
        run.prev = back


# ================================================================================================ every kind of change
_FUSED = {}


def _kind_here(kind):
    if kind.endswith("_fused"):
        if "ok" not in _FUSED:
            _FUSED["ok"] = S.fused_optimizer_offered(DEV)
        if not _FUSED["ok"]:
            return kind[:-len("_fused")] + "_foreach"           # torch offers no fused step on this device: the foreach one runs
    return kind


@pytest.mark.parametrize("kind", S.NOTICED + S.UNCHANGED + S.ALIAS)
@pytest.mark.parametrize("model", S.KIND_MODELS)
def test_every_kind_of_change(model, kind):
    kind = _kind_here(kind)
    run = Run(model)
    run.check("first forward")
    for name in S.KIND_TARGETS[model]:
        if not S.applies(kind, run.live, name):
            continue
        what = "%s of %s (%s)" % (kind, name, S.fold_class(model, name))
        new = S.mutated(run.get(name), *S.mutation(name))
        h = run.handle()
        run.live = S.apply_kind(kind, run.live, name, new)
        if kind in S.UNCHANGED:
            run.check(what, changed=False)
            assert run.handle() == h, "%s: requires_grad_ cost the binding" % what
        elif kind in S.ALIAS:
            if kind == "j_flat_vector":
                run.check(what + ": the parameters became views of one flat buffer", changed=False)
                S.write_through_flat_vector(run.live, name, new)
            # the contract: such a write is followed by weights_changed(); then the forward runs the new weights
            assert run.live.weights_changed() is run.live
            run.check(what + " + weights_changed()")
        else:
            run.check(what)


# ================================================================================================ a change of route around a change of weights
@pytest.mark.parametrize("change", S.ROUTE_CHANGES)
@pytest.mark.parametrize("routes", S.ROUTE_PAIRS, ids=lambda r: "%s-%s" % r)
@pytest.mark.parametrize("model", S.ROUTE_MODELS)
def test_route_change_around_a_weight_change(model, routes, change):
    """forward on route 1, update, forward on route 2, forward on route 1 again (with "auto", False: the sequence that ended in
    'binding ... is not alive' before _marshal took the shortcut's handle away with the binding it released)."""
    r1, r2 = routes
    run = Run(model, route=r1)
    run.check("forward on %r" % (r1,))
    name = S.KIND_TARGETS[model][0 if change == "a_copy" else 1]
    run.live = S.apply_kind(change, run.live, name, S.mutated(run.get(name), *S.mutation(name)))
    run.live.use_torch_op(r2)
    run.check("%s of %s, then forward on %r" % (change, name, r2))
    run.live.use_torch_op(r1)
    run.check("back on %r" % (r1,), changed=False)
    run.live.use_torch_op(r2)
    run.check("and on %r once more" % (r2,), changed=False)


# ================================================================================================ copies and shared parameters
@pytest.mark.parametrize("model", ("small_engine_b1", "multi_spt", "deep_head"))
def test_copies_carry_their_own_weights(model):
    run = Run(model)
    base = run.check("first forward")
    name = S.KIND_TARGETS[model][0]
    for how, cp in S.copies_of(run.live):
        run.also = [cp]
        assert not cp._hip_cache and not cp._fast_bind, "%s: derived state travelled with the %s" % (model, how)
        S.assert_same_bits(run.forward(cp), base, "%s: the %s gives the original's bits" % (model, how))
        orig = run.get(name).detach().clone()
        run.update_in_place(name)                                                      # the original changes ...
        moved = run.check("the original after its update (a %s exists)" % how)
        S.assert_same_bits(run.forward(cp), base, "%s: the %s keeps its own weights" % (model, how))
        with torch.no_grad():
            run.get(name).copy_(orig)
            cpp = S._get(cp, name)
            cpp.add_(S.mutated(cpp, "add", 0.5) - cpp)                                 # ... then the copy does
        run.check("the original, restored, after the %s changed" % how)
        S.assert_same_bits(run.prev, base, "%s: the original keeps its own weights" % model)
        got = run.forward(cp)
        assert not torch.equal(got, base), "%s: the %s did not follow its own update" % (model, how)
        S.assert_same_bits(got, run.forward(run.fresh(cp)[0]), "%s: the %s after its own update" % (model, how))


def test_two_modules_that_share_their_parameters():
    model = "small_engine_b1"
    run = Run(model)
    flags, prec, small = S.MODELS[model][:3]
    with torch.device(DEV):
        m2 = MultiView_MPL(**flags)
    for n, child in run.live.named_children():
        setattr(m2, n, child)
    for n, p in run.live.named_parameters(recurse=False):
        setattr(m2, n, p)
    m2.eval().set_matmul_precision(prec).set_small_batch_engine(small)
    assert all(a is b for a, b in zip(m2._param_list(), run.live._param_list()))
    run.also = [m2]
    run.check("first forward")
    S.assert_same_bits(run.forward(m2), run.prev, "the sharing module")
    for name in S.KIND_TARGETS[model]:
        run.update_in_place(name)                                                      # through the first module
        run.check("after %s was updated" % name)
        S.assert_same_bits(run.forward(m2), run.prev, "the sharing module after %s was updated through the other one" % name)


def test_replicas_follow_an_update_of_their_source():
    """DataParallel makes new replicas on every forward: shallow copies with freshly broadcast parameters that share the SOURCE's
    packed operands, keyed on the source's tensors.  Two replicas on one GPU; the source is updated; the next replicas follow."""
    model = "team_rows16_direct"                   # replicas never take the small engine: a model whose engine setting is False
    run = Run(model)
    run.check("first forward of the source")
    for name in S.KIND_TARGETS["small_engine_b1"]:                 # the same flag set: FPT-folded, SPT-folded, read in place
        reps = torch.nn.parallel.replicate(run.live, [run.idx, run.idx])
        assert len(reps) == 2 and all(r._dp_replica for r in reps)
        for i, r in enumerate(reps):
            S.assert_same_bits(run.forward(r), run.prev, "replica %d before %s is updated" % (i, name))
        run.update_in_place(name)                                  # the source, in place
        for i, r in enumerate(torch.nn.parallel.replicate(run.live, [run.idx, run.idx])):
            got = run.forward(r)
            assert not torch.equal(got, run.prev), "replica %d did not follow the update of %s" % (i, name)
            S.assert_same_bits(got, run.forward(run.fresh(run.live)[0]), "replica %d after %s was updated in the source" % (i, name))
        run.check("the source after replicas ran on its operands")


def test_update_on_a_side_stream_ordered_by_an_event():
    model = "small_engine_b1"
    run = Run(model)
    run.check("first forward")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for name in S.KIND_TARGETS[model]:
        torch.cuda.synchronize()
        ev = torch.cuda.Event()
        with torch.cuda.stream(s1):
            run.update_in_place(name)
            ev.record(s1)
        s2.wait_event(ev)
        with torch.cuda.stream(s2):
            live = run.forward(run.live)
        s2.synchronize()
        fresh = run.forward(run.fresh(run.live)[0])
        S.assert_same_bits(live, fresh, "%s updated on one stream, forward on another behind an event" % name)
        assert not torch.equal(live, run.prev) and not cabi.device_error()
        run.prev = live


# ================================================================================================ bindings and finalizers
def test_bindings_and_their_finalizers_go_with_what_they_serve():
    from openmpl_amd import torch_ext
    o = torch_ext.ops()
    gc.collect()
    n0 = o.live_bindings()
    run = Run("small_engine_b1")
    run.check("first forward")
    assert o.live_bindings() == n0 + 1                                   # the fresh modules of check() take the ctypes route
    name = S.KIND_TARGETS["small_engine_b1"][0]
    fins = []
    for i in range(5):                                                   # re-bind five times
        fins.append(run.live._hip_cache[run.idx]["bind_fin"])
        with torch.no_grad():
            run.get(name).mul_(1.01)
        run.forward(run.live)
        assert o.live_bindings() == n0 + 1
    assert not any(f.alive for f in fins), "a released binding left its finalizer pinned to the module"
    assert run.live._hip_cache[run.idx]["bind_fin"].alive
    cp = S.copies_of(run.live)[0][1]
    run.forward(cp)
    assert o.live_bindings() == n0 + 2
    run.live.weights_changed()
    assert o.live_bindings() == n0 + 1 and not run.live._fast_bind
    run.forward(run.live)
    del run, cp
    gc.collect()
    assert o.live_bindings() == n0
