"""Guarded allocations for the memory contract of the entry points: where a call writes, and what it reads
that it was never given.

Every wrapper of the package takes its outputs and workspaces from ``torch.empty`` / ``torch.empty_like``, and the caching
allocator rounds every block up, so a write one row behind an output lands in slack that nothing looks at.  ``Guarded`` is a
context manager under which those two functions hand out, for tensors of the guarded device, a view into the middle of a larger
allocation of its own:

* a guard in front of the payload and one behind it, each at least as large as the payload and at least 64 KiB;
* the payload starts on a 256-byte boundary (no alignment the caching allocator gives today is taken away);
* guards and payload are prefilled with one repeating 8-byte word.  ``PATTERN`` = 0xFFF5A5A5FFF5A5A5 is a NaN as float64, as
  float32 and as the upper 16-bit half of every 32-bit word (fp16 and bf16), int32 -678491, bytes 0xA5 / 0xF5 / 0xFF: outside
  the value range of every integer, byte and bool output of the library (`best` is legitimately -1, so the single byte 0xFF would
  not do).  ``ZEROS`` is the second prefill of the tests: a result that differs between the two was read before it was written;
* a request for zero elements is served like any other;
* the allocations are kept until the context is dropped: nothing goes back to the caching allocator in between.

``guarded_copy`` places an input the same way, between guards of NaN or of 1e30; the context wraps ``cabi.launch`` and
keeps the integer arguments of every call, so that a test can assert that the tensors it guards are the ones the kernels were
handed (``assert_launched``): a wrapper that silently copied a tensor fails that check instead of testing nothing.  ``check()``
synchronises and reports per allocation whether both guards are intact and how many payload elements still hold the prefill.

The harness owns every byte it inspects.  Nothing here writes or reads outside an allocation.
"""
from __future__ import annotations

import contextlib
import ctypes
from typing import List, Optional

import numpy as np
import torch

PATTERN = 0xFFF5A5A5FFF5A5A5
ZEROS = 0
MIN_GUARD = 64 * 1024
ALIGN = 256

_real_empty = torch.empty
_real_empty_like = torch.empty_like


def _signed(word: int) -> int:
    return word - (1 << 64) if word >= 1 << 63 else word


def _round_up(n: int, a: int) -> int:
    return (n + a - 1) // a * a


class Allocation:
    """one payload between its two guards: `base` is the whole allocation (int64 words), `start` the payload's byte offset"""

    def __init__(self, shape, dtype, device, word, kind="empty", surround=None):
        self.shape, self.dtype, self.kind = tuple(int(s) for s in shape), dtype, kind
        self.itemsize = _real_empty(0, dtype=dtype).element_size()
        self.numel = int(np.prod(self.shape, dtype=np.int64)) if self.shape else 1
        self.nbytes = self.numel * self.itemsize
        self.guard = max(_round_up(self.nbytes, ALIGN), MIN_GUARD)
        total = 2 * self.guard + _round_up(self.nbytes, ALIGN) + ALIGN
        self.base = _real_empty(total // 8, dtype=torch.int64, device=device)
        self.word, self.surround = word, surround
        if surround is None:
            self.base.fill_(_signed(word))
        else:                                            # an input: the guards hold `surround` in the input's own dtype
            self.base.view(dtype).fill_(surround)
        p = self.base.data_ptr()
        self.start = _round_up(p + self.guard, ALIGN) - p
        assert self.start >= self.guard and total - self.start - self.nbytes >= self.guard
        self.bytes = self.base.view(torch.uint8)
        self.view = self.bytes[self.start:self.start + self.nbytes].view(dtype).view(self.shape)
        assert self.nbytes == 0 or (self.view.data_ptr() % ALIGN == 0 and self.view.data_ptr() == p + self.start)
        self.original = None                             # an input's bits

    @property
    def ptr(self) -> int:
        return self.base.data_ptr() + self.start

    def holds(self, t: torch.Tensor) -> bool:
        """t is the payload or a view into it (an empty tensor at the payload's address counts)"""
        q, n = t.data_ptr(), t.numel() * t.element_size()
        if t.device != self.base.device:
            return False
        if self.nbytes == 0 or n == 0:                   # a tensor without elements has no address to go by
            return n == 0 == self.nbytes and t.dtype == self.dtype and tuple(t.shape) == self.shape
        return self.ptr <= q and q + n <= self.ptr + self.nbytes

    def _pristine(self):
        ref = _real_empty_like(self.base)
        if self.surround is None:
            ref.fill_(_signed(self.word))
        else:
            ref.view(self.dtype).fill_(self.surround)
        return ref.view(torch.uint8)

    def report(self) -> "Report":
        ref = self._pristine()
        end = self.start + self.nbytes
        front = bool(torch.equal(self.bytes[:self.start], ref[:self.start]))
        back = bool(torch.equal(self.bytes[end:], ref[end:]))
        unwritten = None
        if self.surround is None:
            same = (self.bytes[self.start:end] == ref[self.start:end]).view(self.numel, self.itemsize).all(dim=1) if self.numel else None
            unwritten = int(same.sum()) if self.numel else 0
        kept = None if self.original is None else bool(torch.equal(self.bytes[self.start:end].cpu(), self.original))
        return Report(self, front, back, unwritten, kept)


class Report:
    def __init__(self, alloc, front, back, unwritten, kept):
        self.alloc, self.front_intact, self.back_intact, self.unwritten, self.input_kept = alloc, front, back, unwritten, kept

    @property
    def guards_intact(self) -> bool:
        return self.front_intact and self.back_intact

    def __repr__(self):
        a = self.alloc
        return "<%s %s %s at +%d: front %s, back %s, unwritten %s%s>" % (
            a.kind, a.shape, str(a.dtype).replace("torch.", ""), a.start, "intact" if self.front_intact else "HIT",
            "intact" if self.back_intact else "HIT", self.unwritten, "" if self.input_kept is None else ", input kept %s" % self.input_kept)


def _size_of(args, kwargs):
    if "size" in kwargs:
        return kwargs.pop("size")
    if len(args) == 1 and not isinstance(args[0], (int, np.integer)) and not (isinstance(args[0], torch.Tensor) and args[0].ndim == 0):
        return tuple(args[0])
    return tuple(args)


class Guarded(contextlib.AbstractContextManager):
    """with Guarded(device, prefill) as g: ... ; g.check() -- see the module's docstring.  `device`: what to guard, "cuda" (every
    GPU tensor) or, for the self-test of the harness, "cpu".  `launcher`: the object whose ``launch`` is recorded (default: the
    package's cabi, when the device is a GPU)."""

    def __init__(self, device="cuda", prefill: int = PATTERN, launcher=None, record=()):
        self.device_type = torch.device(device).type
        self.prefill = prefill
        self.allocations: List[Allocation] = []
        self.inputs: List[Allocation] = []
        self.launch_ints = set()
        self.launches: List[str] = []
        self._launcher = launcher
        self._record = tuple(record)       # (owner, attribute): further callables whose arguments are recorded (the ctypes functions
        self._saved = None                 # the forward calls directly, structs passed by reference included)
        self._wrapped = []

    # -- the two patched functions ---------------------------------------------------------------------------------------------
    def _wants(self, device, pin=False) -> bool:
        dev = torch.device("cpu") if device is None else torch.device(device)
        return dev.type == self.device_type and not pin

    def _empty(self, *args, **kwargs):
        if not self._wants(kwargs.get("device"), kwargs.get("pin_memory", False)) or kwargs.get("out") is not None \
                or kwargs.get("layout", torch.strided) is not torch.strided:
            return _real_empty(*args, **kwargs)
        kw = dict(kwargs)
        size = _size_of(args, kw)
        dtype = kw.pop("dtype", None) or torch.get_default_dtype()
        device = torch.device("cpu") if kw.pop("device", None) is None else torch.device(kwargs["device"])
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        a = Allocation(size, dtype, device, self.prefill)
        self.allocations.append(a)
        return a.view.requires_grad_(True) if kw.get("requires_grad") else a.view

    def _empty_like(self, t, **kwargs):
        # contiguous whatever the strides of `t`: the wrappers of the package only ever ask for the like of a contiguous tensor
        device = kwargs.get("device", t.device)
        if not self._wants(device, kwargs.get("pin_memory", False)):
            return _real_empty_like(t, **kwargs)
        a = Allocation(t.shape, kwargs.get("dtype") or t.dtype, torch.device(device), self.prefill, kind="empty_like")
        self.allocations.append(a)
        return a.view

    def __enter__(self):
        launcher = self._launcher
        if launcher is None and self.device_type == "cuda":
            from openmpl_amd import cabi as launcher
        self._saved = (torch.empty, torch.empty_like, launcher, None if launcher is None else launcher.launch)
        torch.empty, torch.empty_like = self._empty, self._empty_like
        if launcher is not None:
            inner = launcher.launch

            def launch(name, device, *args):
                self.launches.append(name)
                for v in args:
                    self._note(v)
                return inner(name, device, *args)
            launcher.launch = launch
        for owner, name in self._record:
            self._wrapped.append((owner, name, getattr(owner, name)))
            setattr(owner, name, self._recording(name, getattr(owner, name)))
        return self

    def _recording(self, name, inner):
        def call(*args):
            self.launches.append(name)
            for v in args:
                self._note(v)
            return inner(*args)
        return call

    def __exit__(self, *exc):
        torch.empty, torch.empty_like, launcher, launch = self._saved
        if launcher is not None:
            launcher.launch = launch
        for owner, name, inner in self._wrapped:
            setattr(owner, name, inner)
        self._wrapped = []
        return False

    def _note(self, v):
        if isinstance(v, bool) or v is None:
            return
        if isinstance(v, (int, np.integer)):
            self.launch_ints.add(int(v))
        elif isinstance(v, ctypes.Array):
            for x in v:
                self._note(x)
        elif isinstance(v, ctypes._SimpleCData):
            self._note(v.value)
        elif isinstance(v, ctypes.Structure):
            for field in v._fields_:
                self._note(getattr(v, field[0]))
        elif hasattr(v, "_obj"):                         # ctypes.byref(struct)
            self._note(v._obj)

    # -- inputs ------------------------------------------------------------------------------------------------------------------
    def guarded_copy(self, array, surround=float("nan"), device=None) -> torch.Tensor:
        """`array` (a tensor or a numpy array) placed like an output, between guards filled with `surround` in its own dtype"""
        # np.array copies: the cached cases of the case modules are read-only
        src = array.detach().cpu().contiguous() if isinstance(array, torch.Tensor) else torch.from_numpy(np.array(array))
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if self.device_type == "cuda" else torch.device("cpu")
        if not (src.dtype.is_floating_point):
            surround = -678491 if src.dtype in (torch.int32, torch.int64) else 1
        elif src.dtype == torch.float16 and abs(surround) > 6e4:
            surround = 6e4 if surround > 0 else -6e4     # the largest round figure a half holds
        a = Allocation(src.shape, src.dtype, torch.device(device), self.prefill, kind="input", surround=surround)
        a.view.copy_(src)
        a.original = src.reshape(-1).view(torch.uint8).clone() if src.numel() else _real_empty(0, dtype=torch.uint8)
        self.inputs.append(a)
        return a.view

    def refill_input_guards(self, surround):
        """the guards of every input so far refilled with `surround` (NaN, 1e30) in the input's dtype; the payloads stay"""
        for a in self.inputs:
            if not a.dtype.is_floating_point:
                continue
            keep = a.view.clone()
            a.surround = 6e4 if (a.dtype == torch.float16 and surround > 6e4) else surround
            a.base.view(a.dtype).fill_(a.surround)
            a.view.copy_(keep)

    # -- the questions a test asks ---------------------------------------------------------------------------------------------
    def allocation_of(self, t: torch.Tensor) -> Optional[Allocation]:
        for a in self.allocations + self.inputs:
            if a.holds(t):
                return a
        return None

    def assert_launched(self, tensors):
        """the data_ptr() of every tensor is among the integers some launch was handed: the kernels saw this memory, not a copy"""
        for t in tensors:
            assert self.allocation_of(t) is not None, "a tensor of shape %s is not guarded" % (tuple(t.shape),)
            assert t.data_ptr() in self.launch_ints, "a guarded tensor of shape %s, %s never reached a launch (%s): it was copied" % (
                tuple(t.shape), t.dtype, ", ".join(self.launches) or "none was made")

    def check(self) -> List[Report]:
        """synchronise, then one Report per allocation, outputs and workspaces first, then the inputs"""
        if self.device_type == "cuda":
            torch.cuda.synchronize()
        return [a.report() for a in self.allocations + self.inputs]

    def assert_guards_intact(self, reports=None):
        reports = self.check() if reports is None else reports
        bad = [r for r in reports if not r.guards_intact]
        assert not bad, "written outside an allocation: %s" % bad
        return reports

    def assert_inputs_kept(self, reports=None):
        reports = self.check() if reports is None else reports
        bad = [r for r in reports if r.input_kept is False]
        assert not bad, "an input changed its bits: %s" % bad

    def assert_written(self, tensors, reports=None):
        """every element of the allocation behind each tensor was written (read under PATTERN only: zeros are legitimate values)"""
        assert self.prefill == PATTERN
        reports = self.check() if reports is None else reports
        by_alloc = {id(r.alloc): r for r in reports}
        for t in tensors:
            a = self.allocation_of(t)
            assert a is not None and a.kind != "input", "a returned tensor of shape %s is not a guarded output" % (tuple(t.shape),)
            r = by_alloc[id(a)]
            assert r.unwritten == 0, "%d of %d elements were left unwritten: %r" % (r.unwritten, a.numel, r)

    def guarded_bytes(self):
        return len(self.allocations), sum(a.nbytes for a in self.allocations)


def tensors_of(result) -> List[torch.Tensor]:
    """every tensor of a result: a tensor, None, or any nesting of tuples, lists, NamedTuples and dicts"""
    if result is None:
        return []
    if isinstance(result, torch.Tensor):
        return [result]
    if isinstance(result, dict):
        return [t for k in result for t in tensors_of(result[k])]
    if isinstance(result, (list, tuple)):
        return [t for x in result for t in tensors_of(x)]
    raise TypeError("no tensors in a %s" % type(result).__name__)


def tensors_in(obj) -> List[torch.Tensor]:
    """the tensors among the arguments of a call; whatever else it holds is passed over"""
    if isinstance(obj, torch.Tensor):
        return [obj]
    if isinstance(obj, dict):
        return [t for v in obj.values() for t in tensors_in(v)]
    if isinstance(obj, (list, tuple)):
        return [t for v in obj for t in tensors_in(v)]
    return []


def bits(result) -> List[torch.Tensor]:
    """the tensors of a result as host bytes, for bitwise comparison (NaN payloads included)"""
    return [t.detach().contiguous().cpu().reshape(-1).view(torch.uint8) for t in tensors_of(result)]


def assert_same_bits(a, b, what):
    x, y = bits(a), bits(b)
    assert len(x) == len(y), "%s: %d tensors against %d" % (what, len(x), len(y))
    for i, (p, q) in enumerate(zip(x, y)):
        assert p.shape == q.shape and torch.equal(p, q), "%s: tensor %d of the result differs in %d bytes" % (
            what, i, int((p != q).sum()) if p.shape == q.shape else -1)


# ---- the contract itself: one procedure for the self-test on the CPU and for every entry point on the GPU ----------------------

def place(g: Guarded, obj, surround):
    """the tensors and numpy arrays of `obj` (any nesting of lists, tuples and dicts) as guarded copies; everything else as it is"""
    if isinstance(obj, (torch.Tensor, np.ndarray)):
        return g.guarded_copy(obj, surround)
    if isinstance(obj, dict):
        return {k: place(g, v, surround) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)) and any(isinstance(x, (torch.Tensor, np.ndarray, list, tuple, dict)) for x in obj):
        return type(obj)(place(g, v, surround) for v in obj) if not hasattr(obj, "_fields") else type(obj)(*(place(g, v, surround) for v in obj))
    return obj


def plain(obj, device):
    """the same arguments as ordinary tensors of `device`"""
    if isinstance(obj, (torch.Tensor, np.ndarray)):
        return (obj if isinstance(obj, torch.Tensor) else torch.from_numpy(np.array(obj))).to(device)
    if isinstance(obj, dict):
        return {k: plain(v, device) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)) and any(isinstance(x, (torch.Tensor, np.ndarray, list, tuple, dict)) for x in obj):
        return type(obj)(plain(v, device) for v in obj)
    return obj


RUNS = (("pattern", PATTERN, float("nan")), ("zeros", ZEROS, float("nan")), ("pattern, 1e30 around the inputs", PATTERN, 1e30))


def run_contract(call, kwargs, device="cuda", launcher=None, exempt=None, workspace_bytes=(), min_outputs=1, unlaunched=(), record=(),
                 after=None):
    """The memory contract of one call, `call(**kwargs)`, the tensors of `kwargs` on the host:

    1. every guard of every allocation made during the call is intact;
    2. every element of every returned tensor was written (`exempt`: {index into tensors_of(result): the sentence that grants it});
    3. the result has the same bits under PATTERN and under ZEROS: nothing is read before it is written;
    4. and the same bits with NaN and with 1e30 around the inputs, whose own bits stay: nothing is read outside an input;
    5. those bits are the ones of the plain call;
    and the tensors handed in and out are the ones the launches saw.  `workspace_bytes`: sizes that must be among the guarded
    uint8 allocations; `min_outputs`: how many returned tensors must be guarded allocations; `unlaunched`: names in `kwargs` whose
    tensors the wrapper is documented to transform before the launch; `record`: Guarded's; `after(g, result)`: further assertions
    of the caller on a guarded run.  -> (result of the plain call, allocations, bytes)."""
    exempt = exempt or {}
    seen, stats = [], None
    for what, prefill, surround in RUNS:
        with Guarded(device, prefill, launcher, record) as g:
            args = place(g, kwargs, surround)
            result = call(**args)
            reports = g.check()
        if after is not None:
            after(g, result)
        g.assert_guards_intact(reports)
        g.assert_inputs_kept(reports)
        outs = tensors_of(result)
        guarded = [(i, t) for i, t in enumerate(outs) if any(a.holds(t) for a in g.allocations)]
        assert len(guarded) >= min_outputs, "%s: %d of the %d returned tensors are guarded allocations, expected at least %d" % (
            what, len(guarded), len(outs), min_outputs)
        assert len(g.allocations) >= 1 and g.launches, "%s: the call reached no guarded allocation or made no launch" % what
        sizes = [a.nbytes for a in g.allocations if a.dtype == torch.uint8]
        for need in workspace_bytes:
            assert need in sizes, "%s: no guarded workspace of %d bytes (uint8 allocations: %s)" % (what, need, sizes)
        handed = [t for k, v in args.items() if k not in unlaunched for t in tensors_in(v)]
        for t in handed + [t for _, t in guarded]:
            a = g.allocation_of(t)
            assert a is not None and a.ptr in g.launch_ints, "%s: a guarded %s of shape %s never reached a launch (%s): it was copied" % (
                what, a.kind if a else "tensor", tuple(t.shape), ", ".join(g.launches))
        if prefill == PATTERN:
            g.assert_written([t for i, t in guarded if i not in exempt], reports)
        seen.append((what, [b.clone() for b in bits(result)]))
        if stats is None:
            stats = g.guarded_bytes()
        del result, args
    for what, b in seen[1:]:
        assert len(b) == len(seen[0][1])
        for i, (p, q) in enumerate(zip(seen[0][1], b)):
            assert p.shape == q.shape and torch.equal(p, q), "tensor %d of the result differs between prefill '%s' and '%s' in %d bytes" % (
                i, seen[0][0], what, int((p != q).sum()) if p.shape == q.shape else -1)
    dev = torch.device("cuda", torch.cuda.current_device()) if torch.device(device).type == "cuda" else torch.device("cpu")
    reference = call(**plain(kwargs, dev))
    for i, (p, q) in enumerate(zip(seen[0][1], bits(reference))):
        assert p.shape == q.shape and torch.equal(p, q), "tensor %d of the guarded result differs from the plain call in %d bytes" % (
            i, int((p != q).sum()) if p.shape == q.shape else -1)
    if dev.type == "cuda":
        from openmpl_amd import cabi
        torch.cuda.synchronize()
        assert not cabi.device_error(dev.index), "the device-error word is set"
    return reference, stats[0], stats[1]
