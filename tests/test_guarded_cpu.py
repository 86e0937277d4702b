"""The guarded-allocation harness (tests/guarded.py) on CPU tensors with small fake "kernels": it accepts a correct one and rejects
each constructed mistake, so that a green tests/test_memory_contract_gpu.py means something.  The fakes go through the same
`run_contract` as the entry points on the GPU; they reach outside their tensors only into memory the harness owns (its guards)."""
import numpy as np
import pytest
import torch

from tests import guarded as G


class FakeLib:
    """stands where openmpl_amd.cabi stands on the GPU: launch(name, device, *args) with tensors passed as addresses"""

    def __init__(self):
        self.reg = {}

    def tensor(self, p):
        return self.reg[p]

    def launch(self, name, device, x_ptr, out_ptr, best_ptr, ws_ptr, n, mistake, far):
        x, out, best, ws = self.tensor(x_ptr), self.tensor(out_ptr).view(-1), self.tensor(best_ptr), self.tensor(ws_ptr)
        xf = x.view(-1)
        at = lambda t, i: t.as_strided((1,), (1,), t.storage_offset() + i)      # element i of t's storage, counted from t
        if mistake == "accumulates":
            out += 2 * xf                                # reads the output before writing it
        elif mistake == "one unwritten":
            out[:n - 1].copy_(2 * xf[:n - 1])
        else:
            out.copy_(2 * xf)
        if mistake == "one behind":
            at(out, n).fill_(7.0)
        if mistake == "one before":
            at(out, -1).fill_(7.0)
        if mistake == "far behind":
            at(out, n + far - 1).fill_(7.0)
        if mistake == "reads behind the input":
            at(out, n - 1).add_(1e-30 * at(xf, n))
        if mistake == "reads its workspace":
            out += (ws[:1] != 0).to(out.dtype)           # a counter that was never set to zero
        ws[:2] = 5                                       # a workspace is written in part only, and that is no finding
        if mistake != "best unwritten":
            best.fill_(-1)                               # -1 is a legitimate value of `best`


def double(lib, x, mistake=None):
    """the fake entry point: out = 2 x, best = -1"""
    if mistake == "copies its input":
        x = x.clone()
    out = torch.empty(x.shape, dtype=torch.float32)
    best = torch.empty((3,), dtype=torch.int32, device="cpu")
    empty = torch.empty((0, 5), dtype=torch.float64)
    assert empty.shape == (0, 5) and empty.dtype == torch.float64
    ws = torch.empty(16, dtype=torch.uint8)
    for t in (x, out, best, ws):
        lib.reg[t.data_ptr()] = t
    far = max(-(-out.numel() * 4 // G.ALIGN) * G.ALIGN, G.MIN_GUARD) // 4      # the guard, in elements: "far behind" is its last one
    lib.launch("double", "cpu", x.data_ptr(), out.data_ptr(), best.data_ptr(), ws.data_ptr(), x.numel(), mistake, far)
    return out, best


def contract(mistake, n=37):
    lib = FakeLib()
    x = np.arange(1, n + 1, dtype=np.float32).reshape(1, n)
    return G.run_contract(lambda x: double(lib, x, mistake), dict(x=x), device="cpu", launcher=lib, min_outputs=2, workspace_bytes=(16,))


def test_a_correct_fake_passes_and_reports_what_was_guarded():
    (out, best), n_alloc, n_bytes = contract(None)
    assert torch.equal(out, 2 * torch.arange(1, 38, dtype=torch.float32).reshape(1, 37)) and best.tolist() == [-1, -1, -1]
    assert n_alloc == 4 and n_bytes == 37 * 4 + 3 * 4 + 16      # out, best, the request for zero elements, the workspace


def test_the_allocations_are_what_the_contract_asks_for():
    with G.Guarded("cpu", G.PATTERN) as g:
        a = torch.empty(5, 7, dtype=torch.float32)
        b = torch.empty((100000,), dtype=torch.float64)
        c = torch.empty_like(a, dtype=torch.int32)
        h = torch.empty(6, dtype=torch.float16)
        z = torch.empty(0)
        i = g.guarded_copy(np.ones((2, 3), np.float32), 1e30)
        assert torch.equal(i, torch.ones(2, 3))
        behind = i.as_strided((1,), (1,), i.storage_offset() + 6)        # the harness's own guard word behind the input
        assert float(behind) == np.float32(1e30)
        g.refill_input_guards(float("nan"))
        assert torch.isnan(behind).all() and torch.equal(i, torch.ones(2, 3)) and all(r.guards_intact for r in g.check())
    assert torch.empty is G._real_empty and torch.empty_like is G._real_empty_like
    assert len(g.allocations) == 5 and z.numel() == 0
    for t in (a, b, c, h, i):
        al = g.allocation_of(t)
        assert t.data_ptr() % 256 == 0 and t.is_contiguous()
        assert al.guard >= max(al.nbytes, 64 * 1024) and al.start >= al.guard
        assert al.base.numel() * 8 - al.start - al.nbytes >= al.guard
    # the pattern: NaN as float64, float32 and as the upper half-word; -678491 as int32; never 0xFF alone
    assert torch.isnan(a).all() and torch.isnan(b).all() and (c == -678491).all()
    assert torch.isnan(h[1::2]).all() and torch.isnan(h.view(torch.bfloat16)[1::2]).all()
    assert sorted(set(a.view(torch.uint8).reshape(-1).tolist())) == [0xA5, 0xF5, 0xFF]
    rep = g.check()
    assert all(r.guards_intact for r in rep) and [r.unwritten for r in rep[:5]] == [35, 100000, 35, 6, 0]
    with G.Guarded("cpu", G.ZEROS) as g0:
        assert (torch.empty(9, dtype=torch.int32) == 0).all()
        cuda_like = torch.empty(3, device="meta")         # another device passes through
    assert len(g0.allocations) == 1 and cuda_like.device.type == "meta"


@pytest.mark.parametrize("mistake,complaint", [
    ("one behind", "written outside an allocation"),
    ("one before", "written outside an allocation"),
    ("far behind", "written outside an allocation"),
    ("one unwritten", "1 of 37 elements were left unwritten"),
    ("best unwritten", "3 of 3 elements were left unwritten"),
    ("accumulates", "37 of 37 elements were left unwritten"),      # NaN + x keeps the payload of the NaN it found
    ("reads its workspace", "differs between prefill 'pattern' and 'zeros'"),
    ("reads behind the input", "differs between prefill 'pattern' and 'pattern, 1e30 around the inputs'"),
    ("copies its input", "never reached a launch"),
])
def test_each_constructed_mistake_is_rejected(mistake, complaint):
    with pytest.raises(AssertionError, match=complaint):
        contract(mistake)


def test_an_input_that_changes_its_bits_is_rejected():
    lib = FakeLib()

    def clobber(x):
        out = double(lib, x)
        x.view(-1)[3] = 0.0
        return out
    with pytest.raises(AssertionError, match="an input changed its bits"):
        G.run_contract(clobber, dict(x=np.ones((1, 37), np.float32)), device="cpu", launcher=lib, min_outputs=2, workspace_bytes=(16,))


def test_a_missing_workspace_and_an_unguarded_result_are_rejected():
    """a later change of allocator must not hollow the GPU tests out: the expected workspace has to be among the guarded
    allocations, and the returned tensors have to be guarded ones"""
    lib = FakeLib()
    args = dict(x=np.ones((1, 37), np.float32))
    with pytest.raises(AssertionError, match="no guarded workspace of 17 bytes"):
        G.run_contract(lambda x: double(lib, x), args, device="cpu", launcher=lib, workspace_bytes=(17,))
    with pytest.raises(AssertionError, match="2 of the 3 returned tensors are guarded allocations"):
        G.run_contract(lambda x: double(lib, x) + (torch.zeros(3),), args, device="cpu", launcher=lib, min_outputs=3)


def test_structs_passed_by_reference_are_recorded():
    """the forward hands its inputs over inside a struct passed by reference, not through cabi.launch"""
    import ctypes as C

    class Inputs(C.Structure):
        _fields_ = [("batch", C.c_int32), ("poses", C.c_void_p * 3)]

    class Lib:
        def forward(self, inp, out, stream):
            return 0
    lib = Lib()
    with G.Guarded("cpu", record=[(lib, "forward")]) as g:
        a, b = g.guarded_copy(np.zeros(4, np.float32)), g.guarded_copy(np.zeros(4, np.float32))
        out = torch.empty(4)
        inp = Inputs(2, (C.c_void_p * 3)(a.data_ptr(), b.data_ptr(), None))
        assert lib.forward(C.byref(inp), out.data_ptr(), None) == 0
    assert g.launches == ["forward"] and lib.forward(None, 0, None) == 0 and g.launches == ["forward"]     # the wrapper is gone again
    g.assert_launched([a, b, out])
    with pytest.raises(AssertionError, match="never reached a launch"):
        g.assert_launched([g.guarded_copy(np.zeros(4, np.float32))])
