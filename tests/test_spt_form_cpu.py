"""mpl_spt_form, the SPT launch rule both launchers follow (csrc/spt.hip spt_form), against its independent restatement in
tests/spt_stage_cases.py (closed form instead of the library's search), with the compute-unit count given so that no GPU is needed."""
import ctypes as C

import pytest

from openmpl_amd import cabi
from tests.spt_stage_cases import class_ranges, expected_form, lds_cap, tail_batches

SHAPES = [
    # J, d, H, extra flags
    (17, 32, 8, 0), (17, 32, 8, cabi.F_GENERIC_SPT), (15, 32, 8, 0), (64, 64, 8, 0), (17, 2, 2, 0),
]
LDS_CAP = {(17, 32): 5, (15, 32): 5, (64, 64): 1, (17, 2): 64}      # worked out by hand from the layout above


def _form(lib, cfg, B, use_packed, n_cus):
    spw = C.c_int(-1)
    return lib.mpl_spt_form(C.byref(cfg), B, use_packed, n_cus, C.byref(spw)), spw.value


def test_lds_cap_of_the_generic_kernel():
    for (J, d), cap in LDS_CAP.items():
        assert lds_cap(J, d) == cap


@pytest.mark.parametrize("J,d,H,extra", SHAPES, ids=["J%d-d%d-H%d-f%d" % s for s in SHAPES])
@pytest.mark.parametrize("n_cus", [64, 256, 304])
def test_spt_form_matches_the_rule_over_the_grid(n_cus, J, d, H, extra):
    lib = cabi.load()
    generic = (J, d, H) != (17, 32, 8) or bool(extra)
    for V in (1, 3, 4, 31, 32):
        cfg = cabi.Config(J, d, 2, H, V, 2, cabi.F_POS3D_LEARN | extra, 0)
        seen = set()
        prev = None
        b_max = 16 * n_cus // V + 3
        for B in range(1, b_max + 1):
            for use_packed in (0, 1):
                got = _form(lib, cfg, B, use_packed, n_cus)
                assert got == expected_form(J, d, H, extra, V, B, use_packed, n_cus), (V, B, use_packed, got)
                seen.add(got)
            native = _form(lib, cfg, B, 0, n_cus)
            if prev is not None:
                assert native[1] in (prev[1], prev[1] + 1)         # spw grows one class at a time with the batch
                if not generic and (prev[1], native[1]) == (8, 9):                # the kernel id switches at 8 -> 9, nowhere else
                    assert (prev[0], native[0]) == (cabi.SPT_STAGED, cabi.SPT_FRAGS)
                elif not generic:
                    assert prev[0] == native[0]
            prev = native
        if generic:
            # capped by LDS: every class up to the cap (or to what b_max reaches) is visited, none beyond, whatever use_packed says
            top = min(LDS_CAP[(J, d)], -(-b_max // (n_cus // V)))
            assert seen == {(cabi.SPT_ANY, c) for c in range(1, top + 1)}, (V, seen)
        else:
            assert {s for s in seen if s[0] == cabi.SPT_STAGED} == {(cabi.SPT_STAGED, c) for c in range(1, 9)}
            assert {s for s in seen if s[0] == cabi.SPT_FRAGS} == {(cabi.SPT_FRAGS, c) for c in range(9, 17)}
            assert {s for s in seen if s[0] == cabi.SPT_PACKED} == {(cabi.SPT_PACKED, c) for c in (1, 2, 4, 8, 16)}   # next power of two


def test_spt_form_refuses_bad_arguments_without_a_device():
    lib = cabi.load()
    cfg = cabi.Config(17, 32, 2, 8, 3, 2, cabi.F_POS3D_LEARN, 0)
    spw = C.c_int(-1)
    assert lib.mpl_spt_form(None, 8, 1, 256, C.byref(spw)) == -1 and spw.value == -1
    assert lib.mpl_spt_form(C.byref(cfg), 0, 1, 256, C.byref(spw)) == -1
    assert lib.mpl_spt_form(C.byref(cfg), -3, 1, 256, C.byref(spw)) == -1
    assert lib.mpl_spt_form(C.byref(cfg), 8, 1, 256, None) == cabi.SPT_PACKED          # the count is optional
    bad = cabi.Config(65, 32, 2, 8, 3, 2, cabi.F_POS3D_LEARN, 0)
    assert lib.mpl_spt_form(C.byref(bad), 8, 0, 256, C.byref(spw)) == -2
    bad = cabi.Config(17, 32, 2, 8, 33, 2, cabi.F_POS3D_LEARN, 0)
    assert lib.mpl_spt_form(C.byref(bad), 8, 0, 256, C.byref(spw)) < 0
    assert spw.value == -1


def test_batch_selection_reaches_every_class_with_all_tails_on_a_256_cu_device():
    """The batch selection of tests/test_spt_stage_gpu.py, fed from the library's rule at 256 compute units: at V = 3 class c is
    85 (c - 1) < B <= 85 c, every class exists below B = 1300 and holds all three tails."""
    lib = cabi.load()
    cfg = cabi.Config(17, 32, 2, 8, 3, 2, cabi.F_POS3D_LEARN, 0)
    for use_packed in (0, 1):
        ranges = class_ranges(lambda B: _form(lib, cfg, B, use_packed, 256))
        if not use_packed:
            assert all(ranges[(cabi.SPT_STAGED if c <= 8 else cabi.SPT_FRAGS, c)][0] == 85 * (c - 1) + 1 for c in range(1, 17))
            assert all(ranges[(cabi.SPT_STAGED if c <= 8 else cabi.SPT_FRAGS, c)][1] == 85 * c for c in range(1, 16))
        for (kind, spw), (lo, hi) in ranges.items():
            assert hi < 1400
            got = tail_batches(lo, hi, spw)
            assert all(lo <= B <= hi for B in got)
            if spw > 2:
                assert sorted(B % spw for B in got) == [0, 1, spw - 1], (kind, spw, got)
    assert tail_batches(1, 85, 1) == [1, 85] and tail_batches(86, 170, 2) == [86, 87]
