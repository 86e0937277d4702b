"""The checker of the block-stack stage check (tests/block_stack_cases.py) can fail: on the CPU, at D = 544 and M <= 64 rows, it
accepts the float32 oracle and rejects ten constructed mistakes applied to the float64 result -- each the kind of error a kernel of
the stack could make in one slice, head, sequence or tile.  A mistake the row-wise bound let through would mean that the inputs or
the measure are too weak."""
import pytest
import torch

from oracle import mpl_oracle
from tests import block_stack_cases as bs

D, H, N_TOK, N_SEQ = 544, 8, 4, 15          # 60 rows: a ragged 64-row tile, 15 sequences
SCHED = bs.REFERENCE_SCHEDULE

_case = {}


def _the_case():
    if not _case:
        _, sd = bs.make_stack(D, 2)
        x = bs.make_rows(N_SEQ * N_TOK, D)
        ref64, e32, ref32 = bs.references(sd, x, N_TOK, H, SCHED)
        _case.update(sd=sd, x=x, ref64=ref64, e32=e32, ref32=ref32)
        print("D %d H %d n_tok %d M %d schedule %s: e32 max-scaled %.3e norm-wise %.3e" % (D, H, N_TOK, x.shape[0], SCHED, e32[0], e32[1]))
    return _case


def test_inputs_tell_rows_sequences_and_tiles_apart():
    bs.assert_rows_tell_apart(sorted(set(bs.TEAM_NTOK + bs.BF16_NTOK + bs.SMALL_NTOK + (6, 14, 15))))
    x = bs.make_rows(64, D)
    assert torch.equal(x[:20], bs.make_rows(20, D)), "the first rows of a longer input are not the shorter input"
    amax = x.abs().amax(1)
    assert float(amax.max() / amax.min()) > 2.0 ** 10                      # scales over 2^-6 .. 2^6
    ratio = amax[1:] / amax[:-1]
    assert bool(((ratio > 4) | (ratio < 0.25)).all())                      # neighbours are 2^5 or 2^-8 apart
    mean = (x.double().mean(1) / x.double().std(1))
    assert float(mean.max()) > 0.5 and float(mean.min()) < -0.5            # mean offsets in units of the row's sigma


def test_the_restated_block_is_the_oracle_block():
    c = _the_case()
    assert torch.equal(bs.mutant_stack(c["sd"], c["x"], N_TOK, H, SCHED, None), c["ref64"])


def test_checker_accepts_the_float32_oracle_and_the_reference():
    c = _the_case()
    assert 1e-8 < c["e32"][0] < 1e-5 and 1e-8 < c["e32"][1] < 1e-5, c["e32"]      # float32 round-off, not zero and not garbage
    assert bs.check_rows(c["ref32"], c["ref64"], c["e32"]) is None
    assert bs.check_rows(c["ref64"].float(), c["ref64"], c["e32"]) is None
    # rows are independent of the batch they come in: the stack of the first sequences alone is the slice
    part = bs.reference(c["sd"], c["x"][:5 * N_TOK], N_TOK, H, SCHED)
    assert bs.check_rows(part, c["ref64"][:5 * N_TOK], c["e32"]) is None


def test_checker_rejects_non_finite_rows():
    c = _the_case()
    bad = c["ref64"].float().clone()
    bad[7, 100] = float("nan")
    assert "non-finite" in bs.check_rows(bad, c["ref64"], c["e32"])


def test_row_measures_are_those_of_rel_errors_per_row():
    c = _the_case()
    mx, nw = bs.row_errors(c["ref32"], c["ref64"])
    for r in (0, 17, 59):
        a, b = mpl_oracle.rel_errors(c["ref32"][r:r + 1], c["ref64"][r:r + 1])
        assert abs(float(mx[r]) - a) <= 1e-12 * a and abs(float(nw[r]) - b) <= 1e-12 * b


@pytest.mark.parametrize("mistake", bs.MISTAKES)
def test_checker_rejects_a_constructed_mistake(mistake):
    c = _the_case()
    wrong = bs.mutant_stack(c["sd"], c["x"], N_TOK, H, SCHED, mistake)
    msg = bs.check_rows(wrong, c["ref64"], c["e32"])
    mx, nw = bs.worst_row_errors(wrong, c["ref64"])
    whole = mpl_oracle.rel_errors(wrong, c["ref64"])
    print("%s: worst row %.3e / %.3e (whole tensor: %.3e / %.3e), bound %d x (%.3e, %.3e)"
          % (mistake, mx, nw, whole[0], whole[1], bs.FACTOR, c["e32"][0], c["e32"][1]))
    assert msg is not None, "%s passes the row-wise bound" % mistake
    # an order of magnitude outside it, too: no mistake is a borderline case of the bound
    assert mx > 10 * bs.FACTOR * c["e32"][0] and nw > 10 * bs.FACTOR * c["e32"][1], (mistake, mx, nw)


def test_small_engine_layout_restated():
    """The restated group layout at the shapes the documentation names (256 compute units)."""
    assert bs.small_groups(1, 2, 544, 256) == (1, 1)
    assert bs.small_groups(8, 4, 544, 256) == (2, 4)               # two groups of 16 rows
    assert bs.small_groups(3, 12, 544, 256)[0] == 3                # 36 rows: three groups, two column tiles per workgroup
    assert bs.small_groups(20, 4, 544, 256) == (5, 4)              # 80 rows: five groups of 51 workgroups
    assert bs.small_groups(48, 2, 544, 256)[0] == 0                # six groups do not fit
    assert bs.small_groups(3, 16, 1088, 256)[0] == 0               # no two-tile layout beyond D = 544
