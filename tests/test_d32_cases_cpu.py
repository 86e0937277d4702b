"""The checker of the D = 32 stage check (tests/d32_stage_cases.py, tests/test_d32_stage_gpu.py) can fail, shown without a GPU: at
D = 32 it accepts the float32 oracle on every block-level case of the GPU file and rejects every constructed mistake -- each the
kind of error d32_qkv_kernel, the long attention kernels, d32_mlp_kernel or spt_pack_kernel could make in one tile, head, key,
column tile or k step -- by a factor of 4 or more beyond the bound, under the project's rule 4 x e32 and under the admissible
fallback max(SPT_BOUND, 4 x e32) alike.  The pack decoder is pinned by a block packed on the host from the same formulas."""
import numpy as np
import pytest
import torch

from tests import block_stack_cases as bs
from tests import d32_stage_cases as dc

H, N_TOK, N_SEQ = 8, 51, 3              # 153 rows: 9.6 tiles, an odd sequence length (the pair kernel's zero partner), two waves
SCHED = bs.REFERENCE_SCHEDULE
REJECT = 4                              # a mistake is that many times beyond the bound, in at least one row

_cache = {}


def _sd(scale_set=None):
    if ("sd", scale_set) not in _cache:
        _cache[("sd", scale_set)] = dc.make_stack32(scale_set)[1]
    return _cache[("sd", scale_set)]


def _case(n_tok, n_seq, heads, sched, seqs=None, scale_set=None):
    key = (n_tok, n_seq, heads, tuple(sched), None if seqs is None else tuple(seqs), scale_set)
    if key not in _cache:
        x = bs.make_rows(n_seq * n_tok, dc.D)
        if seqs is not None:
            x = x[(torch.tensor(seqs)[:, None] * n_tok + torch.arange(n_tok)[None, :]).flatten()]
        ref64, e32, ref32 = bs.references(_sd(scale_set), x, n_tok, heads, sched)
        print("D 32 H %d n_tok %d rows %d schedule %s %s: e32 max-scaled %.3e norm-wise %.3e"
              % (heads, n_tok, x.shape[0], sched if len(sched) < 8 else "[%d applications]" % len(sched), scale_set or "", e32[0], e32[1]))
        _cache[key] = dict(x=x, ref64=ref64, e32=e32, ref32=ref32)
    return _cache[key]


def test_inputs_tell_rows_sequences_and_tiles_apart():
    dc.assert_rows_tell_apart()
    assert all(n % bs.SCALE_PERIOD for n in dc.ALL_NTOK)
    x = bs.make_rows(64, dc.D)
    assert torch.equal(x[:20], bs.make_rows(20, dc.D))
    e = bs.row_scale_exponents(64)
    assert bool((e[dc.TILE:] != e[:-dc.TILE]).all()) and bool((e[N_TOK:] != e[:-N_TOK]).all())


BLOCK_CASES = ([("tile-edges", 1, max(dc.TILE_EDGE_M), 8, SCHED, None, None)]
               + [("short-H%d" % h, dc.SHORT["n_tok"], max(dc.SHORT["n_seqs"]), h, SCHED, None, None) for h in dc.SHORT["heads"]]
               + [("long-H%d" % h, dc.LONG["n_tok"], max(dc.LONG["n_seqs"]), h, SCHED, None, None) for h in dc.LONG["heads"]]
               + [("second-tile-%d" % n, dc.SECOND_TILE["n_tok"], n, 8, SCHED, "sample", None) for n in dc.SECOND_TILE["n_seqs"]]
               + [("third-tile", dc.THIRD_TILE["n_tok"], dc.THIRD_TILE["n_seq"], 8, SCHED, "sample", None)]
               + [("schedule-%d" % len(s), N_TOK, N_SEQ, 8, s, None, None) for s in dc.SCHEDULES]
               + [("weights-" + k, N_TOK, N_SEQ, 8, SCHED, None, k) for k in dc.SCALE_SETS])


@pytest.mark.parametrize("name,n_tok,n_seq,heads,sched,seqs,scale_set", BLOCK_CASES, ids=[c[0] for c in BLOCK_CASES])
def test_checker_accepts_the_float32_oracle_on_every_block_level_case(name, n_tok, n_seq, heads, sched, seqs, scale_set):
    c = _case(n_tok, n_seq, heads, sched, dc.sample_seqs(n_seq, n_tok) if seqs else None, scale_set)
    assert 0 < c["e32"][0] < 1e-2 and 0 < c["e32"][1] < 1e-2, c["e32"]
    assert dc.check_rows(c["ref32"], c["ref64"], c["e32"]) is None
    assert dc.check_rows(c["ref64"].float(), c["ref64"], c["e32"]) is None
    assert dc.check_rows(c["ref32"], c["ref64"], c["e32"], dc.BOUND_FLOOR_FALLBACK) is None


def test_sampled_sequences_hold_the_tile_edges():
    """The large cases are compared on sequences that contain the last row before and the first row of a wave's second and third
    tile, and the last sequence holds the ragged last tile."""
    n_tok, (below, above) = dc.SECOND_TILE["n_tok"], dc.SECOND_TILE["n_seqs"]
    assert below * n_tok == dc.TILE * dc.WAVES - 1 and above * n_tok == 4099 * dc.TILE + 2
    s = dc.sample_seqs(above, n_tok)
    assert {0, above - 1, 65535 // n_tok, 65536 // n_tok} <= set(s) and len(s) >= 10
    n_tok, n_seq = dc.THIRD_TILE["n_tok"], dc.THIRD_TILE["n_seq"]
    assert n_seq * n_tok == 131223 and -(-n_seq * n_tok // dc.TILE) == 8202
    s = dc.sample_seqs(n_seq, n_tok)
    assert {0, n_seq - 1, 65535 // n_tok, 65536 // n_tok, 131071 // n_tok, 131072 // n_tok} <= set(s) and len(s) >= 11


def test_the_restated_block_is_the_oracle_block():
    c = _case(N_TOK, N_SEQ, H, SCHED)
    assert torch.equal(dc.mutant_stack32(_sd(), c["x"], N_TOK, H, SCHED, None), c["ref64"])


@pytest.mark.parametrize("mistake", dc.MISTAKES)
def test_checker_rejects_a_constructed_mistake(mistake):
    c = _case(N_TOK, N_SEQ, H, SCHED)
    wrong = dc.mutant_stack32(_sd(), c["x"], N_TOK, H, SCHED, mistake)
    mx, nw = bs.row_errors(wrong, c["ref64"])
    for floor in (0.0, dc.BOUND_FLOOR_FALLBACK):
        b = dc.bound(c["e32"], floor)
        off = (mx > REJECT * dc.FACTOR * b[0]) | (nw > REJECT * dc.FACTOR * b[1])
        print("%s: worst row %.3e / %.3e, bound (%.3e, %.3e): %d of %d rows beyond %d x the bound"
              % (mistake, float(mx.max()), float(nw.max()), dc.FACTOR * b[0], dc.FACTOR * b[1], int(off.sum()), off.numel(), REJECT))
        assert dc.check_rows(wrong, c["ref64"], c["e32"], floor) is not None, "%s passes the row-wise bound" % mistake
        assert float(mx.max()) >= REJECT * dc.FACTOR * b[0] and float(nw.max()) >= REJECT * dc.FACTOR * b[1], (mistake, floor)
    assert dc.BOUND_FLOOR_D32 in (0.0, dc.BOUND_FLOOR_FALLBACK)


def test_the_two_mistakes_left_out_are_no_ops_at_this_width():
    c = _case(N_TOK, N_SEQ, H, SCHED)
    for mistake in ("attention_across_sequences", "proj_slice_left_at_residual"):
        assert bs.worst_row_errors(bs.mutant_stack(_sd(), c["x"], N_TOK, H, SCHED, mistake), c["ref64"]) == (0.0, 0.0), mistake


# ----------------------------------------------------------------------------- the pack decoder
@pytest.mark.parametrize("fold_q", (0, 1))
@pytest.mark.parametrize("scale_set", (None,) + tuple(dc.SCALE_SETS))
def test_pack_decoder_round_trips_a_block_packed_on_the_host(scale_set, fold_q):
    sd = _sd(scale_set)
    raw, put = dc.pack_host(sd, "blocks.1", fold_q)
    assert raw.dtype == np.uint8 and raw.size == dc.PACK_BYTES
    got = dc.decode_pack(raw)
    for k in ("hi", "lo", "c", "sc"):
        assert np.array_equal(got[k], put[k]), k
    assert got["s_att"] == put["s_att"] and got["s_hid"] == put["s_hid"] and not got["tail"].any() and not got["rest"].any()
    # the layout, stated independently of the loop that wrote it: unit 13 = fc2 column tile 0, k step 1; lane 37 = row 5, k 16 .. 23
    f = raw[:dc.PACK_VEC].view(np.float16).reshape(16, 2, 64, 8)
    assert np.array_equal(f[13, 0, 37].astype(np.float64), put["hi"][dc.C_FC2 + 5, 32 + 16:32 + 24])
    assert np.array_equal(f[4, 1, 63].astype(np.float64), put["lo"][64 + 15, 24:32])          # unit 4: v columns 0 .. 15
    # what was packed is the block: W' within two fp16 parts of the float64 W x gamma, c as formed, the scales powers of two
    W, c, terms, bnd = dc.pack_terms(sd, "blocks.1")
    qs = np.ones(dc.NCOL)
    if fold_q:
        qs[:32] = dc.SPT_QS
    colmax = np.abs(W).max(1)
    assert (np.abs(got["W"] - W * qs[:, None]).max(1) <= 2.0 ** -21 * colmax * qs).all()
    assert (np.abs(got["c"] - c * qs) <= 2.0 ** -22 * terms * qs).all()
    assert dc.pow2_exponent(got["s_att"]) is not None and dc.pow2_exponent(got["s_hid"]) is not None
    assert all(dc.pow2_exponent(v) is not None for v in put["sw"])
    fmax = np.abs(got["frag"]).max(1)
    assert ((fmax >= 2.0 ** 13) & (fmax < 2.0 ** 14)).all()
    for s, b in ((got["s_att"], bnd[64:96].max()), (got["s_hid"], bnd[dc.C_FC1:dc.C_FC2].max())):
        assert s * b <= 2.0 ** 15 < 2 * s * b
