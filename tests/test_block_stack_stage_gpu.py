"""The block stack alone (mpl_block_stack_ex: csrc/h2_phase.hpp + h2_stack_walk.inc, csrc/b1_gemm.hip, csrc/sm_stack.hip and the
per-GEMM routes of csrc/api.hip) against float64 at every launch form and shape -- no SPT stage, no tail, no forward.

Every case asks the library, on the device, which form a launch takes (mpl_block_stack_form_ex), runs the stack on synthetic rows
(tests/block_stack_cases.py: every row its own scale and mean offset) and compares every token row with mpl_oracle.block applied
along the schedule in float64.  Asserted for every run: rc, finite output, every row within FACTOR x e32 in both row-wise measures
(e32: the float32 oracle's own worst row on the same case; FACTOR = 4), the canary rows behind row M and the canary bytes behind
mpl_block_stack_workspace_bytes() of workspace keep their bits (the workspace itself is handed over as 0xFF bytes: a kernel that
read what nobody wrote would produce NaN), no device error, and the form launched (mpl_block_stack_last_form) is the form asked
for.  Per engine: rows of a smaller n_seq are BITWISE the rows of the largest one.

  fp16x2 teams, D 544, H 8: ROWS16_DIRECT, ROWS16, ROWS32, TEAMS, PAIRS, PER_GEMM forced at 1, 2, 3 tiles (last tile full, one
      sequence, S - 1 sequences; three tiles under PAIRS = a pair with an absent partner), n_tok 1 .. 32 (both attention epilogues,
      tiles of 60 / 62 / 63 / 64 rows; where no narrow form exists the switches are no-ops); every form the automatic rule can pick, at
      the smallest n_seq where it picks it (PER_GEMM is a switch only: the rule never picks it), a PAIRS launch of more than 64 tiles
      checked on its first tile, its last tile and a fixed sample of sequences
  head dims: D 544 with H 4 / 68 / 136 (hd 136 / 8 / 4: the generic LDS attention with 17 and 34 heads per slice), D 1088 with H 8 /
      16; both sides of the fusable edge (hd 8: 14 | 15 tokens, hd 4: 6 | 7): a team form on one side, UNPACKED within the bound on the other
  widths 1088, 1632, 2176, 3808 with hd 68 and 136: the team kernels at 1088; beyond, no LayerNorm operand can be packed
      (K <= 1088), the library reports UNPACKED and the nn.Linear tensors run.  3808 is the widest multiple of 544 inside the model
      envelope (J d <= 4096); 4352 .. 8704 exist as plain operands through the C ABI only and are left out
  bf16 team engine D 544 / 1088, TEAMS and PER_GEMM; small engine D 128 / 144 / 544 / 1088 (the widest it takes: 1152 is asked for
      and refused), 1 group .. as many as the device takes, up to the most rows it accepts; schedules [0], [0, 0], [1, 0, 1, 1, 0], 64 applications, the refusal of 65; one
      UNPACKED and one BF16_ANY case on the same rows.

e32 and the kernels' own worst errors ("worst so far", printed by every test, NOT asserted) are recorded in
tests/block_stack_cases.py.

The fp32-MFMA kernels on the nn.Linear tensors (csrc/ln_gemm.hip) accumulate dot products longer than 2176 columns in chunks of
512 (ACC_CHUNK): the width cases are what holds them to it.  With ONE accumulator per output element over all K / 4 matrix
instructions (K = 2 D for fc2: 1904 chained steps at D 3808) the worst row was, max-scaled / norm-wise, 2.18e-6 / 1.61e-6 against
4 x e32 = 2.12e-6 / 1.88e-6 at D 2176 hd 68 and 3.41e-6 / 2.16e-6 against 2.37e-6 / 1.89e-6 at D 3808 hd 136 (a quarter of the
rows: those of scale 2^-3 and below, whose output is the block's own), while the float32 oracle's error does not grow with K
(5.2e-7 .. 5.9e-7 from D 544 to 3808).
"""
import ctypes as C

import pytest
import torch

from openmpl_amd import cabi
from openmpl_amd.multiview_mpl import MultiView_MPL, _ptr
from tests import block_stack_cases as bs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY_BITS = 0x5A5AC3C3        # a finite float no kernel produces by accident
CANARY_ROWS = 64                # a ragged last tile that wrote its dead rows would land here
WS_CANARY = 4096
TEAM_FORMS = {cabi.FORM_TEAMS, cabi.FORM_PAIRS, cabi.FORM_ROWS32, cabi.FORM_ROWS16, cabi.FORM_ROWS16_DIRECT}
NARROW = ("ROWS32", "ROWS16", "ROWS16_DIRECT")
FORM_NAMES = {getattr(cabi, "FORM_" + n): n for n in ("UNPACKED", "SMALL", "TEAMS", "PAIRS", "ROWS32", "ROWS16", "ROWS16_DIRECT",
                                                      "PER_GEMM", "BF16_ANY")}
E_UNSUPPORTED = -2
NO_SMALL = cabi.F_NO_SMALL_STACK
_worst = {}                     # engine -> [max-scaled, norm-wise] worst row against float64 so far: printed, not asserted
_weights = {}
_refs = {}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


class _Weights:
    """One set of blocks of width D on the device, with its operands packed once per kind: "raw" (nn.Linear tensors only), "h2"
    (fp16x2), "bf16" (tuned layout), "bf16_any" (shape-general layout).  Packed operands do not depend on n_tok or the head count."""

    def __init__(self, D, depth):
        m, self.sd = bs.make_stack(D, depth)
        self.sd64 = bs.cast_sd(self.sd, torch.float64)
        self.m, self.D, self.depth, self._ops = m.to(DEV), D, depth, {}

    def blocks(self, kind):
        if kind not in self._ops:
            lib, arr, keep = cabi.load(), (cabi.BlockWeights * self.depth)(), []
            for l, b in enumerate(self.m.blocks):
                ptrs = [_ptr(t) for t in MultiView_MPL._block_ptrs(b)]
                if kind != "raw":
                    ops = MultiView_MPL._pack_block(lib, b, torch.device(DEV), _stream(), kind != "h2", kind == "bf16_any")
                    keep.append(ops)
                    ptrs += ([0] * 8 if kind == "h2" else []) + [o.data_ptr() for o in ops]
                arr[l] = cabi.BlockWeights(*ptrs)
            torch.cuda.synchronize()
            self._ops[kind] = (arr, keep)
        return self._ops[kind][0]


def _w(D, depth=2):
    if (D, depth) not in _weights:
        for k in [k for k in _weights if k[0] > 1152]:      # one wide set at a time (3808: half a gigabyte of weights)
            del _weights[k]
        for k in [k for k in _refs if k[0] > 1152 and k[0] != D]:
            del _refs[k]
        _weights[(D, depth)] = _Weights(D, depth)
    return _weights[(D, depth)]


def _ref(w, n_tok, H, sched, n_seq, bf16=False, seqs=None):
    """(input rows, float64 rows, e32) of a case, computed once; seqs: only these sequences of the n_seq (sequences are independent)."""
    key = (w.D, w.depth, n_tok, H, tuple(sched), n_seq, bf16, None if seqs is None else tuple(seqs))
    if key not in _refs:
        x = bs.make_rows(n_seq * n_tok, w.D)
        rows = None
        if seqs is not None:
            rows = (torch.tensor(seqs)[:, None] * n_tok + torch.arange(n_tok)[None, :]).flatten()
        xs = x if rows is None else x[rows]
        ref64 = bs.reference(w.sd64, xs, n_tok, H, sched, torch.float64, bf16)
        e32 = bs.worst_row_errors(bs.reference(w.sd, xs, n_tok, H, sched, torch.float32, bf16), ref64)
        print("D %d H %d n_tok %d schedule %s%s rows %d: e32 max-scaled %.3e norm-wise %.3e"
              % (w.D, H, n_tok, sched if len(sched) < 8 else "[%d applications]" % len(sched), " bf16" if bf16 else "", xs.shape[0],
                 e32[0], e32[1]))
        assert 0 < e32[0] < 1e-2 and 0 < e32[1] < 1e-2, e32
        _refs[key] = (x, ref64, e32, rows)
    return _refs[key]


def _ask(w, n_seq, n_tok, H, sched, parts, flags, raw=1):
    return cabi.load().mpl_block_stack_form_ex(n_seq, n_tok, w.D, H, len(sched), max(sched) + 1, raw, parts, flags)


def _launch(w, kind, x, n_seq, n_tok, H, sched, flags):
    """One call of the stack on the first n_seq sequences of x -> (rc, rows on the host, canary rows intact, workspace canary intact)."""
    lib, D, M = cabi.load(), w.D, n_seq * n_tok
    buf = torch.empty(M + CANARY_ROWS, D, device=DEV)
    buf[:M].copy_(x[:M])
    buf[M:].view(torch.int32).fill_(CANARY_BITS)
    wsb = lib.mpl_block_stack_workspace_bytes(n_seq, n_tok, D)
    ws = torch.full((wsb + WS_CANARY,), 0xFF, dtype=torch.uint8, device=DEV)
    ws[wsb:] = 0xA5
    arr = (C.c_uint8 * len(sched))(*sched)
    rc = lib.mpl_block_stack_ex(buf.data_ptr(), n_seq, n_tok, D, H, w.blocks(kind), arr, len(sched), ws.data_ptr(), wsb, flags, _stream())
    torch.cuda.synchronize()
    return rc, buf[:M].cpu(), bool((buf[M:].view(torch.int32) == CANARY_BITS).all()), bool((ws[wsb:] == 0xA5).all())


def _run(tag, engine, w, kind, n_seq, n_tok, H, sched, ref, flags, want_form, fails):
    """Launches, checks everything that holds for every run (failures are collected in `fails`), returns the rows."""
    x, ref64, e32, rows = ref
    lib = cabi.load()
    rc, got, canary_ok, ws_ok = _launch(w, kind, x, n_seq, n_tok, H, sched, flags)
    tag = "%s n_tok=%d n_seq=%d %s" % (tag, n_tok, n_seq, FORM_NAMES.get(want_form, want_form))
    if rc != 0:
        fails.append("%s: rc %d" % (tag, rc))
        return got
    launched = lib.mpl_block_stack_last_form()
    if launched != want_form:
        fails.append("%s: launched %s" % (tag, FORM_NAMES.get(launched, launched)))
    M = n_seq * n_tok
    cmp_got, cmp_ref = (got, ref64[:M]) if rows is None else (got[rows], ref64)
    msg = bs.check_rows(cmp_got, cmp_ref, e32)
    if bool(torch.isfinite(cmp_got).all()):
        mx, nw = bs.worst_row_errors(cmp_got, cmp_ref)
        wst = _worst.setdefault(engine, [0.0, 0.0])
        wst[0], wst[1] = max(wst[0], mx), max(wst[1], nw)
    if msg:
        fails.append("%s: %s" % (tag, msg))
    if not canary_ok:
        fails.append("%s: canary rows behind row M were overwritten" % tag)
    if not ws_ok:
        fails.append("%s: canary bytes behind the workspace were overwritten" % tag)
    if cabi.device_error():
        fails.append("%s: device error word %d" % (tag, lib.mpl_device_error(-1)))
        cabi.clear_device_error()
    return got


def _bitwise(what, rows_of, fails):
    """rows_of {n_seq: rows}: every smaller launch carries the bits of the largest."""
    big = rows_of[max(rows_of)]
    for n in sorted(rows_of)[:-1]:
        r = rows_of[n]
        if not torch.equal(r, big[:r.shape[0]]):
            diff = (r != big[:r.shape[0]]).any(1).nonzero().flatten()
            fails.append("%s: n_seq %d differs bitwise from n_seq %d in %d rows, first %s"
                         % (what, n, max(rows_of), diff.numel(), diff[:8].tolist()))


def _report(fails):
    print("worst so far (max-scaled, norm-wise): %s" % {k: ("%.3e" % v[0], "%.3e" % v[1]) for k, v in sorted(_worst.items())})
    assert not fails, "\n".join(fails)


def _mode(bits):
    cabi.check(cabi.load().mpl_x3_stack_mode(bits), "stack mode")


# ----------------------------------------------------------------------------- fp16x2 teams, D = 544, H = 8
@pytest.mark.parametrize("n_tok", bs.TEAM_NTOK)
def test_fp16x2_team_forms_forced_at_one_two_three_tiles(n_tok):
    D, H, sched = 544, 8, bs.REFERENCE_SCHEDULE
    w = _w(D)
    S = bs.BM // n_tok
    ref = _ref(w, n_tok, H, sched, 3 * S)
    legal = bs.narrow_legal(n_tok)
    fails, visited, by_form = [], set(), {}
    try:
        for name, bits in bs.FORCE_MODES.items():
            _mode(bits | bs.MODE_NO_SMALL)
            want = getattr(cabi, "FORM_" + name) if (legal or name not in NARROW) else cabi.FORM_TEAMS     # no narrow form: a no-op
            for T in (1, 2, 3):
                for n_seq in bs.tail_n_seqs(n_tok, T):
                    asked = _ask(w, n_seq, n_tok, H, sched, 2, 0)
                    assert asked == want, (name, n_tok, n_seq, FORM_NAMES.get(asked, asked))
                    visited.add((asked, T))
                    by_form.setdefault(name, {})[n_seq] = _run("forced " + name, "fp16x2 teams", w, "h2", n_seq, n_tok, H, sched, ref,
                                                               0, asked, fails)
    finally:
        _mode(0)
    for name, rows_of in by_form.items():
        _bitwise("forced %s n_tok %d" % (name, n_tok), rows_of, fails)
    # every persistent form carries the bits of the whole-tile teams (the per-GEMM launches agree with themselves)
    big = by_form["TEAMS"][3 * S]
    for name in by_form:
        if name != "PER_GEMM" and not torch.equal(by_form[name][3 * S], big):
            fails.append("forced %s n_tok %d: differs bitwise from the whole-tile teams" % (name, n_tok))
    print("n_tok %d visited %s" % (n_tok, sorted((FORM_NAMES[f], T) for f, T in visited)))     # (each form is asserted where it is asked)
    _report(fails)


def _first_n_seq_of_each_form(w, n_tok, H, sched, limit):
    first = {}
    for n_seq in range(1, limit + 1):
        first.setdefault(_ask(w, n_seq, n_tok, H, sched, 2, NO_SMALL), n_seq)
    return first


def _sampled(n_seq, n_tok):
    """First tile, last tile and every 37th sequence in between."""
    S = bs.BM // n_tok
    last_tile = ((n_seq - 1) // S) * S
    return sorted(set(range(S)) | set(range(last_tile, n_seq)) | set(range(0, n_seq, 37)))


def test_fp16x2_team_forms_where_the_automatic_rule_picks_them():
    """No switch set, MPL_F_NO_SMALL_STACK: the smallest n_seq of every form the rule reaches.  256 compute units: ROWS16_DIRECT
    from one sequence, ROWS32 from 17 tiles, TEAMS from 33, PAIRS from 65 (D 544); ROWS16 (ring: the A operand of fc2 does not fit)
    at D 1088.  Launches of more than four tiles are compared on their first tile, last tile and a fixed sample of sequences."""
    H, n_tok, sched = 8, 4, bs.REFERENCE_SCHEDULE
    fails, visited = [], set()
    _mode(0)
    for D, limit in ((544, 1100), (1088, 40)):
        w = _w(D)
        for form, n_seq in sorted(_first_n_seq_of_each_form(w, n_tok, H, sched, limit).items()):
            assert form in TEAM_FORMS, (D, n_seq, form)
            if D == 1088 and form != cabi.FORM_ROWS16:
                continue
            seqs = _sampled(n_seq, n_tok) if n_seq * n_tok > 4 * bs.BM else None
            ref = _ref(w, n_tok, H, sched, n_seq, seqs=seqs)
            print("D %d: the rule picks %s from n_seq %d on" % (D, FORM_NAMES[form], n_seq))
            visited.add(form)
            _run("auto D %d" % D, "fp16x2 teams", w, "h2", n_seq, n_tok, H, sched, ref, NO_SMALL, form, fails)
    if _cus() == 256 and visited != TEAM_FORMS:
        fails.append("visited %s, required %s" % (sorted(visited), sorted(TEAM_FORMS)))
    _report(fails)


# ----------------------------------------------------------------------------- head dims and the fusable edge
@pytest.mark.parametrize("D,H", bs.HEAD_DIM_SHAPES, ids=["D%d-H%d" % c for c in bs.HEAD_DIM_SHAPES])
def test_fp16x2_teams_at_every_head_dim_and_both_sides_of_the_fusable_edge(D, H):
    """Two tiles and a one-sequence tail under the automatic rule, the whole-tile teams and the two-tile stage.  Where the score
    matrices of a slice do not fit the LDS beside the q | k | v tile (h2_attention_fusable) the fp16x2 operands have no engine:
    the library reports UNPACKED and runs the nn.Linear tensors -- within the same bound."""
    hd, sched = D // H, bs.REFERENCE_SCHEDULE
    w = _w(D)
    fails, side = [], {}
    try:
        for n_tok in sorted(set(bs.TEAM_NTOK) | {6, 14, 15}):
            n_seq = 2 * (bs.BM // n_tok) + 1
            ref = _ref(w, n_tok, H, sched, n_seq)
            for name, bits in (("auto", 0), ("TEAMS", bs.FORCE_MODES["TEAMS"]), ("PAIRS", bs.FORCE_MODES["PAIRS"])):
                _mode(bits)
                asked = _ask(w, n_seq, n_tok, H, sched, 2, NO_SMALL)
                assert asked in TEAM_FORMS or asked == cabi.FORM_UNPACKED, (n_tok, asked)
                side[n_tok] = asked in TEAM_FORMS
                if name != "auto" and (asked == cabi.FORM_UNPACKED or asked != getattr(cabi, "FORM_" + name)):
                    assert asked == cabi.FORM_UNPACKED, (name, n_tok, asked)
                    continue
                _run("hd %d %s" % (hd, name), "fp16x2 teams" if side[n_tok] else "fp32 MFMA (unpacked)", w, "h2", n_seq, n_tok, H, sched,
                     ref, NO_SMALL, asked, fails)
    finally:
        _mode(0)
    packed = sorted(n for n, s in side.items() if s)
    print("D %d hd %d: team forms at n_tok %s, UNPACKED at %s" % (D, hd, packed, sorted(n for n, s in side.items() if not s)))
    edge = {8: 14, 4: 6}.get(hd, 32)
    assert packed == [n for n in sorted(side) if n <= edge], (hd, packed)
    _report(fails)


# ----------------------------------------------------------------------------- widths
@pytest.mark.parametrize("D,H", bs.WIDTH_SHAPES, ids=["D%d-hd%d" % (D, D // H) for D, H in bs.WIDTH_SHAPES])
def test_widths_1088_1632_2176_3808(D, H):
    """One block applied twice, two tiles and a one-sequence tail, 4 and 5 tokens (64- and 60-row tiles).  The team kernels take
    widths up to 1088: a LayerNorm is folded into no wider operand (mpl_pack_h2 refuses it: the LayerNorm GEMMs combine at most 8
    slice partials per row), so for 1632 .. 3808 the library must report UNPACKED -- whatever operands the caller claims -- and
    run the nn.Linear tensors within the same bound (test_h2_gpu.py pins the rule)."""
    sched = [0, 0]
    w = _w(D, 1)
    lib = cabi.load()
    teams = lib.mpl_team_stack_shape(D, H, 4) == 1
    assert teams == (D <= 1088), (D, H)
    fails = []
    _mode(0)
    for n_tok in (4, 5):
        n_seq = 2 * (bs.BM // n_tok) + 1
        ref = _ref(w, n_tok, H, sched, n_seq)
        asked = _ask(w, n_seq, n_tok, H, sched, 2, NO_SMALL)
        assert (asked in TEAM_FORMS) if teams else (asked == cabi.FORM_UNPACKED), (D, H, n_tok, asked)
        _run("width %d hd %d" % (D, D // H), "fp16x2 teams" if teams else "fp32 MFMA (unpacked)", w, "h2" if teams else "raw", n_seq,
             n_tok, H, sched, ref, NO_SMALL, asked, fails)
    _report(fails)


# ----------------------------------------------------------------------------- the bf16 team engine
@pytest.mark.parametrize("D", (544, 1088))
def test_bf16_team_engine_against_its_emulation(D):
    """TEAMS and PER_GEMM at 1, 2, 3 tiles against mpl_oracle.block_bf16 in float64; e32 = its float32 evaluation (the operands
    that sit within fp32 noise of a bf16 rounding boundary round the other way there, as they may in the kernels)."""
    H, sched = 8, bs.REFERENCE_SCHEDULE
    w = _w(D)
    lib = cabi.load()
    fails, visited = [], set()
    try:
        for n_tok in bs.BF16_NTOK:
            assert lib.mpl_bf16_operand_layout(D, H, n_tok) == cabi.BF16_TUNED
            S = bs.BM // n_tok
            ref = _ref(w, n_tok, H, sched, 3 * S, bf16=True)
            for name, bits in (("TEAMS", 0), ("PER_GEMM", 1)):
                _mode(bits)
                rows_of = {}
                for T in (1, 2, 3):
                    for n_seq in bs.tail_n_seqs(n_tok, T):
                        asked = _ask(w, n_seq, n_tok, H, sched, 1, 0)
                        assert asked == getattr(cabi, "FORM_" + name), (name, n_tok, n_seq, asked)
                        visited.add(asked)
                        rows_of[n_seq] = _run("bf16 " + name, "bf16 teams", w, "bf16", n_seq, n_tok, H, sched, ref, 0, asked, fails)
                _bitwise("bf16 %s n_tok %d" % (name, n_tok), rows_of, fails)
    finally:
        _mode(0)
    assert visited == {cabi.FORM_TEAMS, cabi.FORM_PER_GEMM}
    _report(fails)


# ----------------------------------------------------------------------------- the small engine
def test_small_engine_width_envelope():
    """Asked, not assumed: the engine takes D % 16 == 0 from 128 to 1088 (sm_stack_ok lets 1152 pass its k-step count, but the two
    16 x 2 D weight tiles of fc2 do not fit the LDS there), and no width that is not a multiple of 16."""
    lib = cabi.load()
    _mode(0)
    small = lambda D, H: lib.mpl_block_stack_form_ex(1, 2, D, H, 3, 2, 1, 0, 0) == cabi.FORM_SMALL
    assert not small(112, 4) and small(128, 8) and small(144, 4) and not small(136, 2) and small(1088, 4)
    assert not small(1104, 4) and not small(1152, 8) and [D for D in range(16, 1300, 16) if small(D, 4)] == list(range(128, 1089, 16))
    assert lib.mpl_block_stack_form_ex(1, 2, 1152, 8, 3, 2, 1, 0, 0) == cabi.FORM_UNPACKED


@pytest.mark.parametrize("D,H,packed", bs.SMALL_SHAPES, ids=["D%d-H%d-%s" % (D, H, "h2" if p else "raw") for D, H, p in bs.SMALL_SHAPES])
def test_small_engine_at_every_group_layout(D, H, packed):
    """Every n_seq the library gives to the small engine is found by asking; run: the first and the last n_seq of every group count,
    launches whose last group is short of sequences, and the most rows the device accepts.  D 128 / 144 and one case at 1088 carry
    no packed operands (the straight-line k-step code at its edges: 8, 9 and 68 k-steps among eight waves)."""
    sched, cus = bs.REFERENCE_SCHEDULE, _cus()
    kind, parts = ("h2", 2) if packed else ("raw", 0)
    w = _w(D)
    fails, counts, short = [], set(), 0
    _mode(0)
    for n_tok in bs.SMALL_NTOK:
        taken = [n for n in range(1, 400 // n_tok + 1) if _ask(w, n, n_tok, H, sched, parts, 0) == cabi.FORM_SMALL]
        assert taken and taken[0] == 1, (D, n_tok, taken)
        groups = {n: bs.small_groups(n, n_tok, D, cus) for n in taken}
        assert all(g > 0 for g, _ in groups.values()), "the restated layout refuses what the library takes: %s" % groups
        # up to the most rows the library takes, it takes exactly what the restated layout takes (beyond: its own row limit)
        assert taken == [n for n in range(1, taken[-1] + 1) if bs.small_groups(n, n_tok, D, cus)[0] > 0], (D, n_tok, taken)
        pick = {taken[-1]}
        for g in sorted({g for g, _ in groups.values()}):
            of_g = [n for n in taken if groups[n][0] == g]
            pick |= {of_g[0], of_g[-1]}
            pick |= set([n for n in of_g if n % groups[n][1]][:1])         # the last group short of sequences
        ref = _ref(w, n_tok, H, sched, taken[-1])
        print("D %d n_tok %d: small engine up to %d rows; n_seq -> (groups, sequences per group): %s"
              % (D, n_tok, taken[-1] * n_tok, {n: groups[n] for n in sorted(pick)}))
        rows_of = {}
        for n_seq in sorted(pick):
            counts.add(groups[n_seq][0])
            short += int(n_seq % groups[n_seq][1] != 0)
            rows_of[n_seq] = _run("small D %d" % D, "small engine", w, kind, n_seq, n_tok, H, sched, ref, 0, cabi.FORM_SMALL, fails)
        _bitwise("small D %d n_tok %d" % (D, n_tok), rows_of, fails)
    print("D %d: group counts visited %s, %d launches with a short last group" % (D, sorted(counts), short))
    if cus == 256:
        assert 1 in counts
        if D <= 544:
            assert 2 in counts and counts & {3, 4, 5} and short > 0, counts
    _report(fails)


# ----------------------------------------------------------------------------- schedules
@pytest.mark.parametrize("engine", ("teams", "small"))
@pytest.mark.parametrize("sched", bs.SCHEDULES, ids=["one", "same-twice", "non-monotone", "64-applications"])
def test_schedules_other_than_the_reference_s(sched, engine):
    """Two blocks, seven sequences of five tokens: one ragged 60-row tile / three groups of the small engine."""
    D, H, n_tok, n_seq = 544, 8, 5, 7
    w = _w(D)
    flags = NO_SMALL if engine == "teams" else 0
    fails = []
    _mode(0)
    ref = _ref(w, n_tok, H, sched, n_seq)
    asked = _ask(w, n_seq, n_tok, H, sched, 2, flags)
    assert asked == cabi.FORM_SMALL if engine == "small" else asked in TEAM_FORMS, asked
    _run("schedule", "small engine" if engine == "small" else "fp16x2 teams", w, "h2", n_seq, n_tok, H, sched, ref, flags, asked, fails)
    _report(fails)


@pytest.mark.parametrize("kind,flags", [("h2", NO_SMALL), ("h2", 0), ("raw", 0), ("bf16", 0)], ids=["teams", "small-shaped", "raw", "bf16"])
def test_65_applications_are_refused_and_nothing_is_touched(kind, flags):
    D, H, n_tok, n_seq = 544, 8, 5, 7
    w = _w(D)
    sched = [i % 2 for i in range(bs.MAX_APPS + 1)]
    x = bs.make_rows(n_seq * n_tok, D)
    _mode(0)
    assert cabi.load().mpl_block_stack_form_ex(n_seq, n_tok, D, H, len(sched), 2, 1, 2, flags) < 0
    rc, got, canary_ok, ws_ok = _launch(w, kind, x, n_seq, n_tok, H, sched, flags)
    assert rc == E_UNSUPPORTED, rc
    assert torch.equal(got, x) and canary_ok and ws_ok
    assert not cabi.device_error()


# ----------------------------------------------------------------------------- the other engines on the same rows
def test_unpacked_and_shape_general_bf16_engines_on_the_same_rows():
    D, n_tok, sched = 544, 4, bs.REFERENCE_SCHEDULE
    w = _w(D)
    lib = cabi.load()
    n_seq = 2 * (bs.BM // n_tok) + 1
    fails = []
    _mode(0)
    asked = _ask(w, n_seq, n_tok, 8, sched, 0, 0)
    assert asked == cabi.FORM_UNPACKED, asked
    _run("raw tensors", "fp32 MFMA (unpacked)", w, "raw", n_seq, n_tok, 8, sched, _ref(w, n_tok, 8, sched, n_seq), 0, asked, fails)
    H = 16          # head dim 34 tiles no 136-column slice: the shape-general bf16 layout
    assert lib.mpl_bf16_operand_layout(D, H, n_tok) == cabi.BF16_ANY
    asked = _ask(w, n_seq, n_tok, H, sched, 1, 0)
    assert asked == cabi.FORM_BF16_ANY, asked
    _run("bf16 any", "bf16 shape-general", w, "bf16_any", n_seq, n_tok, H, sched, _ref(w, n_tok, H, sched, n_seq, bf16=True), 0, asked, fails)
    _report(fails)
