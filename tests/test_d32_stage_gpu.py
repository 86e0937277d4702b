"""The D = 32 block kernels of the joints x views token grid alone against float64: mpl_block_stack_ex at D = 32 (csrc/api.hip,
`if (d32)`: d32_qkv_kernel -> launch_token_attention -> d32_mlp_kernel of csrc/d32_blocks.hip, three launches per application, all
reading the operand of mpl_d32_pack), the long attention kernels at their class edges (mpl_token_attention) and the packed operand
itself (spt_pack_kernel, decoded on the host) -- no SPT stage, no tail, no forward.

Block level: two operand kinds on the same rows (tests/block_stack_cases.py: every row its own scale and mean offset), "d32" (the
nn.Linear tensors plus qkv_w3 from mpl_d32_pack, every other packed field NULL) and "raw" (the nn.Linear tensors only: at K = 32
launch_ng_auto / row_stats32_kernel).  Every token row is compared with mpl_oracle.block along the schedule in float64.  Asserted
for every run: rc 0, finite output, every row within the bound (tests/d32_stage_cases.py: FACTOR x e32, e32 the float32 oracle's
own worst row on the same case), canary rows behind row M and canary bytes behind mpl_block_stack_workspace_bytes() intact (the
workspace is handed over as 0xFF bytes), no device error, mpl_block_stack_last_form() == FORM_UNPACKED, and for "d32" exactly three
launches per application (the d32 kernels ran, not the six-launch route).  Per kind: rows of a smaller n_seq are BITWISE the first
rows of the largest.

  tile edges     n_tok 1, H 8, M 1 / 15 / 16 / 17 / 127 / 128 / 129 (a tile, then a workgroup's eight tiles: short, full, over)
  short          n_tok 17, n_seq 1 / 8 / 16 (17, 136 = 8.5 tiles, 272 rows), H 8 (LDS kernel) and H 32 (head dim 1: any-kernel)
  long           n_tok 51 (odd, two waves), n_seq 1 / 3 / 5, H 8 (long_p4), H 4 (long), H 2 (head dim 16: wide)
  second tile    n_tok 51, n_seq 1285 (M 65535: 4096 tiles, no wave walks twice) | 1286 (M 65586 = 4099 tiles + 2 rows: waves 0 .. 3
                 walk a second tile, wave 3's with two live rows)
  third tile     n_tok 527, n_seq 249 (M 131223, 8202 tiles); the two large cases are compared on a fixed sample of sequences
                 (d32_stage_cases.sample_seqs), the kernels run on everything and everything must be finite
  schedules      [0], the reference's [0, 1, 1], twelve alternating applications (the timed depth), 64, the refusal of 65
  magnitudes     the two weight-magnitude sets of test_spt_split_operands_follow_the_weight_magnitudes, both kinds

e32, the bound in force and the kernels' own worst rows ("worst so far": printed, NOT asserted) are recorded in
tests/d32_stage_cases.py.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from openmpl_amd import cabi
from openmpl_amd.multiview_mpl import MultiView_MPL, _ptr
from tests import block_stack_cases as bs
from tests import d32_stage_cases as dc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = dc.D
CANARY_BITS = 0x5A5AC3C3        # a finite float no kernel produces by accident
CANARY_ROWS = 64                # a ragged last tile that wrote its dead rows would land here
WS_CANARY = 4096
E_UNSUPPORTED = -2
KINDS = ("d32", "raw")
FLOOR = {"d32": dc.BOUND_FLOOR_D32, "raw": 0.0}
ENGINE = {"d32": "d32 kernels (packed operand)", "raw": "fp32 MFMA (unpacked, K 32)"}
_worst = {}                     # engine -> [max-scaled, norm-wise] worst row against float64 so far: printed, not asserted
_weights = {}
_refs = {}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _launches(fn):
    """(result, number of kernels launched while fn ran)."""
    cabi.profile_start()
    try:
        res = fn()
    finally:
        torch.cuda.synchronize()
        counts = cabi.profile_stop()
    return res, sum(n for _, n in counts.values())


class _Weights:
    """Two blocks of width 32 on the device; kind "raw": the nn.Linear tensors only, "d32": plus the operand of mpl_d32_pack in
    qkv_w3 (every other packed field NULL)."""

    def __init__(self, scale_set):
        m, self.sd = dc.make_stack32(scale_set)
        self.sd64 = bs.cast_sd(self.sd, torch.float64)
        self.m, self.scale_set, self._ops = m.to(DEV), scale_set, {}

    def pack(self, l, fold_q=False):
        """The 48-KiB operand of block l on the device, by mpl_d32_pack (fold_q: by mpl_spt_pack)."""
        lib = cabi.load()
        bw = cabi.BlockWeights(*[_ptr(t) for t in MultiView_MPL._block_ptrs(self.m.blocks[l])])
        pk = torch.full((lib.mpl_spt_pack_bytes(),), 0xFF, dtype=torch.uint8, device=DEV)
        fn = lib.mpl_spt_pack if fold_q else lib.mpl_d32_pack
        cabi.check(fn(C.byref(bw), pk.data_ptr(), _stream()), "pack")
        torch.cuda.synchronize()
        return pk

    def blocks(self, kind):
        if kind not in self._ops:
            arr, keep = (cabi.BlockWeights * len(self.m.blocks))(), []
            for l, b in enumerate(self.m.blocks):
                ptrs = [_ptr(t) for t in MultiView_MPL._block_ptrs(b)]
                if kind == "d32":
                    keep.append(self.pack(l))
                    ptrs += [0] * 4 + [keep[-1].data_ptr()]        # qkv_w3 behind the four *_w16 fields
                arr[l] = cabi.BlockWeights(*ptrs)
            self._ops[kind] = (arr, keep)
        return self._ops[kind][0]


def _w(scale_set=None):
    if scale_set not in _weights:
        _weights[scale_set] = _Weights(scale_set)
    return _weights[scale_set]


def _ref(w, n_tok, H, sched, n_seq, seqs=None):
    """(input rows, float64 rows, e32, compared rows or None) of a case, computed once; seqs: only these sequences are compared."""
    key = (w.scale_set, n_tok, H, tuple(sched), n_seq, None if seqs is None else tuple(seqs))
    if key not in _refs:
        x = bs.make_rows(n_seq * n_tok, D)
        rows = None
        if seqs is not None:
            rows = (torch.tensor(seqs)[:, None] * n_tok + torch.arange(n_tok)[None, :]).flatten()
        xs = x if rows is None else x[rows]
        ref64 = bs.reference(w.sd64, xs, n_tok, H, sched, torch.float64)
        e32 = bs.worst_row_errors(bs.reference(w.sd, xs, n_tok, H, sched, torch.float32), ref64)
        print("D 32 H %d n_tok %d schedule %s %s rows %d of %d: e32 max-scaled %.3e norm-wise %.3e"
              % (H, n_tok, sched if len(sched) < 8 else "[%d applications]" % len(sched), w.scale_set or "", xs.shape[0], x.shape[0],
                 e32[0], e32[1]))
        assert 0 < e32[0] < 1e-2 and 0 < e32[1] < 1e-2, e32
        _refs[key] = (x, ref64, e32, rows)
    return _refs[key]


def _launch(w, kind, x, n_seq, n_tok, H, sched):
    """One call of the stack on the first n_seq sequences of x -> (rc, rows on the host, canary rows intact, workspace canary
    intact, kernels launched)."""
    lib, M = cabi.load(), n_seq * n_tok
    buf = torch.empty(M + CANARY_ROWS, D, device=DEV)
    buf[:M].copy_(x[:M])
    buf[M:].view(torch.int32).fill_(CANARY_BITS)
    wsb = lib.mpl_block_stack_workspace_bytes(n_seq, n_tok, D)
    ws = torch.full((wsb + WS_CANARY,), 0xFF, dtype=torch.uint8, device=DEV)
    ws[wsb:] = 0xA5
    arr = (C.c_uint8 * len(sched))(*sched)
    blocks = w.blocks(kind)
    rc, launched = _launches(lambda: lib.mpl_block_stack_ex(buf.data_ptr(), n_seq, n_tok, D, H, blocks, arr, len(sched), ws.data_ptr(),
                                                           wsb, 0, _stream()))
    return rc, buf[:M].cpu(), bool((buf[M:].view(torch.int32) == CANARY_BITS).all()), bool((ws[wsb:] == 0xA5).all()), launched


def _run(tag, w, kind, n_seq, n_tok, H, sched, ref, fails):
    """Launches, checks everything that holds for every run (failures are collected in `fails`), returns the rows."""
    x, ref64, e32, rows = ref
    lib = cabi.load()
    rc, got, canary_ok, ws_ok, launched = _launch(w, kind, x, n_seq, n_tok, H, sched)
    tag = "%s %s n_tok=%d n_seq=%d H=%d" % (tag, kind, n_tok, n_seq, H)
    if rc != 0:
        fails.append("%s: rc %d" % (tag, rc))
        return got
    if lib.mpl_block_stack_last_form() != cabi.FORM_UNPACKED:
        fails.append("%s: launched form %d" % (tag, lib.mpl_block_stack_last_form()))
    if kind == "d32" and launched != 3 * len(sched):
        fails.append("%s: %d launches for %d applications, the d32 route has 3 each" % (tag, launched, len(sched)))
    if kind == "raw" and launched <= 3 * len(sched):
        fails.append("%s: %d launches for %d applications: not the per-GEMM route" % (tag, launched, len(sched)))
    if not bool(torch.isfinite(got).all()):
        fails.append("%s: %d non-finite elements in the whole output" % (tag, int((~torch.isfinite(got)).sum())))
    M = n_seq * n_tok
    if rows is None:
        cmp_got, cmp_ref = got, ref64[:M]
    else:
        keep = rows < M
        cmp_got, cmp_ref = got[rows[keep]], ref64[keep]
    msg = dc.check_rows(cmp_got, cmp_ref, e32, FLOOR[kind])
    if msg and rows is not None and cmp_got.shape == cmp_ref.shape:
        b = dc.bound(e32, FLOOR[kind])
        mxr, nwr = bs.row_errors(cmp_got, cmp_ref)
        off = rows[keep][~((mxr <= dc.FACTOR * b[0]) & (nwr <= dc.FACTOR * b[1]))]
        msg += " (indices into the sampled rows; rows of the launch: %s)" % off[:8].tolist()
    if bool(torch.isfinite(cmp_got).all()):
        mx, nw = bs.worst_row_errors(cmp_got, cmp_ref)
        wst = _worst.setdefault(ENGINE[kind], [0.0, 0.0])
        wst[0], wst[1] = max(wst[0], mx), max(wst[1], nw)
        print("%s: worst row %.3e / %.3e = %.2f / %.2f x e32" % (tag, mx, nw, mx / e32[0], nw / e32[1]))
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


def _family(tag, kind, n_tok, n_seqs, H, sched, scale_set=None, sampled=False):
    """One case family: every n_seq on the rows of the largest, within the bound and bitwise the first rows of the largest."""
    w, fails, rows_of = _w(scale_set), [], {}
    big = max(n_seqs)
    # (sampled: the fixed sample of the largest launch and the last sequence of every smaller one -- its ragged last tile)
    seqs = sorted(set(dc.sample_seqs(big, n_tok)) | {n - 1 for n in n_seqs}) if sampled else None
    ref = _ref(w, n_tok, H, sched, big, seqs=seqs)
    for n_seq in n_seqs:
        rows_of[n_seq] = _run(tag, w, kind, n_seq, n_tok, H, sched, ref, fails)
    _bitwise("%s %s n_tok %d H %d" % (tag, kind, n_tok, H), rows_of, fails)
    _report(fails)


# ----------------------------------------------------------------------------- 3. the stack alone
def test_inputs_tell_rows_sequences_and_tiles_apart():
    dc.assert_rows_tell_apart()


@pytest.mark.parametrize("kind", KINDS)
def test_tile_edges_one_token_sequences(kind):
    _family("tile edges", kind, 1, dc.TILE_EDGE_M, 8, bs.REFERENCE_SCHEDULE)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H", dc.SHORT["heads"])
def test_short_attention_17_tokens(H, kind):
    _family("short", kind, dc.SHORT["n_tok"], dc.SHORT["n_seqs"], H, bs.REFERENCE_SCHEDULE)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H", dc.LONG["heads"])
def test_long_attention_51_tokens(H, kind):
    _family("long", kind, dc.LONG["n_tok"], dc.LONG["n_seqs"], H, bs.REFERENCE_SCHEDULE)


@pytest.mark.parametrize("kind", KINDS)
def test_a_second_tile_per_wave_both_sides_of_the_edge(kind):
    _family("second tile", kind, dc.SECOND_TILE["n_tok"], dc.SECOND_TILE["n_seqs"], 8, bs.REFERENCE_SCHEDULE, sampled=True)


@pytest.mark.parametrize("kind", KINDS)
def test_a_third_tile_per_wave(kind):
    _family("third tile", kind, dc.THIRD_TILE["n_tok"], (dc.THIRD_TILE["n_seq"],), 8, bs.REFERENCE_SCHEDULE, sampled=True)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("sched", dc.SCHEDULES, ids=["one", "reference", "12-applications", "64-applications"])
def test_schedules(sched, kind):
    _family("schedule", kind, 51, (3,), 8, sched)


@pytest.mark.parametrize("kind", KINDS)
def test_65_applications_are_refused_and_nothing_is_touched(kind):
    n_tok, n_seq = 51, 3
    sched = [i % 2 for i in range(bs.MAX_APPS + 1)]
    x = bs.make_rows(n_seq * n_tok, D)
    rc, got, canary_ok, ws_ok, launched = _launch(_w(), kind, x, n_seq, n_tok, 8, sched)
    assert rc == E_UNSUPPORTED and launched == 0, (rc, launched)
    assert torch.equal(got, x) and canary_ok and ws_ok
    assert not cabi.device_error()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("scale_set", list(dc.SCALE_SETS))
def test_weights_at_unusual_magnitudes(scale_set, kind):
    _family("weights " + scale_set, kind, 51, (3,), 8, bs.REFERENCE_SCHEDULE, scale_set=scale_set)


# ----------------------------------------------------------------------------- 4. the long attention kernels at their class edges
def _attention_ref(qkv, n_seq, n_tok, H, dtype):
    hd = D // H
    t = qkv.to(dtype).reshape(n_seq, n_tok, 3, H, hd).permute(2, 0, 3, 1, 4)
    att = ((t[0] @ t[1].transpose(-2, -1)) * hd ** -0.5).softmax(-1)
    return (att @ t[2]).transpose(1, 2).reshape(n_seq * n_tok, D)


def _attention_rows(n_tok, H, scale=1.0, factor=dc.FACTOR):
    """mpl_token_attention on two sequences (the second one's base offset counts), NaN-filled output, error per query row against
    float64; bound: factor x the worst row of the same formula evaluated by torch in float32 on the same inputs."""
    lib, n_seq = cabi.load(), 2
    g = torch.Generator().manual_seed(n_tok * 10 + H)
    qkv = torch.randn(n_seq * n_tok, 3 * D, generator=g) * scale
    qd = qkv.to(DEV)
    out = torch.full((n_seq * n_tok, D), float("nan"), device=DEV)
    (rc, launched) = _launches(lambda: lib.mpl_token_attention(qd.data_ptr(), n_seq, n_tok, D, H, out.data_ptr(), _stream()))
    cabi.check(rc, "mpl_token_attention")
    assert launched == 1
    ref64 = _attention_ref(qkv, n_seq, n_tok, H, torch.float64)
    e32 = bs.worst_row_errors(_attention_ref(qkv, n_seq, n_tok, H, torch.float32), ref64)
    got = out.cpu()
    assert torch.isfinite(got).all(), "%d elements not written or not finite" % int((~torch.isfinite(got)).sum())
    mx, nw = bs.worst_row_errors(got, ref64)
    wst = _worst.setdefault("attention hd %d" % (D // H), [0.0, 0.0])
    wst[0], wst[1] = max(wst[0], mx / e32[0]), max(wst[1], nw / e32[1])
    print("attention n_tok %d H %d: float32 torch worst row %.3e / %.3e, kernel %.3e / %.3e = %.2f / %.2f x (worst ratio so far %.2f / %.2f)"
          % (n_tok, H, e32[0], e32[1], mx, nw, mx / e32[0], nw / e32[1], wst[0], wst[1]))
    msg = bs.check_rows(got, ref64, e32, factor)
    assert msg is None, "attention n_tok %d H %d: %s" % (n_tok, H, msg)
    assert not cabi.device_error()


@pytest.mark.parametrize("n_tok", dc.ATT_P4_NTOK)
def test_long_p4_attention_at_its_class_edges(n_tok):
    """H 8, head dim 4: wave counts 1 | 2 | 3 | 4 at 48 | 96 | 144 tokens, one / two / three rows per lane with dead lanes in the last
    set, the second round from 769 tokens on, odd last keys, the production length 527, the LDS cap 2048."""
    _attention_rows(n_tok, 8)


@pytest.mark.parametrize("n_tok", dc.ATT_LONG_NTOK)
def test_long_attention_head_dim_8_at_its_class_edges(n_tok):
    _attention_rows(n_tok, 4)


def test_long_p4_attention_large_scores_at_the_production_length():
    """|q.k| x scale of about 60 (test_token_attention_large_scores_subtract_the_max): the softmax of such scores amplifies the
    scores' own float32 rounding by their magnitude, hence 60 x the bound."""
    _attention_rows(527, 8, scale=60 ** 0.5, factor=60 * dc.FACTOR)


# ----------------------------------------------------------------------------- 5. the packed operand itself
def _degenerate():
    """One all-zero weight row in qkv (a v column), proj, fc2, one zero gain in norm1 and norm2 = 0 altogether (every fc1 column
    of W' zero): the amax == 0 branch of the column scale."""
    w = _Weights(None)
    with torch.no_grad():
        b = w.m.blocks[1]
        b.attn.qkv.weight[70].zero_(); b.attn.proj.weight[3].zero_(); b.mlp.fc2.weight[31].zero_()
        b.norm1.weight[7] = 0.0
        b.norm2.weight.zero_()
    w.sd = {k: v.detach().cpu().clone() for k, v in w.m.state_dict().items()}
    return w


@pytest.mark.parametrize("which", [None] + list(dc.SCALE_SETS) + ["degenerate"], ids=lambda v: v or "normal")
def test_packed_operand_decoded_on_the_host(which):
    """mpl_spt_pack and mpl_d32_pack on the same block.  W' = (hi + lo) sc_n x input scale within 2^-21 of the column's largest
    magnitude of the float64 W x gamma (two fp16 parts carry 22 bits); c_n within 2^-23 (|b_n| + sum_k |beta_k W_nk|) (summed in
    fp64, rounded once); every scale a power of two, max_k |W'_nk| sw_n in [2^13, 2^14), s x bound <= 2^15 < 2 s x bound; the two
    packs byte-identical except c and sc of the q columns, which differ by SPT_QS to one float32 rounding."""
    w = _degenerate() if which == "degenerate" else _w(which)
    for l in (0, 1):
        raw_d, raw_s = w.pack(l).cpu().numpy(), w.pack(l, fold_q=True).cpu().numpy()
        pd, ps = dc.decode_pack(raw_d), dc.decode_pack(raw_s)
        W, c, terms, bnd = dc.pack_terms(w.sd, "blocks.%d" % l)
        colmax = np.abs(W).max(1)
        zero = colmax == 0
        assert zero.any() == (which == "degenerate" and l == 1)
        for name, p in (("d32", pd), ("spt", ps)):
            for k in ("frag", "c", "sc", "W"):
                assert np.isfinite(p[k]).all(), (name, k)
            assert np.isfinite([p["s_att"], p["s_hid"]]).all() and not p["tail"].any(), name
            assert dc.pow2_exponent(p["s_att"]) is not None and dc.pow2_exponent(p["s_hid"]) is not None, (p["s_att"], p["s_hid"])
            for s, b in ((p["s_att"], bnd[64:96].max()), (p["s_hid"], bnd[dc.C_FC1:dc.C_FC2].max())):
                assert s * b <= 2.0 ** 15 < 2 * s * b, (name, s, b)
            fmax = np.abs(p["frag"]).max(1)
            assert ((fmax[~zero] >= 2.0 ** 13) & (fmax[~zero] < 2.0 ** 14)).all(), name
            assert not fmax[zero].any()
            cols = slice(32, None) if name == "spt" else slice(None)      # the q columns of mpl_spt_pack: against the other pack below
            sw = 1.0 / (p["sc"] * p["in_scale"])
            assert all(dc.pow2_exponent(v) is not None for v in sw[cols]), name
            assert (sw[zero] == 1.0).all()
            errW = np.abs(p["W"] - W).max(1)
            assert (errW[cols] <= 2.0 ** -21 * colmax[cols]).all(), (name, float((errW[cols] / np.maximum(colmax[cols], 1e-300)).max()))
            errc = np.abs(p["c"] - c)
            assert (errc[cols] <= 2.0 ** -23 * terms[cols]).all(), (name, float((errc[cols] / terms[cols]).max()))
        # the two packs against each other
        same = raw_d == raw_s
        vec0 = dc.PACK_VEC
        same[vec0:vec0 + 32 * 4] = True
        same[vec0 + dc.NCOL * 4:vec0 + (dc.NCOL + 32) * 4] = True
        assert same.all(), "%d bytes differ outside c / sc of the q columns" % int((~same).sum())
        for k in ("c", "sc"):
            a, b = ps[k][:32], pd[k][:32] * dc.SPT_QS
            assert (np.abs(a - b) <= 2.0 ** -24 * np.abs(b)).all(), k
        assert (ps["sc"][:32] != pd["sc"][:32]).all()
        # W' of the q columns of mpl_spt_pack carries SPT_QS
        errq = np.abs(ps["W"][:32] - W[:32] * dc.SPT_QS).max(1)
        assert (errq <= 2.0 ** -21 * colmax[:32] * dc.SPT_QS).all()
        # (printed, not asserted: the host's fp64 sum of c_n need not round as the device's does)
        host, written = dc.pack_host(w.sd, "blocks.%d" % l, 0)[0], dc.PACK_VEC + (2 * dc.NCOL + 8) * 4
        print("%s block %d: s_att 2^%d s_hid 2^%d, worst W' %.2f x 2^-24 of its column, worst c %.2f x 2^-24 of its terms; %d of the %d "
              "bytes written differ from the block packed on the host"
              % (which or "normal", l, dc.pow2_exponent(pd["s_att"]), dc.pow2_exponent(pd["s_hid"]),
                 float((np.abs(pd["W"] - W).max(1)[~zero] / colmax[~zero]).max() * 2 ** 24),
                 float((np.abs(pd["c"] - c) / terms).max() * 2 ** 24), int((host[:written] != raw_d[:written]).sum()), written))
