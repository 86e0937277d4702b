"""Cases, inputs, float64 / float32 references and the row-wise checker of the block-stack stage check
(tests/test_block_stack_stage_gpu.py) and of its self-check (tests/test_block_stack_cases_cpu.py).  No pytest and no GPU needed to
import.

Weights: bare Blocks (multiview_mpl.Block, mlp_ratio 2, qkv bias) under the names blocks.{l}, filled by detrng.fill_module_: LayerNorm
gains U(0.5, 1.5), offsets N(0, 0.1), Linear biases U(+-1/sqrt(fan_in)) -- the builder asserts that none of them is trivial (the fp16x2
operands fold gamma into W and beta into c_n: a stack with gamma = 1, beta = 0 would not notice a fold that was left out).  The
tensors do not depend on the head count or the sequence length: one set per (width, depth), packed once per precision.

Input rows x (M, D): row r = 2^e(r) (u_r + m(r)), u_r ~ N(0, 1) per element (detrng, element (r, c) a function of r D + c: the first
n rows of a longer input ARE the shorter input), e(r) = 5 r mod 13 - 6 (powers of two over 2^-6 .. 2^6; neighbouring rows are 2^5
or 2^-8 apart; period 13, coprime to every sequence length and to the 60 / 62 / 63 / 64 rows of a tile, so rows one sequence or one
tile apart never share a scale) and m(r) = (3 r mod 7 - 3) / 4 (mean offsets of up to 0.75 sigma).  A row, sequence, head or tile
mix-up is an O(1) error on the smaller of the rows involved.

Reference: mpl_oracle.block (block_bf16 for the bf16 engines: the engine's own rounding points) along the schedule, in float64 and
again in float32, once per case at the largest M; sequences are independent, so rows [0 : n] are the stack of the first n rows alone.

Error measure: both measures of mpl_oracle.rel_errors taken PER TOKEN ROW (|d|_max / |ref row|_max and |d|_2 / |ref row|_2), the
worst row of each.  Bound: FACTOR x e32 in each measure, e32 = the float32 oracle's own worst per-row error against float64 on the
same case -- a property of the reference (for bf16: the float32 evaluation of the bf16-operand emulation against its float64
evaluation, i.e. the operands that sit within fp32 noise of a bf16 rounding boundary and round the other way; see the comment in
test_bf16_matmul_path).  FACTOR = 4 is the project's factor (spt_stage_cases.E32_FACTOR).

e32 per case family, measured on the CPU at the largest M of each case, max-scaled / norm-wise (smallest .. largest case):
  fp16x2 teams D 544, H 8, schedule [0, 1, 1], n_tok 1 .. 32      7.1e-7 .. 8.9e-7 / 6.3e-7 .. 7.1e-7
  head dims D 544 hd 4 / 8 / 136, D 1088 hd 68 / 136              7.1e-7 .. 1.0e-6 / 6.1e-7 .. 8.1e-7
  widths 1088 .. 3808, one block, [0, 0]                          6.2e-7 .. 8.5e-7 / 5.7e-7 .. 6.7e-7
  small engine D 128 .. 1088                                      5.6e-7 .. 9.2e-7 / 4.5e-7 .. 7.5e-7
  schedules [0] .. 64 applications                                6.9e-7 .. 8.1e-7 / 4.4e-7 .. 6.2e-7
  bf16 emulation D 544 / 1088 (and D 544, H 16: 2.6e-3 / 2.4e-3)  2.0e-3 .. 3.1e-3 / 1.8e-3 .. 2.8e-3
(the whole-tensor measures of the same float32 oracle are 1.5e-7 / 6e-8 at D 544: the row-wise ones are set by the rows of small
scale, whose output is the sum of block outputs that cancel in part.)

The kernels' own worst row per engine over the whole GPU file, as printed on an MI355X ("worst so far": PRINTED, NOT ASSERTED; the
bound does not come from them), max-scaled / norm-wise:
  fp16x2 teams (every form, D 544 / 1088, head dims 4 .. 136)     1.3e-6 / 9.5e-7      (D 544, H 8 alone: 9.1e-7 / 7.5e-7)
  small engine                                                    7.4e-7 / 5.1e-7
  fp32 MFMA on the nn.Linear tensors (UNPACKED), D 544 .. 3808    1.7e-6 / 1.4e-6      (one accumulator chain up to K = 2176, chunks of
                                                                  512 columns beyond; one chain at any K: 3.4e-6 / 2.2e-6 at D 3808)
  bf16 teams / bf16 shape-general (against the emulation)         2.7e-3 / 2.7e-3 and 2.2e-3 / 2.2e-3
"""
import math

import torch
from torch import nn

from openmpl_amd import detrng
from openmpl_amd.multiview_mpl import Block
from oracle import mpl_oracle

FACTOR = 4              # the project's factor on the float32 reference's own error (spt_stage_cases.E32_FACTOR)
WSEED, XSEED = 41, 43
SCALE_PERIOD, OFFSET_PERIOD = 13, 7
BM, BN = 64, 136        # rows of a whole tile, columns of a slice (csrc/gemm_common.hpp)
MAX_APPS = 64           # MPL_MAX_APPS

TEAM_NTOK = (1, 2, 3, 4, 5, 7, 8, 16, 31, 32)
BF16_NTOK = (1, 2, 5, 8, 31, 32)
SMALL_NTOK = (1, 2, 3, 5, 8, 16)
# (D, H, packed operands beside the tensors): head dims 16, 36, 68, 136, 272.  128 is the narrowest width the engine takes, 144 has
# nine 16-deep k-steps for eight waves, 1088 is the widest (68 k-steps: 8.5 per wave, the last wave's steps beyond K run on zeroed
# operands) -- sm_stack_ok admits D <= 1152 by its k-step count, but two 16 x 2 D weight tiles of fc2 must fit 136 KiB of LDS: D <= 1088
SMALL_SHAPES = ((128, 8, False), (144, 4, False), (544, 8, True), (1088, 8, True), (1088, 4, False))
HEAD_DIM_SHAPES = ((544, 4), (544, 68), (544, 136), (1088, 8), (1088, 16))  # (D, H): head dims 136, 8, 4, 136, 68
WIDTH_SHAPES = tuple((D, D // hd) for D in (1088, 1632, 2176, 3808) for hd in (68, 136))
SCHEDULES = ([0], [0, 0], [1, 0, 1, 1, 0], [(i * 5 // 3) % 2 for i in range(MAX_APPS)])
REFERENCE_SCHEDULE = [0, 1, 1]      # depth 2 as the reference applies it: the last block twice


# ----------------------------------------------------------------------------- weights
class Stack(nn.Module):
    """`depth` bare Blocks of width D under the state-dict names blocks.{l}.* -- what mpl_oracle.block reads."""

    def __init__(self, D, depth):
        super().__init__()
        self.blocks = nn.ModuleList([Block(dim=D, num_heads=1, mlp_ratio=2.0, qkv_bias=True) for _ in range(depth)])


def make_stack(D, depth, seed=WSEED):
    """(module on the CPU, its state dict as float32 CPU tensors); asserts that no LayerNorm gain / offset and no bias is trivial."""
    m = detrng.fill_module_(Stack(D, depth), seed=seed).eval()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    for k, v in sd.items():
        if k.endswith(("norm1.weight", "norm2.weight")):
            assert float((v - 1).abs().mean()) > 0.1 and float(v.std()) > 0.1, k + ": LayerNorm gain is (nearly) 1"
        elif k.endswith(("norm1.bias", "norm2.bias")):
            assert float(v.abs().mean()) > 0.02 and float(v.std()) > 0.02, k + ": LayerNorm offset is (nearly) 0"
        elif k.endswith(".bias"):
            assert float(v.abs().mean()) > 0.1 / math.sqrt(v.numel()) and float(v.std()) > 0, k + ": bias is (nearly) 0"
    return m, sd


# ----------------------------------------------------------------------------- input rows
def row_scale_exponents(M):
    return (5 * torch.arange(M)) % SCALE_PERIOD - 6


def row_offsets(M):
    return ((3 * torch.arange(M)) % OFFSET_PERIOD - 3).double() / 4


def make_rows(M, D, seed=XSEED):
    u = torch.from_numpy(detrng.normal(seed, "block_stack.x.%d" % D, (M, D), 0.0, 1.0)).double()
    x = (u + row_offsets(M)[:, None]) * torch.pow(2.0, row_scale_exponents(M).double())[:, None]
    return x.float()


def assert_rows_tell_apart(n_toks):
    """The scale period is coprime to every sequence length and tile height in use: rows one sequence / one tile apart differ in
    scale, and so do neighbouring rows."""
    e = row_scale_exponents(4 * SCALE_PERIOD)
    assert bool((e[1:] != e[:-1]).all()) and int(e.min()) == -6 and int(e.max()) == 6
    for n in n_toks:
        for step in (n, (BM // n) * n):
            assert math.gcd(step, SCALE_PERIOD) == 1, (n, step)


# ----------------------------------------------------------------------------- references
def cast_sd(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


def reference(sd, x, n_tok, H, schedule, dtype=torch.float64, bf16=False):
    """The stack along `schedule` on rows x (M, D), M a multiple of n_tok, evaluated in `dtype` -> (M, D) in `dtype`."""
    D = x.shape[1]
    s = cast_sd(sd, dtype)
    y = x.to(dtype).reshape(-1, n_tok, D)
    fn = mpl_oracle.block_bf16 if bf16 else mpl_oracle.block
    with torch.no_grad():
        for l in schedule:
            y = fn(y, s, "blocks.%d" % l, H)
    return y.reshape(-1, D)


def references(sd, x, n_tok, H, schedule, bf16=False):
    """(float64 rows, e32 = (max-scaled, norm-wise) worst per-row error of the float32 evaluation against them)."""
    ref64 = reference(sd, x, n_tok, H, schedule, torch.float64, bf16)
    ref32 = reference(sd, x, n_tok, H, schedule, torch.float32, bf16)
    return ref64, worst_row_errors(ref32, ref64), ref32


# ----------------------------------------------------------------------------- measure and checker
def row_errors(out, ref):
    """Per token row: (|out - ref|_max / |ref|_max, |out - ref|_2 / |ref|_2), two (M,) float64 tensors."""
    o, r = out.double(), ref.double()
    d = o - r
    mx = d.abs().amax(1) / r.abs().amax(1).clamp_min(1e-30)
    nw = torch.linalg.norm(d, dim=1) / torch.linalg.norm(r, dim=1).clamp_min(1e-30)
    return mx, nw


def worst_row_errors(out, ref):
    mx, nw = row_errors(out, ref)
    return float(mx.max()), float(nw.max())


def check_rows(got, ref64, e32, factor=FACTOR):
    """None when every row of `got` is finite and within factor x e32 of ref64 in both measures, else one line saying what is off
    (NaN compares false: it fails)."""
    if tuple(got.shape) != tuple(ref64.shape):
        return "shape %s, expected %s" % (tuple(got.shape), tuple(ref64.shape))
    if not bool(torch.isfinite(got).all()):
        return "%d non-finite elements" % int((~torch.isfinite(got)).sum())
    mx, nw = row_errors(got, ref64)
    ok = (mx <= factor * e32[0]) & (nw <= factor * e32[1])
    if bool(ok.all()):
        return None
    bad = (~ok).nonzero().flatten()
    return ("worst row max-scaled %.3e norm-wise %.3e, bound %d x (%.3e, %.3e); %d rows off, first %s"
            % (float(mx.max()), float(nw.max()), factor, e32[0], e32[1], bad.numel(), bad[:8].tolist()))


# ----------------------------------------------------------------------------- batches of the team kernels
def rows_per_tile(n_tok):
    return (BM // n_tok) * n_tok


def tail_n_seqs(n_tok, n_tiles):
    """n_seq whose last of n_tiles row tiles is full, holds one sequence, and holds S - 1 sequences (S = sequences per tile)."""
    S = BM // n_tok
    return sorted({(n_tiles - 1) * S + k for k in (S, 1, S - 1) if k >= 1})


# stack-mode bits (mpl_x3_stack_mode) that force each team form of the fp16x2 engine; bit 3 keeps the call off the small engine
MODE_NO_SMALL = 8
FORCE_MODES = dict(TEAMS=(1 << 5) | (1 << 1), PAIRS=2 << 1, ROWS32=2 << 5, ROWS16=(3 << 5) | 16, ROWS16_DIRECT=3 << 5, PER_GEMM=1)


def narrow_legal(n_tok):
    """Row-narrow teams exist where a tile has 64 rows and a 16-row group holds whole sequences (h2_phase.hpp h2_stack_form)."""
    return rows_per_tile(n_tok) == BM and 16 % n_tok == 0


# ----------------------------------------------------------------------------- the small engine's layout, restated
def small_groups(n_seq, n_tok, D, cus):
    """(groups of sequences, sequences per full group) of a small-engine launch: csrc/sm_stack.hip sm_stack_groups restated, 0 groups
    where the engine does not take the launch for its layout."""
    if n_tok > 16 or D % 16:
        return 0, 0
    tiles, fit = 3 * D // 16, 16 // n_tok
    g_min = -(-n_seq // fit)
    if g_min <= 2 and (2 if n_seq >= 2 else 1) * tiles <= cus:
        g = 2 if n_seq >= 2 else 1
    elif g_min == 1 and tiles <= cus:
        g = 1
    else:
        half = (tiles + 1) // 2
        if 256 * D > 136 * 1024 or D // 16 > half or g_min * half > cus:
            return 0, 0
        g = min(cus // half, n_seq)
    spg = -(-n_seq // g)
    return -(-n_seq // spg), spg


# ----------------------------------------------------------------------------- constructed mistakes (the checker's self-check)
def _ln(x, sd, p, beta=True):
    y = torch.nn.functional.layer_norm(x, (x.shape[-1],), sd[p + ".weight"], sd[p + ".bias"] if beta else None, 1e-6)
    return y


def _lin(x, sd, p):
    return torch.nn.functional.linear(x, sd[p + ".weight"], sd[p + ".bias"])


def mutant_block(x, sd, p, H, mistake=None):
    """Block.forward in the dtype of x (S, n, D), restated op by op so that one step can be done wrongly."""
    S, n, D = x.shape
    hd = D // H
    qkv = _lin(_ln(x, sd, p + ".norm1"), sd, p + ".attn.qkv").reshape(S, n, 3, H, hd).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2].clone()
    if mistake == "v_of_next_head":
        v[:, 2] = qkv[2][:, 3]
    scale = (D // (H // 2)) ** -0.5 if mistake == "scale_of_wrong_head_dim" else hd ** -0.5
    att = ((q @ k.transpose(-2, -1)) * scale).softmax(dim=-1)
    a = _lin((att @ v).transpose(1, 2).reshape(S, n, D), sd, p + ".attn.proj")
    if mistake == "proj_slice_left_at_residual":
        a[..., BN:2 * BN] = 0
    x = x + a
    h = torch.nn.functional.gelu(_lin(_ln(x, sd, p + ".norm2", beta=mistake != "norm2_beta_omitted"), sd, p + ".mlp.fc1"),
                                 approximate="tanh" if mistake == "tanh_gelu" else "none")
    if mistake == "fc2_last_32_inputs_dropped":
        h = h.clone()
        h[..., -32:] = 0
    return x + _lin(h, sd, p + ".mlp.fc2")


def mutant_stack(sd, x, n_tok, H, schedule, mistake=None):
    """The float64 stack with one constructed mistake (None: no mistake -- must equal reference())."""
    D, M = x.shape[1], x.shape[0]
    s = cast_sd(sd, torch.float64)
    if mistake == "schedule_shifted":
        schedule = list(schedule[1:]) + list(schedule[:1])
    y = x.double().reshape(-1, n_tok, D)
    with torch.no_grad():
        for l in schedule:
            p = "blocks.%d" % l
            if mistake == "attention_across_sequences":
                # the first 32 rows attend as sequences of 2 n_tok tokens: every second boundary is ignored
                rows = y.reshape(M, D)
                k = (32 // (2 * n_tok)) * 2 * n_tok
                y = torch.cat([mutant_block(rows[:k].reshape(-1, 2 * n_tok, D), s, p, H).reshape(k, D),
                               mutant_block(rows[k:].reshape(-1, n_tok, D), s, p, H).reshape(M - k, D)]).reshape(-1, n_tok, D)
            else:
                y = mutant_block(y, s, p, H, mistake)
    out = y.reshape(M, D).clone()
    if mistake == "neighbour_sequences_exchanged":
        out[n_tok:2 * n_tok], out[2 * n_tok:3 * n_tok] = y.reshape(M, D)[2 * n_tok:3 * n_tok], y.reshape(M, D)[n_tok:2 * n_tok]
    if mistake == "last_sequence_unwritten":
        out[M - n_tok:] = x.double()[M - n_tok:]
    return out


MISTAKES = ("neighbour_sequences_exchanged", "attention_across_sequences", "v_of_next_head", "scale_of_wrong_head_dim",
            "fc2_last_32_inputs_dropped", "norm2_beta_omitted", "tanh_gelu", "proj_slice_left_at_residual", "schedule_shifted",
            "last_sequence_unwritten")
