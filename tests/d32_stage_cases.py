"""Cases, weights, the D = 32 mistakes and the pack decoder of the stage check of the joints x views block kernels
(tests/test_d32_stage_gpu.py: csrc/d32_blocks.hip, the long kernels of csrc/token_attention.hip and spt_pack_kernel of
csrc/spt_packed.hip) and of its self-check (tests/test_d32_cases_cpu.py).  No pytest and no GPU needed to import.  Inputs, references,
measure and checker are those of tests/block_stack_cases.py (bs): rows of scales 2^-6 .. 2^6 with period 13, mpl_oracle.block along
the schedule in float64 and float32, both measures of rel_errors PER TOKEN ROW.

Weights: bs.make_stack(32, 2), and two copies with the scale sets of test_spt_split_operands_follow_the_weight_magnitudes applied
to every block (SCALE_SETS: qkv / proj / fc1 / fc2 / norm1 / norm2 up to 1e4 from their usual magnitudes, the products qkv x proj
and fc1 x fc2 near one); e32 is recomputed for those weights.

Bound IN FORCE, both kinds ("d32": the packed operand; "raw": the nn.Linear tensors, fp32 MFMA): the project's rule FACTOR x e32 =
4 x e32 in both row-wise measures, e32 = the float32 oracle's own worst row on the same case -- BOUND_FLOOR_D32 = 0, the fallback
max(SPT_BOUND, 4 x e32) is NOT used.  Measured on an MI355X the d32 kernels' worst row over the whole GPU file is 1.23 x e32 = 0.31
of the bound (the fp32-MFMA route: 1.32 x e32 = 0.33 of it): the terms that do not shrink with K = 32 (v_rsq_f32, exp2, the
Abramowitz-Stegun erf) stay below the float32 oracle's own rounding at this width.  Attention rows: 4 x the worst row of the same
formula evaluated by torch in float32 on the same inputs.  Pack: derived bounds only (the GPU file states them).

e32 per case family at D = 32, max-scaled / norm-wise, as two machines' float32 evaluations gave it (H = 8, schedule [0, 1, 1]
unless said; the value a test uses is the one it measures itself):
  n_tok 1, M 129                                         5.0e-7 / 3.6e-7
  n_tok 17, 16 sequences, H 8 / H 32                     3.5e-7 .. 4.0e-7 / 3.1e-7 .. 3.6e-7,  3.9e-7 / 3.1e-7
  n_tok 51, 5 sequences, H 8 / 4 / 2                     4.1e-7 .. 4.2e-7 / 3.0e-7 .. 3.5e-7,  3.5e-7 .. 3.9e-7 / 2.8e-7 .. 3.0e-7,  3.2e-7 / 2.8e-7
  n_tok 51, the sampled sequences of 1285 | 1286         3.8e-7 .. 4.3e-7 / 2.9e-7 .. 3.5e-7
  n_tok 527, the sampled sequences of 249                4.5e-7 .. 7.2e-7 / 3.6e-7 .. 4.9e-7
  schedules [0], [0, 1, 1], 12, 64 applications, n_tok 51   3.8e-7 .. 7.5e-7 / 2.7e-7 .. 5.0e-7
  magnitude sets big_qkv / small_qkv, n_tok 51           3.9e-7 / 3.1e-7,  4.5e-7 .. 5.0e-7 / 3.7e-7 .. 3.8e-7
  attention alone (torch float32 against float64), H 8   2.8e-7 / 2.4e-7 at 33 tokens .. 3.6e-6 / 2.0e-6 at 2048 (527: 1.5e-6 / 9.6e-7;
                                                         scores of about 60 at 527: 1.5e-5 / 6.3e-6);  H 4: 3.8e-7 / 3.2e-7 .. 2.6e-6 / 1.4e-6

The kernels' own worst rows as printed on an MI355X ("worst so far": PRINTED, NOT ASSERTED; no bound comes from them), max-scaled /
norm-wise, and the worst ratio to the e32 of the same case:
  d32 kernels, every block-level case                    6.7e-7 / 4.1e-7 (64 applications)      1.23 / 1.10 x e32
  fp32 MFMA on the nn.Linear tensors, K = 32             7.5e-7 / 4.2e-7                        1.32 / 1.19 x e32
  token_attention_long_p4_kernel, 33 .. 2048 tokens      3.9e-6 / 1.7e-6 (2048 tokens)          1.41 / 1.15 x float32 torch (at 512)
  token_attention_long_kernel, 33 .. 1024 tokens         3.0e-6 / 1.9e-6                        1.85 / 1.68 x float32 torch (at 49 / 769)
  long_p4, scores of about 60, 527 tokens                9.8e-6 / 5.2e-6                        0.66 / 0.82 x float32 torch
  packed operand: W' within 2.8 x 2^-24 of its column's maximum (bound 2^-21), c_n within 0.87 x 2^-24 of its terms (bound 2^-23);
  the bytes written by the device equal the block packed on the host by pack_host() in every case.
"""
import math

import numpy as np
import torch

from tests import block_stack_cases as bs
from tests.spt_stage_cases import SPT_BOUND

D = 32
TILE = 16                   # rows of a wave's tile (d32_blocks.hip)
WAVES = 512 * 8             # the grid cap: 512 workgroups of 8 waves; beyond WAVES tiles a wave walks a second tile
FACTOR = bs.FACTOR
# The bound of kind "d32": max(BOUND_FLOOR_D32, FACTOR x e32) per measure.  0.0 = the project's rule FACTOR x e32 alone; SPT_BOUND =
# the project's bound for this same packed arithmetic (tests/spt_stage_cases.py), admissible only while the CPU self-check rejects
# every mistake by 4 x under it.
BOUND_FLOOR_D32 = 0.0
BOUND_FLOOR_FALLBACK = SPT_BOUND

SCALE_SETS = dict(
    big_qkv=dict(qkv=64.0, proj=1 / 64.0, fc1=1e-3, fc2=1e3, g1=30.0, g2=0.02),
    small_qkv=dict(qkv=1e-4, proj=1e4, fc1=300.0, fc2=1 / 300.0, g1=0.01, g2=50.0),
)

# ----------------------------------------------------------------------------- cases of the GPU file (section 3 of its header)
TILE_EDGE_M = (1, 15, 16, 17, 127, 128, 129)                    # n_tok 1: a tile / a workgroup's eight tiles short, full, over
SHORT = dict(n_tok=17, n_seqs=(1, 8, 16), heads=(8, 32))        # LDS kernel; head dim 1: token_attention_any_kernel
LONG = dict(n_tok=51, n_seqs=(1, 3, 5), heads=(8, 4, 2))        # long_p4, long, wide
SECOND_TILE = dict(n_tok=51, n_seqs=(1285, 1286))               # M 65535 = 4096 tiles | 65586 = 4099 tiles + 2 rows
THIRD_TILE = dict(n_tok=527, n_seq=249)                         # M 131223, 8202 tiles
SCHED_12 = [i % 2 for i in range(12)]
SCHED_64 = [i % 2 for i in range(bs.MAX_APPS)]
SCHEDULES = ([0], bs.REFERENCE_SCHEDULE, SCHED_12, SCHED_64)
ATT_P4_NTOK = (33, 48, 49, 96, 97, 144, 145, 256, 257, 511, 512, 513, 527, 768, 769, 1025, 2047, 2048)
ATT_LONG_NTOK = (33, 49, 257, 513, 769, 1023, 1024)
ALL_NTOK = (1, 17, 51, 527)


def assert_rows_tell_apart(n_toks=ALL_NTOK):
    """bs.assert_rows_tell_apart for the 16-row tiles of the d32 kernels: the scale period is coprime to every sequence length and
    to the tile, so rows one sequence or one tile apart never share a scale."""
    e = bs.row_scale_exponents(4 * bs.SCALE_PERIOD)
    assert bool((e[1:] != e[:-1]).all()) and int(e.min()) == -6 and int(e.max()) == 6
    assert math.gcd(TILE, bs.SCALE_PERIOD) == 1 and math.gcd(TILE * WAVES, bs.SCALE_PERIOD) == 1
    for n in n_toks:
        assert n == 1 or n % bs.SCALE_PERIOD, n
        assert math.gcd(n, bs.SCALE_PERIOD) == 1, n


def sample_seqs(n_seq, n_tok):
    """The sequences of a large case that are compared: the first, the last, those that contain rows 65535 / 65536 and 131071 /
    131072 (the first row of a wave's second / third tile and the row before it) and eight others at fixed ninths."""
    M = n_seq * n_tok
    s = {0, n_seq - 1} | {r // n_tok for r in (65535, 65536, 131071, 131072) if r < M} | {(k * n_seq) // 9 for k in range(1, 9)}
    return sorted(s)


# ----------------------------------------------------------------------------- weights
def make_stack32(scale_set=None, depth=2):
    """(module on the CPU, state dict) of bs.make_stack(32, depth), with one of SCALE_SETS applied to every block."""
    m, sd = bs.make_stack(D, depth)
    if scale_set is None:
        return m, sd
    s = SCALE_SETS[scale_set]
    with torch.no_grad():
        for blk in m.blocks:
            blk.attn.qkv.weight.mul_(s["qkv"]); blk.attn.qkv.bias.mul_(s["qkv"])
            blk.attn.proj.weight.mul_(s["proj"])
            blk.mlp.fc1.weight.mul_(s["fc1"]); blk.mlp.fc1.bias.mul_(s["fc1"])
            blk.mlp.fc2.weight.mul_(s["fc2"])
            blk.norm1.weight.mul_(s["g1"]); blk.norm1.bias.mul_(s["g1"])
            blk.norm2.weight.mul_(s["g2"]); blk.norm2.bias.mul_(s["g2"])
    return m, {k: v.detach().clone() for k, v in m.state_dict().items()}


def bound(e32, floor):
    """The pair check_rows divides by FACTOR again: max(floor, FACTOR x e32) per measure."""
    return (max(e32[0], floor / FACTOR), max(e32[1], floor / FACTOR))


def check_rows(got, ref64, e32, floor=0.0):
    return bs.check_rows(got, ref64, bound(e32, floor))


# ----------------------------------------------------------------------------- the packed block (csrc/spt_pack.hpp), restated
PACK_BYTES, PACK_VEC = 48 * 1024, 32 * 1024
NCOL = 224
C_QKV, C_PROJ, C_FC1, C_FC2 = 0, 96, 128, 192
SPT_SA = 1024.0
SPT_QS = float(np.float32(0.5) * np.float32(1.4426950408889634))    # hd^-0.5 log2 e as the kernel holds it (float32)
# unit -> (first column of its 16-column tile, k step): 6 qkv, 2 proj, 4 fc1, 4 fc2 = [n tile][k step]
UNITS = ([(C_QKV + 16 * n, 0) for n in range(6)] + [(C_PROJ + 16 * n, 0) for n in range(2)] + [(C_FC1 + 16 * n, 0) for n in range(4)]
         + [(C_FC2 + 16 * n, ks) for n in range(2) for ks in range(2)])


def pow2_exponent(v):
    """e with v == 2^e, or None."""
    m, e = math.frexp(float(v))
    return e - 1 if m == 0.5 else None


def decode_pack(raw):
    """The 48-KiB block as the kernels read it -> dict(frag (224, 64) float64: (hi + lo) of column n at input k (columns of K = 32 hold
    zeros beyond 32), hi, lo (the two parts alone), c (224,), sc (224,), s_att, s_hid, tail (the six unused scalars), W (224, 64):
    frag x sc x input scale -- the effective weight W' (gamma folded; times SPT_QS in the q columns of mpl_spt_pack))."""
    raw = np.ascontiguousarray(np.asarray(raw, dtype=np.uint8).reshape(-1))
    assert raw.size == PACK_BYTES, raw.size
    f = raw[:PACK_VEC].view(np.float16).reshape(16, 2, 64, 8).astype(np.float64)     # [unit][hi | lo][lane][8]
    hi, lo = np.zeros((NCOL, 64)), np.zeros((NCOL, 64))
    for u, (n0, ks) in enumerate(UNITS):
        for lane in range(64):
            li, kq = lane & 15, lane >> 4
            hi[n0 + li, 32 * ks + 8 * kq: 32 * ks + 8 * kq + 8] = f[u, 0, lane]
            lo[n0 + li, 32 * ks + 8 * kq: 32 * ks + 8 * kq + 8] = f[u, 1, lane]
    vec = raw[PACK_VEC:].view(np.float32)
    c, sc = vec[:NCOL].astype(np.float64), vec[NCOL:2 * NCOL].astype(np.float64)
    s_att, s_hid = float(vec[2 * NCOL]), 2.0 * float(vec[2 * NCOL + 1])
    in_scale = np.full(NCOL, SPT_SA)
    in_scale[C_PROJ:C_FC1] = s_att
    in_scale[C_FC2:] = s_hid
    return dict(frag=hi + lo, hi=hi, lo=lo, c=c, sc=sc, s_att=s_att, s_hid=s_hid, tail=vec[2 * NCOL + 2:2 * NCOL + 8].copy(),
                rest=raw[PACK_VEC + (2 * NCOL + 8) * 4:].copy(), in_scale=in_scale, W=(hi + lo) * (sc * in_scale)[:, None])


def _window_scale(v):
    """Largest power of two p with p v <= 2^15 (spt_window_scale); 1 for v == 0."""
    if not (v > 0 and math.isfinite(v)):
        return 1.0
    p = 2.0 ** math.floor(math.log2(32768.0 / v))
    while p * v > 32768.0:
        p /= 2
    while 2 * p * v <= 32768.0:
        p *= 2
    return p


def pack_terms(sd, prefix):
    """float64: (W' (224, 64): gamma folded, zero beyond K; c (224,); sum |terms| of c (224,); the bound sqrt(32) |W'_n|_2 + |c_n| of
    the LayerNorm columns (224,), 0 elsewhere) of a block -- the formulas in the header of spt_pack_kernel."""
    g = lambda k: sd[prefix + "." + k].double().numpy()
    W, c, terms, bnd = np.zeros((NCOL, 64)), np.zeros(NCOL), np.zeros(NCOL), np.zeros(NCOL)
    for n0, lin, ln in ((C_QKV, "attn.qkv", "norm1"), (C_PROJ, "attn.proj", None), (C_FC1, "mlp.fc1", "norm2"), (C_FC2, "mlp.fc2", None)):
        w, b = g(lin + ".weight"), g(lin + ".bias")
        N, K = w.shape
        sl = slice(n0, n0 + N)
        c[sl], terms[sl] = b, np.abs(b)
        if ln:
            gam, bet = g(ln + ".weight"), g(ln + ".bias")
            W[sl, :K] = w * gam[None, :]
            c[sl] += (w * bet[None, :]).sum(1)
            terms[sl] += np.abs(w * bet[None, :]).sum(1)
            bnd[sl] = math.sqrt(32.0) * np.sqrt((W[sl] ** 2).sum(1)) + np.abs(c[sl])
        else:
            W[sl, :K] = w
    return W, c, terms, bnd


def pack_host(sd, prefix, fold_q):
    """The packed block built on the host from the same formulas (float64 where the kernel uses float32 for W x gamma: the
    decoder's round trip does not depend on it) -> (bytes (49152,) uint8, dict of what went in: hi, lo, c, sc, s_att, s_hid)."""
    W, c, _, bnd = pack_terms(sd, prefix)
    W = W.astype(np.float32)
    amax = np.abs(W).max(1)
    sw = np.ones(NCOL)
    nz = amax > 0
    sw[nz] = 2.0 ** (14 - (np.frexp(amax[nz])[1]))
    s_att, s_hid = _window_scale(float(bnd[64:96].max())), _window_scale(float(bnd[C_FC1:C_FC2].max()))
    in_scale = np.full(NCOL, SPT_SA)
    in_scale[C_PROJ:C_FC1] = s_att
    in_scale[C_FC2:] = s_hid
    sc = (1.0 / (in_scale * sw)).astype(np.float32)
    c32 = c.astype(np.float32)
    if fold_q:
        sc[:32] = sc[:32] * np.float32(SPT_QS)
        c32[:32] = c32[:32] * np.float32(SPT_QS)
    x = (W.astype(np.float64) * sw[:, None]).astype(np.float32)          # exact: a power of two
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    frag = np.zeros((16, 2, 64, 8), dtype=np.float16)
    for u, (n0, ks) in enumerate(UNITS):
        for lane in range(64):
            li, kq = lane & 15, lane >> 4
            frag[u, 0, lane] = hi[n0 + li, 32 * ks + 8 * kq: 32 * ks + 8 * kq + 8]
            frag[u, 1, lane] = lo[n0 + li, 32 * ks + 8 * kq: 32 * ks + 8 * kq + 8]
    vec = np.zeros((PACK_BYTES - PACK_VEC) // 4, dtype=np.float32)
    vec[:NCOL], vec[NCOL:2 * NCOL] = c32, sc
    vec[2 * NCOL], vec[2 * NCOL + 1] = s_att, 0.5 * s_hid
    raw = np.concatenate([frag.reshape(-1).view(np.uint8), vec.view(np.uint8)])
    return raw, dict(hi=hi.astype(np.float64), lo=lo.astype(np.float64), c=c32.astype(np.float64), sc=sc.astype(np.float64),
                     s_att=s_att, s_hid=s_hid, sw=sw)


# ----------------------------------------------------------------------------- constructed mistakes at D = 32
def _fp16_part(w, sd_gamma=None):
    """W (gamma folded when given) rounded to ONE fp16 part after its power-of-two column scale (max |W'_n| sw_n in [2^13, 2^14))."""
    wf = w if sd_gamma is None else w * sd_gamma[None, :]
    amax = wf.abs().amax(1).clamp_min(1e-300)
    sw = torch.pow(2.0, 14 - torch.frexp(amax)[1].double())
    return (wf * sw[:, None]).to(torch.float16).double() / sw[:, None]


def mutant_block32(x, sd, p, H, mistake=None):
    """Block.forward in float64 on x (S, n, 32), restated op by op so that one step can be done the way a D = 32 kernel could get
    it wrong (None: no mistake)."""
    S, n, Dm = x.shape
    hd = Dm // H
    F = torch.nn.functional
    one_part = mistake == "weights_one_fp16_part"

    def ln_linear(x, ln, lin):
        w, b = sd[p + lin + ".weight"], sd[p + lin + ".bias"]
        if not one_part:
            return F.linear(F.layer_norm(x, (Dm,), sd[p + ln + ".weight"], sd[p + ln + ".bias"], 1e-6), w, b)
        z = F.layer_norm(x, (Dm,), None, None, 1e-6)            # gamma lives in W', beta in c_n = b_n + sum_k beta_k W_nk
        return F.linear(z, _fp16_part(w, sd[p + ln + ".weight"]), b + w @ sd[p + ln + ".bias"])

    def linear(x, lin):
        w = sd[p + lin + ".weight"]
        return F.linear(x, _fp16_part(w) if one_part else w, sd[p + lin + ".bias"])

    qkv = ln_linear(x, ".norm1", ".attn.qkv").reshape(S, n, 3, H, hd).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    scale = hd ** -0.5
    if mistake == "q_scaled_twice":
        scale = scale * scale
    sc = (q @ k.transpose(-2, -1)) * scale
    if mistake == "zero_partner_of_odd_last_key_in_softmax" and n % 2:
        # the pair kernel pads an odd last key with k = v = 0: score 0, weight exp(0 - max) instead of none
        att = torch.cat([sc, torch.zeros_like(sc[..., :1])], -1).softmax(-1)[..., :n]
    else:
        att = sc.softmax(-1)
    y = (att @ v).transpose(1, 2).reshape(S, n, Dm)
    if mistake == "attention_across_first_boundary" and S >= 2:
        # the first two sequences attend as one of 2 n tokens
        q2, k2, v2 = (t[:2].transpose(0, 1).reshape(1, H, 2 * n, hd) for t in (q, k, v))
        y2 = (((q2 @ k2.transpose(-2, -1)) * scale).softmax(-1) @ v2).transpose(1, 2).reshape(2, n, Dm)
        y = torch.cat([y2, y[2:]])
    if mistake == "rows_16_31_from_attention_rows_of_tile_0" and S * n >= 2 * TILE:
        y = y.reshape(S * n, Dm).clone()
        y[TILE:2 * TILE] = y[:TILE]
        y = y.reshape(S, n, Dm)
    a = linear(y, ".attn.proj")
    if mistake == "proj_columns_16_31_left_at_residual":
        a = a.clone()
        a[..., 16:32] = 0
    x = x + a
    h = F.gelu(ln_linear(x, ".norm2", ".mlp.fc1"))
    return x + linear(h, ".mlp.fc2")


NEW_MISTAKES = ("attention_across_first_boundary", "proj_columns_16_31_left_at_residual", "rows_16_31_from_attention_rows_of_tile_0",
                "zero_partner_of_odd_last_key_in_softmax", "q_scaled_twice", "weights_one_fp16_part")
# of bs.MISTAKES, attention_across_sequences and proj_slice_left_at_residual (columns 136 .. 271) are no-ops at this width;
# fc2_last_32_inputs_dropped is exactly unit w2[n][1], the second k step of fc2
BS_MISTAKES = tuple(m for m in bs.MISTAKES if m not in ("attention_across_sequences", "proj_slice_left_at_residual"))
MISTAKES = NEW_MISTAKES + BS_MISTAKES


def mutant_stack32(sd, x, n_tok, H, schedule, mistake=None):
    """The float64 stack with one constructed mistake (None: none -- must equal bs.reference())."""
    if mistake in BS_MISTAKES:
        return bs.mutant_stack(sd, x, n_tok, H, schedule, mistake)
    s = bs.cast_sd(sd, torch.float64)
    y = x.double().reshape(-1, n_tok, D)
    with torch.no_grad():
        for l in schedule:
            y = mutant_block32(y, s, "blocks.%d" % l, H, mistake)
    return y.reshape(-1, D)
