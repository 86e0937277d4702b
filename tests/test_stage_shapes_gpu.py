"""The shape-general kernels against float64 at their tile and envelope edges.

Every kernel result here is compared with a float64 torch reference of the same operation (max-scaled and norm-wise relative
error, mpl_oracle.rel_errors): 2e-6 for a single stage, 1e-4 for a whole forward.  Outputs start NaN-filled, so an element a
kernel never writes fails.  The comment on each case names the launcher route it takes (csrc/ln_gemm.hip launch_ln_gemm /
launch_ng_auto / launch_row_stats, csrc/token_attention.hip launch_token_attention, csrc/fuse_head.hip launch_fuse_head and
fuse_head.hpp fh_params).
"""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from openmpl_amd import cabi, detrng
from openmpl_amd.multiview_mpl import MultiView_MPL
from oracle import mpl_oracle
from tests.golden.cases import CASES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4          # whole forward
STAGE_TOL = 2e-6    # one stage
E_UNSUPPORTED = -2


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _assert_close(out, ref, what, tol):
    mx, nw = mpl_oracle.rel_errors(out.detach().cpu(), ref.detach().cpu())
    assert mx <= tol and nw <= tol, "%s: max-scaled %.3e norm-wise %.3e (tol %.0e)" % (what, mx, nw, tol)


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _launches(fn):
    """(result or raised exception, number of kernels launched while fn ran)."""
    cabi.profile_start()
    try:
        res = fn()
    except Exception as e:      # noqa: BLE001 -- handed back to the caller, which asserts on it
        res = e
    finally:
        torch.cuda.synchronize()
        counts = cabi.profile_stop()
    return res, sum(n for _, n in counts.values())


# ----------------------------------------------------------------------------- 1. mpl_ln_linear
B_, G_, R_ = cabi.EPI_BIAS, cabi.EPI_BIAS_GELU, cabi.EPI_BIAS_RESIDUAL
LN_CASES = [
    # M, K, N, epilogue, LayerNorm, residual aliases y, rows of mean 1e3 / std 1e-2
    # ln_gemm_any_kernel (K % 32 != 0); statistics: row_stats_any_kernel (K & 3), row_stats_kernel (K & 3 == 0)
    (1, 1, 1, B_, True, False, False),          # any-K, one element; row_stats_any
    (63, 3, 64, G_, True, False, False),        # any-K, one row tile short by one row, one whole column tile; row_stats_any
    (65, 5, 65, R_, False, True, False),        # any-K, one row / column past a 64 tile, y aliased as residual
    (129, 31, 135, B_, True, False, False),     # any-K, k one short of a 32-chunk, 3 x 3 tiles; row_stats_any
    (64, 33, 137, G_, True, False, False),      # any-K, 2 k chunks (1 into the second); row_stats_any
    (4000, 34, 480, R_, True, False, True),     # any-K, 63 row tiles, 7.5 column tiles; row_stats_any; large-mean rows
    (129, 136, 63, B_, True, False, False),     # any-K (136 % 32 = 8); row_stats_kernel, K % 136 == 0: one 136 slice
    (65, 272, 1440, G_, True, False, False),    # any-K; row_stats_kernel two 136 slices -> ln_combine of 2 partials
    (4000, 272, 65, B_, True, False, True),     # any-K, 2 slices, large-mean rows through ln_combine
    (63, 4095, 3, R_, True, True, False),       # any-K, 128 k chunks, last one 31 deep; row_stats_any one slice; alias
    # launch_ng_auto (K % 32 == 0)
    (129, 32, 63, B_, True, False, False),      # row_stats32_kernel; column-split ln_gemm_cs_kernel (3 workgroups)
    (1, 480, 1, B_, True, False, False),        # row_stats_kernel one slice (480 % 136 != 0); cs kernel, one row, one column
    (63, 480, 1440, G_, True, False, False),    # one slice; cs kernel (11 workgroups <= 256), N = 10.6 tiles
    (4000, 4096, 480, R_, True, True, False),   # one slice K = 4096; cs kernel (252 workgroups <= 256); alias
    (4000, 480, 1000, G_, False, False, False),  # cs kernel, 504 workgroups (<= 512, not residual)
    (4000, 480, 1000, R_, True, False, False),  # 504 residual workgroups -> ln_gemm_ng_kernel NG = 1, 2-stage ring
    (4000, 480, 2000, B_, True, False, False),  # 945 workgroups -> NG = 1, 3-stage ring (cost(3) > cost(2))
    (4000, 480, 2040, G_, True, False, False),  # N % 408 == 0, 63 x 5 >= 256 workgroups -> NG = 3
    (64, 1088, 137, R_, True, False, False),    # row_stats_kernel eight 136 slices; cs kernel, N one past a 136 tile
    (129, 1088, 137, B_, True, False, True),    # eight slices with large-mean rows
]


def _ln_ids(c):
    return "M%d-K%d-N%d-e%d%s%s%s" % (c[0], c[1], c[2], c[3], "-ln" if c[4] else "", "-alias" if c[5] else "", "-bigmean" if c[6] else "")


@pytest.mark.parametrize("M,K,N,epi,ln,alias,bigmean", LN_CASES, ids=[_ln_ids(c) for c in LN_CASES])
def test_ln_linear_any_shape_matches_fp64(M, K, N, epi, ln, alias, bigmean):
    lib = cabi.load()
    g = torch.Generator().manual_seed(M * 31 + K * 7 + N)
    x = torch.randn(M, K, generator=g) * 1.5 + 0.3
    big = torch.zeros(M, dtype=torch.bool)
    if bigmean:
        big[::5] = True
        x[big] = 1e3 + 1e-2 * torch.randn(int(big.sum()), K, generator=g)
    W = (torch.rand(N, K, generator=g) * 2 - 1) * K ** -0.5
    b = torch.randn(N, generator=g)
    lw, lb = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g) * 0.1
    res = torch.randn(M, N, generator=g)
    xd, Wd, Ld = (t.to(DEV) for t in (x, W, torch.stack([lw, lb])))
    bd = b.to(DEV)
    y = res.to(DEV) if alias else _nan(M, N)
    r = y if alias else res.to(DEV)
    stats = _nan(2 * M * max(1, K // 136))
    rc = lib.mpl_ln_linear(xd.data_ptr(), M, K, Ld[0].data_ptr() if ln else None, Ld[1].data_ptr() if ln else None, 1e-6,
                           Wd.data_ptr(), bd.data_ptr(), N, epi, r.data_ptr() if epi == R_ else None, y.data_ptr(),
                           stats.data_ptr(), _stream())
    cabi.check(rc, "mpl_ln_linear")

    def ref(dt):
        a = x.to(dt)
        if ln:
            a = F.layer_norm(a, (K,), lw.to(dt), lb.to(dt), 1e-6)
        o = a @ W.to(dt).t() + b.to(dt)
        if epi == G_:
            o = F.gelu(o)
        return o + res.to(dt) if epi == R_ else o

    r64, out = ref(torch.float64), y.cpu()
    _assert_close(out[~big], r64[~big], "ln_linear", STAGE_TOL)
    if bigmean:
        # mean 1e3, spread 1e-2: fp32 cannot hold these rows' statistics to better than ~1e-3 of the spread, whatever the
        # order of summation (torch's own fp32 LayerNorm is a few 1e-3 off).  A two-pass kernel stays near that; a one-pass
        # E[x^2] - E[x]^2 variance would be noise (cancellation of 1e6 against 1e-4).
        mx32, nw32 = mpl_oracle.rel_errors(ref(torch.float32)[big], r64[big])
        mx, nw = mpl_oracle.rel_errors(out[big], r64[big])
        assert mx <= max(STAGE_TOL, 4 * mx32) and nw <= max(STAGE_TOL, 4 * nw32), (mx, nw, mx32, nw32)


# ----------------------------------------------------------------------------- 2. mpl_token_attention
def _attention_ref(qkv, n_seq, n_tok, dim, H):
    hd = dim // H
    t = qkv.double().cpu().reshape(n_seq, n_tok, 3, H, hd).permute(2, 0, 3, 1, 4)
    att = ((t[0] @ t[1].transpose(-2, -1)) * hd ** -0.5).softmax(-1)
    return (att @ t[2]).transpose(1, 2).reshape(n_seq * n_tok, dim)


def _attention(n_seq, n_tok, dim, H, seed, scale=1.0):
    lib = cabi.load()
    g = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(n_seq * n_tok, 3 * dim, generator=g) * scale).to(DEV)
    out = _nan(n_seq * n_tok, dim)
    rc = lib.mpl_token_attention(qkv.data_ptr(), n_seq, n_tok, dim, H, out.data_ptr(), _stream())
    return rc, qkv, out


# token_attention_any_kernel<VT> (hd & 3): VT = 4 for n_tok <= 4, 8 for <= 8, 16 for <= 16, 32 for <= 32
@pytest.mark.parametrize("n_tok", [1, 2, 4, 5, 8, 9, 16, 17, 32])
@pytest.mark.parametrize("hd", [1, 2, 3, 5, 6, 7, 17])
def test_token_attention_any_head_dim(hd, n_tok):
    H = 3
    rc, qkv, out = _attention(37, n_tok, H * hd, H, hd * 100 + n_tok)
    cabi.check(rc, "mpl_token_attention")
    _assert_close(out, _attention_ref(qkv, 37, n_tok, H * hd, H), "attention hd=%d n_tok=%d" % (hd, n_tok), STAGE_TOL)


@pytest.mark.parametrize("n_seq,n_tok,hd,H", [
    (37, 32, 4, 3),      # token_attention_lds_kernel (n_tok <= 32, hd % 4 == 0)
    (37, 32, 8, 2),      # token_attention_lds_kernel
    (5, 33, 4, 3),       # token_attention_long_p4_kernel (n_tok > 32, hd = 4)
    (5, 33, 8, 2),       # token_attention_long_kernel (n_tok > 32, hd = 8)
    (2, 2048, 4, 2),     # long p4 kernel at the 64-KiB limit: n_tok * hd * 8 = 65536
    (2, 1024, 8, 2),     # long kernel at the 64-KiB limit
    (9, 32, 52, 8),      # seq_bytes = 193 KiB > 150 KiB: global-memory token_attention_kernel<32>, hd = 52
])
def test_token_attention_short_and_long_kernels(n_seq, n_tok, hd, H):
    rc, qkv, out = _attention(n_seq, n_tok, H * hd, H, n_tok * 10 + hd)
    cabi.check(rc, "mpl_token_attention")
    _assert_close(out, _attention_ref(qkv, n_seq, n_tok, H * hd, H), "attention n_tok=%d hd=%d" % (n_tok, hd), STAGE_TOL)


@pytest.mark.parametrize("n_tok,hd", [(17, 5), (32, 8)])
def test_token_attention_large_scores_subtract_the_max(n_tok, hd):
    """|q.k| * scale of about 60 (exp(60 + 3 sigma) overflows fp32): only a max-subtracted softmax is finite here.  The
    softmax of such scores amplifies the scores' own fp32 rounding by their magnitude, hence 60x the stage tolerance."""
    H = 2
    rc, qkv, out = _attention(11, n_tok, H * hd, H, 7, scale=60 ** 0.5)
    cabi.check(rc, "mpl_token_attention")
    ref = _attention_ref(qkv, 11, n_tok, H * hd, H)
    assert torch.isfinite(out).all()
    _assert_close(out, ref, "attention large scores", 60 * STAGE_TOL)


@pytest.mark.parametrize("n_tok,hd", [(33, 12), (33, 3), (2049, 4), (1025, 8)])
def test_token_attention_refuses_without_writing(n_tok, hd):
    """Beyond the short kernels (n_tok > 32) only hd 4 / 8 with K / V of a head in 64 KiB run: MPL_E_UNSUPPORTED, nothing written."""
    (res, launched) = _launches(lambda: _attention(2, n_tok, 2 * hd, 2, 1))
    rc, _, out = res
    assert rc == E_UNSUPPORTED and launched == 0
    assert torch.isnan(out).all()


# ----------------------------------------------------------------------------- 3. the tail building blocks
STRIP_FLAGS = {"plain": 0, "rays_token": cabi.F_RAYS_TOKEN, "pos3d_to_rays": cabi.F_RAYS_TOKEN | cabi.F_POS3D_TO_RAYS}
TAIL_SHAPES = [
    # J, d -> E = J*d; fh_params: fused fuse_head_kernel needs E <= 576, E even, 3J*E <= FH_W_FLOATS (28672), 3J*E % 4 == 0
    (17, 32),   # E = 544, 3J*E = 27744: fused
    (16, 36),   # E = 576 (9 features per lane), 3J*E = 27648: fused at both limits
    (2, 2),     # E = 4, 3J*E = 24: fused, smallest
    (17, 34),   # E = 578 > 576: fuse_any_kernel
    (18, 30),   # E = 540 but 3J*E = 29160 > FH_W_FLOATS: fuse_any_kernel
    (5, 3),     # odd E = 15: fuse_any_kernel
    (7, 2),     # E = 14, 3J*E = 294 not a multiple of 4 floats: fuse_any_kernel
    (64, 64),   # E = 4096 = FA_MAX_E: fuse_any_kernel
]
TAIL_VB = [(1, 1), (2, 3), (2, 4), (32, 5), (3, 1000)]      # batches of 1, a workgroup's 4 poses -1 / +1, ~1000


def _tail_weights(J, d, V, g):
    E, n_out = J * d, 3 * J
    t = dict(vn_w=torch.rand(E, generator=g) + 0.5, vn_b=torch.randn(E, generator=g) * 0.1,
             wm_w=torch.randn(V, generator=g) * 0.5, wm_b=torch.randn(1, generator=g) * 0.1,
             hl_w=torch.rand(E, generator=g) + 0.5, hl_b=torch.randn(E, generator=g) * 0.1,
             hw=(torch.rand(n_out, E, generator=g) * 2 - 1) * E ** -0.5, hb=torch.randn(n_out, generator=g))
    dev = {k: v.to(DEV) for k, v in t.items()}
    w = cabi.Weights()
    w.view_norm_w, w.view_norm_b = dev["vn_w"].data_ptr(), dev["vn_b"].data_ptr()
    w.wmean_w, w.wmean_b = dev["wm_w"].data_ptr(), dev["wm_b"].data_ptr()
    w.head_ln_w, w.head_ln_b = dev["hl_w"].data_ptr(), dev["hl_b"].data_ptr()
    w.head_w, w.head_b = dev["hw"].data_ptr(), dev["hb"].data_ptr()
    return t, dev, w


def _tail_ref(x, t, J, d, V, B, strip):
    """multiview_mpl.py:425-446 (strip, View_norm, Conv1d weighted mean) and :521-523 (head), in float64."""
    E = J * d
    x = x.double().reshape(B, V, -1)
    if strip == "rays_token":
        x = x.reshape(B, V, 2, J, d)[:, :, 0]
    elif strip == "pos3d_to_rays":
        x = x.reshape(B, V, J, 2 * d)[..., :d]
    t = {k: v.double() for k, v in t.items()}
    xn = F.layer_norm(x.reshape(B, V, E), (E,), t["vn_w"], t["vn_b"], 1e-6)
    y = (xn * t["wm_w"].reshape(1, V, 1)).sum(1) + t["wm_b"]
    out = F.layer_norm(y, (E,), t["hl_w"], t["hl_b"], 1e-5) @ t["hw"].t() + t["hb"]
    return xn.reshape(B, V * E), y, out


@pytest.mark.parametrize("strip", list(STRIP_FLAGS))
@pytest.mark.parametrize("J,d", TAIL_SHAPES)
def test_tail_blocks_match_fp64(J, d, strip):
    """mpl_view_norm, mpl_view_fuse and mpl_fuse_head on the same rows, for every strip mode, V in {1, 2, 3, 32} and batches
    of 1 up to ~1000 poses."""
    lib = cabi.load()
    E = J * d
    Df = E * (2 if strip != "plain" else 1)
    for V, B in TAIL_VB:
        if E * B * V > 1 << 24:
            B = max(1, (1 << 24) // (E * V))
        g = torch.Generator().manual_seed(J * 1000 + d * 10 + V + B)
        t, _dev, w = _tail_weights(J, d, V, g)
        cfg = cabi.Config(J, d, 1, 1, V, 2, STRIP_FLAGS[strip], 0)
        x = torch.randn(B * V, Df, generator=g) * 1.3 + 0.2
        xd = x.to(DEV)
        xn, y, out = _nan(B, V * E), _nan(B, E), _nan(B, 3 * J)
        cabi.check(lib.mpl_view_norm(C.byref(cfg), C.byref(w), xd.data_ptr(), B, xn.data_ptr(), _stream()), "mpl_view_norm")
        cabi.check(lib.mpl_view_fuse(C.byref(cfg), C.byref(w), xd.data_ptr(), B, y.data_ptr(), _stream()), "mpl_view_fuse")
        cabi.check(lib.mpl_fuse_head(C.byref(cfg), C.byref(w), xd.data_ptr(), B, out.data_ptr(), _stream()), "mpl_fuse_head")
        rn, ry, ro = _tail_ref(x, t, J, d, V, B, strip)
        what = "J=%d d=%d %s V=%d B=%d" % (J, d, strip, V, B)
        _assert_close(xn, rn, what + " view_norm", STAGE_TOL)
        _assert_close(y, ry, what + " view_fuse", STAGE_TOL)
        _assert_close(out, ro, what + " fuse_head", STAGE_TOL)


@pytest.mark.parametrize("M,K", [(1, 1), (5, 3), (64, 51), (65, 578), (1000, 544), (3, 4096)])
def test_layernorm_block_matches_fp64(M, K):
    lib = cabi.load()
    g = torch.Generator().manual_seed(M * 13 + K)
    x, gam, bet = torch.randn(M, K, generator=g) * 2 + 1, torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g)
    xd, gd, bd = x.to(DEV), gam.to(DEV), bet.to(DEV)
    y = _nan(M, K)
    cabi.check(lib.mpl_layernorm(xd.data_ptr(), M, K, gd.data_ptr(), bd.data_ptr(), 1e-5, y.data_ptr(), _stream()), "mpl_layernorm")
    _assert_close(y, F.layer_norm(x.double(), (K,), gam.double(), bet.double(), 1e-5), "layernorm M=%d K=%d" % (M, K), STAGE_TOL)


@pytest.mark.parametrize("M,Ka,Kb,N,bn,relu", [
    (1, 3, 0, 5, False, False),         # element-wise staging (odd Ka), one row
    (77, 51, 544, 1024, True, True),    # the kadkhod concat [3J | E]: Ka not a multiple of 4 -> element-wise staging
    (65, 64, 68, 63, True, False),      # 16-byte staging across the concat boundary (Ka % 4 == 0)
    (1000, 33, 7, 65, False, True),     # odd Ka / Kb, 16 row tiles, one column past a 64 tile
    (129, 544, 0, 51, False, False),    # 16-byte staging, single source (the default head width)
    (64, 1, 1, 1, True, True),          # K = 2 of one k slab
])
def test_linear_block_matches_fp64(M, Ka, Kb, N, bn, relu):
    lib = cabi.load()
    g = torch.Generator().manual_seed(M + Ka * 3 + Kb * 5 + N * 7)
    K = Ka + Kb
    xa, xb = torch.randn(M, Ka, generator=g), torch.randn(M, max(Kb, 1), generator=g)[:, :Kb].contiguous()
    W, bias = (torch.rand(N, K, generator=g) * 2 - 1) * K ** -0.5, torch.randn(N, generator=g)
    bnp = [torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g) * 0.1, torch.randn(N, generator=g) * 0.2,
           torch.rand(N, generator=g) + 0.2]
    dev = [t.to(DEV) for t in [xa, xb, W, bias] + bnp]
    y = _nan(M, N)
    p = lambda t: t.data_ptr()
    rc = lib.mpl_linear(p(dev[0]), Ka, p(dev[1]) if Kb else None, Kb, M, p(dev[2]), p(dev[3]), N,
                        *([p(t) for t in dev[4:]] if bn else [None] * 4), 1e-5, int(relu), p(y), _stream())
    cabi.check(rc, "mpl_linear")
    ref = torch.cat([xa, xb], 1).double() @ W.double().t() + bias.double()
    if bn:
        w_, b_, mean_, var_ = (t.double() for t in bnp)
        ref = (ref - mean_) / torch.sqrt(var_ + 1e-5) * w_ + b_
    if relu:
        ref = ref.clamp_min(0)
    _assert_close(y, ref, "linear", STAGE_TOL)


# ----------------------------------------------------------------------------- 4. envelope corners, end to end
def _detrng_model(flags, seed):
    m = MultiView_MPL(**flags)
    detrng.fill_module_(m, seed=seed)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    return m.to(DEV).eval(), sd


def _inputs(B, V, J, seed):
    p, r, c = detrng.make_inputs(B, V, J, seed=seed)
    return tuple([torch.from_numpy(x) for x in lst] for lst in (p, r, c))


def _check_forward(out, sd, flags, inp, ref, what):
    if isinstance(out, tuple):
        out, ref = out[0], ref[0]
    assert torch.isfinite(out).all(), what
    if flags["embed_dim_ratio"] > 2:
        _assert_close(out, ref, what, TOL)
        return
    # d <= 2: LayerNorm over one or two channels is ill-conditioned where they nearly agree (test_shapes_gpu.py,
    # test_timed_shapes_against_fp64_oracle): within 1e-4 norm-wise and within 4x the fp32 oracle's own max-scaled error
    mx, nw = mpl_oracle.rel_errors(out.cpu(), ref)
    r32 = mpl_oracle.forward(sd, flags, *inp, dtype=torch.float32)
    mx32, _ = mpl_oracle.rel_errors(r32[0] if isinstance(r32, tuple) else r32, ref)
    assert nw <= TOL and mx <= max(TOL, 4 * mx32), (what, mx, nw, mx32)


def _corner(J, d, H, V, depth, **extra):
    return dict(num_joints=J, embed_dim_ratio=d, num_heads=H, depth=depth, num_views=V, pose_3d_emb_learnable=True, **extra)


KP = dict(FPT_blocks_view_keypoint_tokens=True)
CORNERS = [
    # flags, batch (B*V crossing a 64-row tile where given)
    ("J1", _corner(1, 32, 8, 4, 2), 17),                       # J = 1: D_f = 32, 68 FPT rows
    ("J64_Df4096", _corner(64, 64, 8, 2, 1), 2),               # D_f = 4096: tuned GEMMs at K = 4096 / 8192, fuse_any_kernel at E = 4096
    ("d128_H1", _corner(17, 128, 1, 3, 2), 2),                 # d = 128, one head of 2176
    ("hd1", _corner(17, 5, 5, 3, 2), 22),                      # hd = 1 in the SPT; FPT width 85 (any-K), 66 rows
    ("J64_d1", _corner(64, 1, 1, 3, 2), 2),                    # d = 1: SPT LayerNorm over one channel
    ("rays_4096", _corner(64, 32, 8, 2, 1, input_rays_as_token=True), 2),   # 2 J d = 4096 with ray tokens
    ("V32_E640", _corner(20, 32, 8, 32, 2), 2),                # 32 views, E = 640: fuse_any_kernel
    ("kp32_hd3", _corner(16, 6, 2, 2, 2, **KP), 3),            # 32 keypoint tokens, hd = 3: token_attention_any_kernel<32>
    ("kp2048_hd4", _corner(64, 4, 1, 32, 1, **KP), 2),         # 2048 tokens x hd 4 x 8 B = 64 KiB: long p4 kernel at its limit
]


@pytest.mark.parametrize("name,flags,B", CORNERS, ids=[c[0] for c in CORNERS])
def test_envelope_corner_matches_fp64_oracle(name, flags, B):
    m, sd = _detrng_model(flags, seed=41)
    assert m._unsupported is None, m._unsupported
    inp = _inputs(B, flags["num_views"], flags["num_joints"], seed=9)
    ref = mpl_oracle.forward(sd, flags, *inp, dtype=torch.float64)
    P, R, Cn = ([x.to(DEV) for x in lst] for lst in inp)
    for prec, route in itertools.product(("fp32", "fp32_mfma"), ("auto", False)):
        m.set_matmul_precision(prec).use_torch_op(route)
        with torch.no_grad():
            out = m(P, rays=R, centers=Cn)
        _check_forward(out, sd, flags, inp, ref, "%s %s route=%s" % (name, prec, route))


def test_keypoint_tokens_beyond_32_with_odd_head_dim_raise_before_any_launch():
    flags = _corner(11, 6, 2, 3, 2, **KP)         # 33 tokens, hd = 3: no attention kernel takes it
    m = MultiView_MPL(**flags).to(DEV).eval()
    assert m._unsupported
    cfg = cabi.Config(11, 6, 2, 2, 3, 2, cabi.F_POS3D_LEARN | cabi.F_KPTOK, 0)
    assert cabi.load().mpl_config_supported(C.byref(cfg)) == E_UNSUPPORTED
    P, R, Cn = ([x.to(DEV) for x in lst] for lst in _inputs(2, 3, 11, seed=1))
    for route in ("auto", False):
        with torch.no_grad():
            err, launched = _launches(lambda: m.use_torch_op(route)(P, rays=R, centers=Cn))
        assert isinstance(err, NotImplementedError) and launched == 0, (route, err, launched)


def test_any_k_row_limit_is_refused_before_the_first_launch():
    """Keypoint tokens at J = 64, d = 4 (any-K GEMMs, K = 4): B = 65536 poses are 65536 row tiles of 64, one more than the
    any-K kernel's grid takes.  The forward refuses the batch before it launches anything (one pose fewer runs)."""
    flags = _corner(64, 4, 1, 1, 1, **KP)
    m = MultiView_MPL(**flags).to(DEV).eval().use_torch_op(False)
    assert m._unsupported is None
    B = 65536
    P, R, Cn = [torch.zeros(B, 64, 3, device=DEV)], [torch.zeros(B, 64, 3, device=DEV)], [torch.zeros(B, 1, 3, device=DEV)]
    with torch.no_grad():
        err, launched = _launches(lambda: m(P, rays=R, centers=Cn))
        assert isinstance(err, RuntimeError) and "not supported" in str(err) and launched == 0, (err, launched)
        out, launched = _launches(lambda: m([x[:B - 1] for x in P], rays=[x[:B - 1] for x in R], centers=[x[:B - 1] for x in Cn]))
    assert not isinstance(out, Exception) and launched > 0, out
    assert torch.isfinite(out).all()


# ----------------------------------------------------------------------------- 5. the predicate and the launchers agree
def _flag_sets():
    seen, out = set(), []
    for c in CASES:
        f = {k: v for k, v in c["flags"].items() if k not in ("num_joints", "embed_dim_ratio", "num_heads", "depth", "num_views")}
        key = tuple(sorted(f.items()))
        if key not in seen:
            seen.add(key)
            out.append(f)
    return out


def _width(J, d, flags):
    return J * d * (2 if flags.get("input_rays_as_token") else 1)


def _walk(n=240, heavy=8):
    """A fixed sample of J x (d, H) x V x flag set, at most `heavy` of them with an FPT width from 2048 to 4096 (the CPU
    oracle and the weight upload dominate there)."""
    sets = _flag_sets()
    dh = [(d, H) for d in (1, 2, 5, 6, 24, 32, 64, 128) for H in range(1, 17) if d % H == 0]
    grid = list(itertools.product((1, 2, 7, 17, 33, 64), dh, (1, 3, 32), range(len(sets))))
    rs = np.random.RandomState(2024)
    picked, n_heavy = [], 0
    for i in rs.permutation(len(grid)):
        J, (d, H), V, fi = grid[i]
        if 2048 <= _width(J, d, sets[fi]) <= 4096:
            if n_heavy >= heavy:
                continue
            n_heavy += 1
        picked.append((J, d, H, V, fi))
        if len(picked) == n:
            break
    return picked


def test_predicate_and_launchers_agree_on_a_grid():
    lib = cabi.load()
    sets = _flag_sets()
    n_ok = n_refused = 0
    for J, d, H, V, fi in _walk():
        # a model wider than the envelope is refused at any depth: it is built without blocks (whose Linear layers alone
        # would take gigabytes), every other one with depth 1
        depth = 1 if _width(J, d, sets[fi]) <= 4096 else 0
        flags = dict(sets[fi], num_joints=J, embed_dim_ratio=d, num_heads=H, depth=depth, num_views=V)
        what = "J=%d d=%d H=%d V=%d %s" % (J, d, H, V, sorted(sets[fi]))
        torch.manual_seed(J * 7919 + d * 31 + H * 7 + V + fi)
        m = MultiView_MPL(**flags)
        accepted = lib.mpl_config_supported(C.byref(m._config())) == 0
        assert accepted == (m._unsupported is None), (what, m._unsupported)
        inp = _inputs(2, V, J, seed=fi)
        P, R, Cn = ([x.to(DEV) for x in lst] for lst in inp)
        if not accepted:
            m = m.to(DEV).eval()
            with torch.no_grad():
                err, launched = _launches(lambda: m(P, rays=R, centers=Cn))
            assert isinstance(err, NotImplementedError) and launched == 0, (what, err, launched)
            n_refused += 1
            continue
        sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
        m = m.to(DEV).eval()
        with torch.no_grad():
            out = m(P, rays=R, centers=Cn)
        torch.cuda.synchronize()
        _check_forward(out, sd, flags, inp, mpl_oracle.forward(sd, flags, *inp, dtype=torch.float64), what)
        n_ok += 1
        del m, sd
    print("predicate walk: %d accepted and run, %d refused before any launch" % (n_ok, n_refused))
    assert n_ok > 50 and n_refused > 10
