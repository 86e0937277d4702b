"""set_matmul_precision("bf16") for every view-token model: the shape-general bf16 engine (csrc/b1_any.hip) on the GPU.

Yardsticks: oracle/mpl_oracle.py forward(..., fpt_matmul_bf16=True) in float64 (the engine's own rounding points) for whole
forwards; float64 arithmetic on bf16-exact operands with a bound derived from fp32 round-off for one GEMM; a numpy statement of
the operand layout (below) for mpl_pack_bf16_any.  Every figure is printed before it is asserted."""
import ctypes as C

import numpy as np
import pytest
import torch

from openmpl_amd import cabi, detrng
from openmpl_amd.multiview_mpl import MultiView_MPL
from oracle import mpl_oracle
from tests import bf16_any_cases as bc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B_, G_, R_ = cabi.EPI_BIAS, cabi.EPI_BIAS_GELU, cabi.EPI_BIAS_RESIDUAL
U = 2.0 ** -24          # unit round-off of fp32


def _stream():
    return torch.cuda.current_stream().cuda_stream


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


def _model(flags, seed=bc.WEIGHT_SEED):
    m = MultiView_MPL(**flags)
    detrng.fill_module_(m, seed=seed)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    return m.to(DEV).eval(), sd


def _inputs(B, flags, seed=bc.INPUT_SEED):
    p, r, c = detrng.make_inputs(B, flags["num_views"], flags["num_joints"], seed=seed)
    return tuple([torch.from_numpy(x) for x in lst] for lst in (p, r, c))


def _fwd(m, inp):
    P, R, Cn = ([x.to(DEV) for x in lst] for lst in inp)
    with torch.no_grad():
        return m(P, rays=R, centers=Cn)


J15 = dict(num_joints=15, embed_dim_ratio=32, num_heads=8, depth=2, num_views=4, pose_3d_emb_learnable=True)


# ----------------------------------------------------------------------------- fails without the feature
def test_j15_runs_under_bf16():
    m, _ = _model(J15, seed=3)
    m.set_matmul_precision("bf16")          # NotImplementedError before the shape-general engine existed
    out = _fwd(m, _inputs(6, J15))
    assert tuple(out.shape) == (6, 15, 3) and torch.isfinite(out).all()
    assert cabi.load().mpl_block_stack_last_form() == cabi.FORM_BF16_ANY


def test_pack_bf16_any_bytes_exists():
    assert cabi.load().mpl_pack_bf16_any_bytes(45, 15) > 0


# ----------------------------------------------------------------------------- parity against the engine's own emulation
@pytest.mark.parametrize("name,flags,B", bc.PARITY_CASES, ids=[c[0] for c in bc.PARITY_CASES])
def test_bf16_any_against_its_emulation(name, flags, B):
    """Gate per component (max-scaled, norm-wise): <= max(floor, 4 x n32), n32 = the frozen emulation evaluated in float32 against
    itself in float64 -- the bf16 roundings that flip under fp32 noise, no kernel involved; floor = the bounds of
    test_bf16_matmul_path (1e-3 / 7e-4 up to depth 2, 3e-3 / 2.5e-3 beyond).  Loose gate against the reference semantics: 5e-2."""
    m, sd = _model(flags)
    assert m._unsupported is None, m._unsupported
    m.set_matmul_precision("bf16")
    inp = _inputs(B, flags)
    out = _fwd(m, inp).cpu()
    assert cabi.load().mpl_block_stack_last_form() == cabi.FORM_BF16_ANY
    emu = mpl_oracle.forward(sd, flags, *inp, dtype=torch.float64, fpt_matmul_bf16=True)
    emu32 = mpl_oracle.forward(sd, flags, *inp, dtype=torch.float32, fpt_matmul_bf16=True)
    ref = mpl_oracle.forward(sd, flags, *inp, dtype=torch.float64)
    n32 = mpl_oracle.rel_errors(emu32, emu)
    got = mpl_oracle.rel_errors(out, emu)
    loose = mpl_oracle.rel_errors(out, ref)
    floor = bc.floor_of(flags)
    gate = (max(floor[0], 4 * n32[0]), max(floor[1], 4 * n32[1]))
    print("bf16-any %-13s kernel-vs-emu64 %.2e/%.2e  n32 %.2e/%.2e  gate %.2e/%.2e  vs-fp64-reference %.2e/%.2e"
          % (name, got[0], got[1], n32[0], n32[1], gate[0], gate[1], loose[0], loose[1]))
    assert torch.isfinite(out).all()
    assert got[0] <= gate[0] and got[1] <= gate[1], (name, got, n32, gate)
    assert loose[0] < 5e-2 and loose[1] < 5e-2, (name, loose)


# ----------------------------------------------------------------------------- one GEMM against a derivable bound
def _bf16_exact(t):
    return t.to(torch.bfloat16).to(torch.float32)


def _bf16_of_bits(u16):
    return torch.from_numpy((u16.astype(np.uint32) << 16).view(np.float32).copy())


GEMM_K = [1, 5, 31, 32, 33, 85, 544, 8192]
GEMM_N = [1, 15, 16, 17, 136, 255]
GEMM_M = [1, 63, 64, 65, 1000]


@pytest.mark.parametrize("K", GEMM_K)
def test_one_gemm_within_the_fp32_accumulation_bound(K):
    """Operands bf16-exact on the host (x, W, and gamma a power of two, so gamma o W is too): every product is exact in fp32 and
    the accumulator differs from the float64 sum by at most B_acc = 2 K u (|A16| . |W16|^T), u = 2^-24, in any summation order.

    residual (plain GEMM, y aliases the residual): bias c_n >= max_m sum_k |a_mk w_nk| and residual r >= 0, so acc + c >= 0 and
      |acc + c| <= |y|: the two epilogue roundings are within 2 u |y| and the bound is exactly B_acc + 2^-23 |y|.
    bias / GELU (LayerNorm folded: rs (acc - mu s) + c): on top of rs B_acc, the fp32 statistics (two-pass sums of K terms:
      |d mu| <= g S1 with S1 = mean_k |x|, |d rs| <= 2 g rs, g = (K + 8) u), the rounding of s and c in the operand and the four
      epilogue roundings (6 u (rs (|acc| + |mu s|) + |c|)).  GELU: that bound through the activation (|gelu'| <= 1.13), the fp32
      erf (8 u |g| + u |t|), then ONE bf16 ulp (<= 2^-7 |g|) for the rounding of the output.  Nothing here is a measured number."""
    lib = cabi.load()
    worst = {B_: 0.0, G_: 0.0, R_: 0.0}
    for N in GEMM_N:
        g = torch.Generator().manual_seed(K * 1000 + N)
        W = _bf16_exact((torch.rand(N, K, generator=g) * 2 - 1) * K ** -0.5)
        gam = 2.0 ** torch.randint(-1, 2, (K,), generator=g).float()
        bet = torch.randn(K, generator=g) * 0.1
        bias = torch.randn(N, generator=g)
        for M in GEMM_M:
            x = _bf16_exact(torch.randn(M, K, generator=g) * 1.5 + 0.3)
            xd, Wd = x.to(DEV), W.to(DEV)
            for epi in (B_, G_, R_):
                ln = epi != R_
                Wg = (W * gam[None, :]) if ln else W                      # bf16-exact
                absprod = x.double().abs() @ Wg.double().abs().t()
                acc = x.double() @ Wg.double().t()
                b_acc = 2 * K * U * absprod
                if ln:
                    c = bias.double() + W.double() @ bet.double()
                    b = bias
                else:
                    b = (absprod.max(0).values * 1.01 + torch.rand(N, generator=g).double()).float()
                    c = b.double()
                vecs = torch.stack([gam, bet]).to(DEV)
                bd = b.to(DEV)
                op = torch.zeros(lib.mpl_pack_bf16_any_bytes(N, K), dtype=torch.uint8, device=DEV)
                cabi.check(lib.mpl_pack_bf16_any(Wd.data_ptr(), bd.data_ptr(), vecs[0].data_ptr() if ln else None,
                                                 vecs[1].data_ptr() if ln else None, N, K, op.data_ptr(), _stream()), "pack")
                stats = torch.full((2 * M * max(1, K // 136),), float("nan"), device=DEV)
                ws = torch.empty(max(16, lib.mpl_ln_linear_bf16_any_workspace_bytes(M, K)), dtype=torch.uint8, device=DEV)
                if epi == R_:
                    res = torch.rand(M, N, generator=g) * 2
                    y = res.to(DEV)                                       # y aliases the residual
                    resp = y.data_ptr()
                elif epi == G_:
                    y = torch.full((M, N), -1, dtype=torch.int16, device=DEV)
                    resp = None
                else:
                    y = torch.full((M, N), float("nan"), device=DEV)
                    resp = None
                rc = lib.mpl_ln_linear_bf16_any(xd.data_ptr(), M, K, int(ln), 1e-6, op.data_ptr(), N, epi, resp, y.data_ptr(),
                                                stats.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
                cabi.check(rc, "mpl_ln_linear_bf16_any")
                torch.cuda.synchronize()
                what = "K=%d N=%d M=%d epi=%d" % (K, N, M, epi)
                if epi == R_:
                    want = res.double() + acc + c
                    bound = b_acc + 2.0 ** -23 * want.abs()
                    got = y.cpu().double()
                else:
                    xx = x.double()
                    mu = xx.mean(1, keepdim=True)
                    rs = 1.0 / torch.sqrt(xx.var(1, unbiased=False, keepdim=True) + 1e-6)
                    s = Wg.double().sum(1)
                    lin = rs * (acc - mu * s) + c
                    gk = (K + 8) * U
                    s1 = xx.abs().mean(1, keepdim=True)
                    bound = rs * b_acc + rs * s.abs() * gk * s1 + 2 * gk * rs * (acc - mu * s).abs() \
                        + 6 * U * (rs * (acc.abs() + (mu * s).abs()) + c.abs())
                    bound = bound * 1.001                                  # second-order terms
                    if epi == B_:
                        want, got = lin, y.cpu().double()
                    else:
                        want = torch.nn.functional.gelu(lin)
                        bound = 1.13 * bound + 8 * U * want.abs() + U * lin.abs() + 2.0 ** -7 * want.abs() + 1e-37
                        got = _bf16_of_bits(y.cpu().numpy().view(np.uint16)).double()
                err = (got - want).abs()
                assert torch.isfinite(got).all(), what
                ratio = float((err / bound.clamp_min(1e-300)).max())
                worst[epi] = max(worst[epi], ratio)
                assert bool((err <= bound).all()), "%s: worst error / bound %.3f" % (what, ratio)
    print("bf16-any GEMM K=%d: worst error / bound  bias %.3f  gelu %.3f  residual %.3f" % (K, worst[B_], worst[G_], worst[R_]))


def test_one_gemm_refuses_what_a_block_has_not():
    lib = cabi.load()
    x = torch.zeros(64, 64, device=DEV)
    op = torch.zeros(lib.mpl_pack_bf16_any_bytes(8, 8), dtype=torch.uint8, device=DEV)
    call = lambda has_ln, epi, res: lib.mpl_ln_linear_bf16_any(x.data_ptr(), 4, 8, has_ln, 1e-6, op.data_ptr(), 8, epi, res, x.data_ptr(),
                                                               x.data_ptr(), x.data_ptr(), x.numel() * 4, _stream())
    (rcs, launched) = _launches(lambda: (call(1, R_, x.data_ptr()), call(0, B_, None), call(0, G_, None), call(0, R_, None)))
    assert all(rc != 0 for rc in rcs) and launched == 0, (rcs, launched)


# ----------------------------------------------------------------------------- operand bytes
def _np_bf16_bits(x):
    """Round float32 to bf16 (nearest even), as uint16."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _np_operand(W, bias, gamma, beta):
    """THE layout of mpl_pack_bf16_any: [ceil(N/64)][ceil(K/32)][4 column tiles][64 lanes][8] bf16 words -- lane l, element j of
    tile t of block (nb, kt) = bf16(gamma_k W_nk) at n = 64 nb + 16 t + (l & 15), k = 32 kt + 8 (l >> 4) + j, zero beyond N or K --
    then c[N] = bias + W . beta and s[N] = sum_k of the rounded words (fp64 sums, stored fp32), zero-padded to 16 bytes."""
    N, K = W.shape
    NB, KT = (N + 63) // 64, (K + 31) // 32
    Wg = (W * gamma[None, :]).astype(np.float32) if gamma is not None else W.astype(np.float32)
    bits = np.zeros((NB * 64, KT * 32), dtype=np.uint16)
    bits[:N, :K] = _np_bf16_bits(Wg)
    # [nb][t][li][kt][kq][j] -> [nb][kt][t][kq][li][j]  (lane = 16 kq + li)
    words = bits.reshape(NB, 4, 16, KT, 4, 8).transpose(0, 3, 1, 4, 2, 5).reshape(-1)
    rounded = (bits[:N, :K].astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    if gamma is not None:
        c = (bias.astype(np.float64) + (W.astype(np.float64) * beta.astype(np.float64)[None, :]).sum(1)).astype(np.float32)
        s = rounded.sum(1).astype(np.float32)
    else:
        c, s = bias.astype(np.float32), np.zeros(N, dtype=np.float32)
    tr = np.concatenate([c, s]).view(np.uint8)
    tr = np.concatenate([tr, np.zeros((-tr.size) % 16, dtype=np.uint8)])
    return words, c, s, words.view(np.uint8).size + tr.size


@pytest.mark.parametrize("N,K,ln", [(45, 15, True), (1, 1, False), (64, 32, True), (65, 33, True), (136, 85, False), (255, 544, True),
                                    (17, 8192, True)])
def test_operand_bytes_match_the_layout(N, K, ln):
    lib = cabi.load()
    g = torch.Generator().manual_seed(N * 7 + K)
    W = torch.randn(N, K, generator=g) * K ** -0.5
    W.view(-1)[0] = 1.0 + 2 ** -8          # a tie of the bf16 rounding: to even
    bias = torch.randn(N, generator=g)
    gam, bet = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g) * 0.1
    if ln:
        gam[0] = 1.0
    Wd, bd, gd, bed = (t.to(DEV) for t in (W, bias, gam, bet))
    nbytes = lib.mpl_pack_bf16_any_bytes(N, K)
    dst = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    cabi.check(lib.mpl_pack_bf16_any(Wd.data_ptr(), bd.data_ptr(), gd.data_ptr() if ln else None, bed.data_ptr() if ln else None,
                                     N, K, dst.data_ptr(), _stream()), "mpl_pack_bf16_any")
    torch.cuda.synchronize()
    raw = dst.cpu().numpy()
    words, c, s, size = _np_operand(W.numpy(), bias.numpy(), gam.numpy() if ln else None, bet.numpy() if ln else None)
    assert size == nbytes
    got = raw[:words.size * 2].view(np.uint16)
    assert np.array_equal(got, words), "N=%d K=%d: %d of %d bf16 words differ" % (N, K, int((got != words).sum()), words.size)
    vec = raw[words.size * 2:words.size * 2 + 8 * N].view(np.float32)
    assert np.array_equal(vec[:N], c) and np.array_equal(vec[N:], s), "fold vectors differ"
    assert (raw[nbytes:] == 0xA5).all(), "the pack wrote behind the operand"
    # padding is zero: every word whose column or k lies beyond the matrix
    NB, KT = (N + 63) // 64, (K + 31) // 32
    grid = got.reshape(NB, KT, 4, 4, 16, 8)            # [nb][kt][t][kq][li][j]
    n_idx = (np.arange(NB)[:, None, None] * 64 + np.arange(4)[None, :, None] * 16 + np.arange(16)[None, None, :])   # [nb][t][li]
    k_idx = (np.arange(KT)[:, None, None] * 32 + np.arange(4)[None, :, None] * 8 + np.arange(8)[None, None, :])     # [kt][kq][j]
    pad = (n_idx[:, None, :, None, :, None] >= N) | (k_idx[None, :, None, :, None, :] >= K)
    assert (grid[pad] == 0).all()


def test_operand_arguments_are_validated():
    lib = cabi.load()
    x = torch.zeros(4096, device=DEV)
    p = x.data_ptr()
    (rcs, launched) = _launches(lambda: (
        lib.mpl_pack_bf16_any(p, p, p, None, 8, 8, p, _stream()),        # a LayerNorm needs both of its vectors
        lib.mpl_pack_bf16_any(p, p, None, p, 8, 8, p, _stream()),
        lib.mpl_pack_bf16_any(p, p, None, None, 0, 8, p, _stream()),
        lib.mpl_pack_bf16_any(p, p, None, None, 8, -1, p, _stream()),
        lib.mpl_pack_bf16_any(None, p, None, None, 8, 8, p, _stream()),
        lib.mpl_pack_bf16_any(p, None, None, None, 8, 8, p, _stream())))
    assert all(rc != 0 for rc in rcs) and launched == 0, (rcs, launched)


# ----------------------------------------------------------------------------- properties
def test_bits_do_not_depend_on_batch_split_or_order():
    m, _ = _model(J15, seed=3)
    m.set_matmul_precision("bf16")
    inp = _inputs(1000, J15, seed=1)
    a = _fwd(m, inp)
    assert torch.equal(a, _fwd(m, inp)), "not repeatable"
    sub = lambda idx: tuple([x[idx] for x in lst] for lst in inp)
    for i in (0, 63, 64, 999):
        assert torch.equal(_fwd(m, sub(slice(i, i + 1)))[0], a[i]), "pose %d alone" % i
    perm = torch.randperm(1000, generator=torch.Generator().manual_seed(5))
    assert torch.equal(_fwd(m, sub(perm)), a[perm.to(DEV)]), "permuted batch"
    two = torch.cat([_fwd(m, sub(slice(0, 437))), _fwd(m, sub(slice(437, 1000)))])
    assert torch.equal(two, a), "two shards"


def test_three_host_routes_give_the_same_bits():
    m, _ = _model(J15, seed=3)
    m.set_matmul_precision("bf16")
    inp = _inputs(33, J15, seed=2)
    outs = [_fwd(m.use_torch_op(route), inp).clone() for route in ("auto", True, False)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_forms_and_nothing_sticks():
    lib = cabi.load()
    for J, d, H in ((15, 32, 8), (17, 2, 2), (16, 64, 16), (17, 32, 16)):
        flags = dict(J15, num_joints=J, embed_dim_ratio=d, num_heads=H)
        m, sd = _model(flags, seed=2)
        inp = _inputs(256, flags, seed=3)
        m.set_matmul_precision("bf16")
        _fwd(m, inp)
        assert lib.mpl_block_stack_last_form() == cabi.FORM_BF16_ANY, (J, d, H)
        assert lib.mpl_block_stack_form(256, 4, J * d, H, 3, 1, 0) == cabi.FORM_BF16_ANY
        assert lib.mpl_block_stack_form(1, 4, J * d, H, 3, 1, 0) == cabi.FORM_BF16_ANY          # a bf16 request keeps its engine
        m.set_matmul_precision("fp32")
        out = _fwd(m, inp)
        assert lib.mpl_block_stack_last_form() == cabi.FORM_UNPACKED, (J, d, H)
        ref = mpl_oracle.forward(sd, flags, *inp, dtype=torch.float64)
        mx, nw = mpl_oracle.rel_errors(out.cpu(), ref)
        # d = 2: LayerNorm over two channels is ill-conditioned where they nearly agree and the reference's own fp32 arithmetic is
        # beyond 1e-4 max-scaled there: the bound test_shapes_gpu.py::test_timed_shapes_against_fp64_oracle holds that model to
        mx_tol = 1e-4 if d > 2 else max(1e-4, 4 * mpl_oracle.rel_errors(mpl_oracle.forward(sd, flags, *inp, dtype=torch.float32), ref)[0])
        print("back to fp32 J=%d d=%d H=%d: %.2e/%.2e (max-scaled bound %.2e)" % (J, d, H, mx, nw, mx_tol))
        assert mx <= mx_tol and nw <= 1e-4, (J, d, H, mx, nw)
    # the tuned shape keeps the tuned engine
    flags = dict(J15, num_joints=17, num_views=8)
    m, _ = _model(flags, seed=11)
    m.set_matmul_precision("bf16")
    _fwd(m, _inputs(4, flags, seed=7))
    assert lib.mpl_block_stack_last_form() == cabi.FORM_TEAMS


def test_a_changed_weight_is_repacked():
    m, _ = _model(J15, seed=3)
    m.set_matmul_precision("bf16")
    inp = _inputs(8, J15, seed=4)
    a = _fwd(m, inp).clone()
    ops = [t.data_ptr() for t in m._hip_cache[0]["derived"]["fpt"][0]]
    assert torch.equal(a, _fwd(m, inp)) and ops == [t.data_ptr() for t in m._hip_cache[0]["derived"]["fpt"][0]]
    with torch.no_grad():
        m.blocks[0].mlp.fc2.weight.mul_(1.5)          # in place: same storage, _version bumped
    b = _fwd(m, inp)
    assert not torch.equal(a, b)
    import copy
    m2 = copy.deepcopy(m)                              # derived operands are dropped by __getstate__ and rebuilt by the copy
    assert not m2._hip_cache and torch.equal(_fwd(m2, inp), b)


def test_keypoint_token_model_still_refuses_bf16():
    flags = dict(J15, FPT_blocks_view_keypoint_tokens=True, num_views=2)
    m, _ = _model(flags, seed=3)
    with pytest.raises(NotImplementedError):
        m.set_matmul_precision("bf16")
    assert torch.isfinite(_fwd(m, _inputs(3, flags))).all()


def test_row_count_beyond_the_stack_envelope_is_refused_before_any_launch():
    """One joint, one channel, one view: B token rows of width 1.  The block stack takes at most 65535 row tiles of 64 for a width
    that is not a multiple of 32 (ln_gemm_rows_ok, the stack's engine-independent row envelope): one pose more is refused
    before the first launch, under bf16 as under fp32."""
    flags = dict(num_joints=1, embed_dim_ratio=1, num_heads=1, depth=1, num_views=1, pose_3d_emb_learnable=True)
    m, _ = _model(flags, seed=3)
    m.set_matmul_precision("bf16").use_torch_op(False)
    out = _fwd(m, _inputs(130, flags))                  # (also packs the operands: the refused call below must launch NOTHING)
    assert torch.isfinite(out).all() and cabi.load().mpl_block_stack_last_form() == cabi.FORM_BF16_ANY
    B = 65535 * 64 + 1
    P, R, Cn = [torch.zeros(B, 1, 3, device=DEV)], [torch.zeros(B, 1, 3, device=DEV)], [torch.zeros(B, 1, 3, device=DEV)]
    with torch.no_grad():
        err, launched = _launches(lambda: m(P, rays=R, centers=Cn))
    assert isinstance(err, RuntimeError) and "not supported" in str(err) and launched == 0, (err, launched)
