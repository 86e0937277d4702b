"""The joints x views token grid (FPT_blocks_view_keypoint_tokens) at head dims 16 .. 128: the streaming attention kernel
(csrc/token_attention_wide.hip) against float64, stage by stage and through whole forwards.

Stage bound: max(STAGE_TOL, 4 * e32), e32 = the error of the same formula evaluated by torch in float32 on the CPU (computed
here, per case) -- wide heads sum up to 128 products per score and up to 2048 per output, and plain fp32 already uses much of
STAGE_TOL = 2e-6 there; 4 is the factor the project uses for its ill-conditioned cases.  Whole forwards: TOL = 1e-4.  Both as
mpl_oracle.rel_errors (max-scaled and norm-wise).  Outputs start NaN-filled, so an element the kernel never writes fails.

The kernel's tiles: 64 keys per LDS tile (four 16-key MFMA tiles), 16 query rows per wave, up to four waves (64 query rows)
per workgroup -- 47 / 48 / 49 and 63 / 64 / 65 are the edges of both.
"""
import ctypes as C
import itertools

import pytest
import torch

from openmpl_amd import cabi, detrng
from openmpl_amd.multiview_mpl import MultiView_MPL
from oracle import mpl_oracle
from tests.kptok_wide_cases import STAGE_CASES, attention_formula, stage_errors, stage_qkv

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4          # whole forward
STAGE_TOL = 2e-6    # one stage
E_UNSUPPORTED = -2


def _stream():
    return torch.cuda.current_stream().cuda_stream


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


def run_attention(qkv_cpu, n_seq, n_tok, dim, H):
    qkv = qkv_cpu.to(DEV)
    out = _nan(n_seq * n_tok, dim)
    rc = cabi.load().mpl_token_attention(qkv.data_ptr(), n_seq, n_tok, dim, H, out.data_ptr(), _stream())
    torch.cuda.synchronize()
    return rc, out


def _assert_within_4_e32(qkv_cpu, out, n_seq, n_tok, dim, H, what):
    (mx, nw), (mx32, nw32) = stage_errors(qkv_cpu, out, n_seq, n_tok, dim, H)
    msg = "%s: kernel max-scaled %.3e norm-wise %.3e | float32 formula %.3e %.3e" % (what, mx, nw, mx32, nw32)
    print(msg)
    assert torch.isfinite(out).all(), msg
    assert mx <= max(STAGE_TOL, 4 * mx32) and nw <= max(STAGE_TOL, 4 * nw32), msg


# ----------------------------------------------------------------------------- stage: mpl_token_attention
@pytest.mark.parametrize("n_seq,n_tok,hd,H", STAGE_CASES, ids=["s%d-n%d-hd%d-H%d" % c for c in STAGE_CASES])
def test_wide_attention_matches_fp64(n_seq, n_tok, hd, H):
    qkv = stage_qkv(n_seq, n_tok, hd, H)
    rc, out = run_attention(qkv, n_seq, n_tok, H * hd, H)
    cabi.check(rc, "mpl_token_attention")
    _assert_within_4_e32(qkv, out, n_seq, n_tok, H * hd, H, "wide attention n_tok=%d hd=%d" % (n_tok, hd))


@pytest.mark.parametrize("n_tok,hd", [(33, 16), (257, 32), (527, 64), (2048, 16)])
def test_wide_attention_large_scores_subtract_the_max(n_tok, hd):
    """|q.k| * scale of about 60 (exp(60 + 3 sigma) overflows fp32): only a max-subtracted softmax is finite here; the bound of
    test_token_attention_large_scores_subtract_the_max (the softmax amplifies the scores' own rounding by their magnitude)."""
    H, n_seq = 2, 2
    qkv = stage_qkv(n_seq, n_tok, hd, H, scale=60 ** 0.5, seed=7)
    rc, out = run_attention(qkv, n_seq, n_tok, H * hd, H)
    cabi.check(rc, "mpl_token_attention")
    assert torch.isfinite(out).all()
    mx, nw = mpl_oracle.rel_errors(out.cpu(), attention_formula(qkv, n_seq, n_tok, H * hd, H, torch.float64))
    print("large scores n_tok=%d hd=%d: max-scaled %.3e norm-wise %.3e" % (n_tok, hd, mx, nw))
    assert mx <= 60 * STAGE_TOL and nw <= 60 * STAGE_TOL, (mx, nw)


def peaked_qkv(n_seq, n_tok, hd, H, j_star, seed):
    """Every query of every head scores about 40 above everything else on key j_star: q and k small and random except channel 0
    of each head, which is 1 in every q, 0 in every k and 40 hd^0.5 in k[j_star]."""
    g = torch.Generator().manual_seed(seed)
    dim = H * hd
    t = torch.randn(n_seq, n_tok, 3, H, hd, generator=g)
    t[:, :, :2] *= 0.5
    t[:, :, 0, :, 0] = 1.0
    t[:, :, 1, :, 0] = 0.0
    t[:, j_star, 1, :, 0] = 40.0 * hd ** 0.5
    return t.reshape(n_seq * n_tok, 3 * dim).contiguous()


@pytest.mark.parametrize("where", ["last_tile", "first_tile"])
@pytest.mark.parametrize("n_tok,hd", [(527, 16), (527, 32), (200, 64), (2048, 128)])
def test_wide_attention_maximum_in_a_late_or_early_tile(n_tok, hd, where):
    """The online softmax: with the row maximum in the LAST key tile everything accumulated before it is rescaled by
    exp(-40) when that tile arrives; with it in the first tile every later tile adds under an old maximum."""
    H, n_seq = 2 if hd <= 32 else 1, 2
    j_star = n_tok - 3 if where == "last_tile" else 2
    assert (j_star // 64 == (n_tok - 1) // 64) if where == "last_tile" else j_star < 64
    qkv = peaked_qkv(n_seq, n_tok, hd, H, j_star, seed=n_tok + hd)
    rc, out = run_attention(qkv, n_seq, n_tok, H * hd, H)
    cabi.check(rc, "mpl_token_attention")
    _assert_within_4_e32(qkv, out, n_seq, n_tok, H * hd, H, "peaked (%s) n_tok=%d hd=%d" % (where, n_tok, hd))


@pytest.mark.parametrize("n_tok,hd", [(33, 12), (33, 3), (2049, 4), (1025, 8), (2049, 16), (33, 144), (33, 20)])
def test_token_attention_still_refuses_without_writing(n_tok, hd):
    qkv = stage_qkv(2, n_tok, hd, 2, seed=1)
    (res, launched) = _launches(lambda: run_attention(qkv, 2, n_tok, 2 * hd, 2))
    rc, out = res
    assert rc == E_UNSUPPORTED and launched == 0
    assert torch.isnan(out).all()


# ----------------------------------------------------------------------------- whole forwards
def _flags(J, d, H, V, depth):
    return dict(num_joints=J, embed_dim_ratio=d, num_heads=H, depth=depth, num_views=V, pose_3d_emb_learnable=True,
                FPT_blocks_view_keypoint_tokens=True)


def _detrng_model(flags, seed):
    m = MultiView_MPL(**flags)
    detrng.fill_module_(m, seed=seed)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    return m.to(DEV).eval(), sd


def _inputs(B, V, J, seed):
    p, r, c = detrng.make_inputs(B, V, J, seed=seed)
    return tuple([torch.from_numpy(x) for x in lst] for lst in (p, r, c))


def _assert_forward(out, ref, what):
    assert torch.isfinite(out).all(), what
    mx, nw = mpl_oracle.rel_errors(out.detach().cpu(), ref)
    print("%s: max-scaled %.3e norm-wise %.3e" % (what, mx, nw))
    assert mx <= TOL and nw <= TOL, "%s: max-scaled %.3e norm-wise %.3e (tol %.0e)" % (what, mx, nw, TOL)


FORWARD_CASES = [
    # J, DIM, H, V, depth, B
    (17, 32, 2, 2, 2, 3), (17, 32, 1, 4, 2, 3), (17, 64, 4, 3, 2, 2), (17, 64, 1, 3, 2, 2), (17, 128, 8, 2, 2, 2),
    (17, 128, 1, 2, 2, 2), (17, 48, 1, 2, 2, 2), (64, 16, 1, 32, 1, 1), (64, 64, 1, 32, 1, 1), (17, 32, 2, 31, 12, 2),
]


@pytest.mark.parametrize("J,d,H,V,depth,B", FORWARD_CASES, ids=["J%d-d%d-H%d-V%d-L%d-B%d" % c for c in FORWARD_CASES])
def test_wide_head_keypoint_token_forward_matches_fp64_oracle(J, d, H, V, depth, B):
    flags = _flags(J, d, H, V, depth)
    m, sd = _detrng_model(flags, seed=41)
    assert m._unsupported is None, m._unsupported
    inp = _inputs(B, V, J, seed=9)
    ref = mpl_oracle.forward(sd, flags, *inp, dtype=torch.float64)
    P, R, Cn = ([x.to(DEV) for x in lst] for lst in inp)
    for prec, route in itertools.product(("fp32", "fp32_mfma"), ("auto", False)):
        m.set_matmul_precision(prec).use_torch_op(route)
        with torch.no_grad():
            out = m(P, rays=R, centers=Cn)
        _assert_forward(out, ref, "J%d d%d H%d V%d depth %d %s route=%s" % (J, d, H, V, depth, prec, route))


@pytest.mark.parametrize("small", ["auto", False])
def test_one_pose_of_34_tokens_with_and_without_the_small_batch_engine(small):
    """B = 1 at 17 joints x 2 views: 34 token rows, inside the small-batch engine's row range -- it refuses sequences longer
    than 16 tokens (sm_stack_ok), so both settings take the per-GEMM route with the streaming attention."""
    flags = _flags(17, 32, 2, 2, 2)
    m, sd = _detrng_model(flags, seed=41)
    inp = _inputs(1, 2, 17, seed=9)
    ref = mpl_oracle.forward(sd, flags, *inp, dtype=torch.float64)
    P, R, Cn = ([x.to(DEV) for x in lst] for lst in inp)
    m.set_small_batch_engine(small)
    lib = cabi.load()
    for prec, route in itertools.product(("fp32", "fp32_mfma"), ("auto", False)):
        m.set_matmul_precision(prec).use_torch_op(route)
        with torch.no_grad():
            out, launched = _launches(lambda: m(P, rays=R, centers=Cn))
        assert not isinstance(out, Exception), out
        # the route: per-GEMM kernels with one attention launch per block application (depth 2: the last block twice = 3),
        # and the library reports that form, not the small-batch engine's
        assert lib.mpl_block_stack_last_form() == cabi.FORM_UNPACKED, lib.mpl_block_stack_last_form()
        cabi.profile_start()
        with torch.no_grad():
            m(P, rays=R, centers=Cn)
        torch.cuda.synchronize()
        assert cabi.profile_stop()["attention"][1] == 3
        _assert_forward(out, ref, "34 rows small=%s %s route=%s" % (small, prec, route))


@pytest.mark.parametrize("J,d,H,V", [(17, 32, 2, 2), (17, 64, 1, 3)])
def test_a_batch_of_64_equals_its_halves_bitwise(J, d, H, V):
    m, _ = _detrng_model(_flags(J, d, H, V, 2), seed=41)
    m.set_small_batch_engine(False)
    inp = _inputs(64, V, J, seed=5)
    dev = lambda lst, sl=slice(None): [x[sl].contiguous().to(DEV) for x in lst]      # noqa: E731
    with torch.no_grad():
        big = m(dev(inp[0]), rays=dev(inp[1]), centers=dev(inp[2]))
        assert torch.isfinite(big).all()
        for sl in (slice(0, 32), slice(32, 64)):
            part = m(dev(inp[0], sl), rays=dev(inp[1], sl), centers=dev(inp[2], sl))
            assert torch.equal(big[sl], part), "wide-head kptok: batch slice changed results"


def test_bf16_on_a_wide_head_keypoint_token_model_still_raises():
    m = MultiView_MPL(**_flags(17, 32, 2, 2, 2)).to(DEV).eval()
    with pytest.raises(NotImplementedError):
        m.set_matmul_precision("bf16")


def test_odd_head_dims_beyond_32_tokens_raise_before_any_launch():
    for J, d, H, V in ((11, 6, 2, 3), (11, 6, 3, 3), (20, 4, 2, 4), (17, 20, 1, 2), (17, 24, 2, 2)):
        m = MultiView_MPL(**_flags(J, d, H, V, 2)).to(DEV).eval()
        assert m._unsupported and "head dim 4 or 8, or a multiple of 16 up to 128" in m._unsupported
        assert cabi.load().mpl_config_supported(C.byref(m._config())) == E_UNSUPPORTED
        P, R, Cn = ([x.to(DEV) for x in lst] for lst in _inputs(2, V, J, seed=1))
        for route in ("auto", False):
            with torch.no_grad():
                err, launched = _launches(lambda: m.use_torch_op(route)(P, rays=R, centers=Cn))
            assert isinstance(err, NotImplementedError) and launched == 0, (route, err, launched)
