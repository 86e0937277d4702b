"""Cases and float64 / float32 references of the wide-head token attention, shared by tests/test_kptok_wide_gpu.py and
tools/kptok_wide_prof.py (no pytest, no GPU needed to import)."""
import torch

from oracle import mpl_oracle

STAGE_CASES = [
    # n_seq, n_tok, hd, H
    (5, 33, 16, 3), (5, 33, 128, 1), (3, 47, 48, 2), (3, 48, 32, 2), (3, 49, 80, 1), (3, 64, 16, 2), (3, 65, 64, 2),
    (2, 255, 112, 1), (2, 256, 96, 1), (2, 257, 16, 2), (2, 527, 16, 2), (2, 527, 32, 1), (2, 1024, 128, 1), (2, 2048, 16, 2),
    (1, 2048, 64, 1),
    (3, 63, 16, 2),      # one short of the key tile and of a four-wave query tile (64 and 65 are above)
    (2, 127, 32, 2), (2, 129, 32, 2),    # around two key tiles / two query tiles (128 = 2 x 64: 256 above is 4 x 64)
]


def stage_qkv(n_seq, n_tok, hd, H, scale=1.0, seed=None):
    g = torch.Generator().manual_seed(n_tok * 10 + hd if seed is None else seed)
    return torch.randn(n_seq * n_tok, 3 * H * hd, generator=g) * scale


def attention_formula(qkv, n_seq, n_tok, dim, H, dtype):
    """Attention.forward of the reference (:55-64) on the CPU in `dtype`."""
    hd = dim // H
    t = qkv.cpu().to(dtype).reshape(n_seq, n_tok, 3, H, hd).permute(2, 0, 3, 1, 4)
    att = ((t[0] @ t[1].transpose(-2, -1)) * hd ** -0.5).softmax(-1)
    return (att @ t[2]).transpose(1, 2).reshape(n_seq * n_tok, dim)


def stage_errors(qkv_cpu, out, n_seq, n_tok, dim, H):
    """((max-scaled, norm-wise) of the kernel, (max-scaled, norm-wise) of the float32 formula), both against float64."""
    r64 = attention_formula(qkv_cpu, n_seq, n_tok, dim, H, torch.float64)
    r32 = attention_formula(qkv_cpu, n_seq, n_tok, dim, H, torch.float32)
    return mpl_oracle.rel_errors(out.detach().cpu(), r64), mpl_oracle.rel_errors(r32, r64)
