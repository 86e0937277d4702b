"""Cases, batch selection and float64 / float32 references of the SPT stage check (tests/test_spt_stage_gpu.py) and the launch
rule restated (tests/test_spt_form_cpu.py).  No pytest and no GPU needed to import.

The SPT launch puts `spw` sequences (one pose in one view) into a workgroup: the smallest c in 1 .. cap with
V * ceil(B / c) <= CUs, else cap (csrc/spt.hip spt_form, reported by mpl_spt_form).  Restated here in closed form: with
q = CUs // V workgroups per view, ceil(B / c) <= q holds from c = ceil(B / q) on, so spw = min(cap, ceil(B / q)), and cap when
q = 0.  cap is 16 for the tuned kernels (17 / 32 / 8) and, for the shape-general kernel, the sequences whose token rows (X and A
of odd stride d | 1, T of odd stride 3 d | 1 floats) fit 64 KiB of LDS beside the 64 x 33 weight tile, at least 1.
"""
import torch

from openmpl_amd import cabi, detrng
from oracle import mpl_oracle
from tests.golden.cases import BY_NAME, CHOSEN, FULL

SPT_BOUND = 2e-5        # the project's SPT-tap bound (test_shape_spt_tokens_match_reference_tap)
E32_FACTOR = 4          # the project's factor on the float32 reference's own error
WSEED, ISEED = 23, 31

# flag sets of tests/golden/cases.py by their short names
VARIANTS = dict(chosen=CHOSEN, full=FULL)
for _n in ("chosen_conf3rd", "multi_spt", "no_spt", "conf_add", "conf_mult", "conf_attnw", "conf_fpt", "geo3d", "inspatial_learn",
           "inspatial_geo", "raytoken", "kptok"):
    VARIANTS[_n] = {k: v for k, v in BY_NAME[_n + "_v3_b3_l2"]["flags"].items()
                    if k not in ("num_joints", "embed_dim_ratio", "num_heads", "depth", "num_views")}

# (variant, V, depth) at 17 / 32 / 8: every variant at V = 3, three of them at V = 4 and 31, two at depth 12 (with
# confidence_as_attention_uncertainty_weight: 25 scheduled applications, the schedule bytes staged in LDS)
TUNED_CASES = [(n, 3, 2) for n in VARIANTS] + [(n, V, 2) for V in (4, 31) for n in ("chosen", "full", "conf_attnw")] + \
              [("chosen", 3, 12), ("conf_attnw", 3, 12)]

# the shape-general kernel elsewhere: (J, d, H) with the flag variants rotated over them, V = 3, depth 2
_ROT = ("conf_attnw", "conf_mult", "conf_fpt", "raytoken", "multi_spt", "geo3d")
SHAPES = [(15, 32, 8), (12, 24, 3), (17, 2, 2), (16, 64, 16), (21, 32, 8), (64, 64, 8), (1, 32, 8)]
SHAPE_CASES = [(J, d, H, _ROT[i % len(_ROT)]) for i, (J, d, H) in enumerate(SHAPES)]

NATIVE_SPW = {cabi.SPT_STAGED: (1, 2, 5, 8), cabi.SPT_FRAGS: (9, 12, 16)}
PACKED_SS = (1, 2, 4, 8, 16)


def case_flags(variant, V, depth, J=17, d=32, H=8):
    return dict(VARIANTS[variant], num_joints=J, embed_dim_ratio=d, num_heads=H, depth=depth, num_views=V)


# ----------------------------------------------------------------------------- the launch rule, restated
def lds_cap(J, d):
    row_bytes = (2 * (d | 1) + (3 * d | 1)) * 4
    return max(1, (64 * 1024 - 64 * 33 * 4) // (row_bytes * J))


def expected_form(J, d, H, flags, V, B, use_packed, n_cus):
    generic = (J, d, H) != (17, 32, 8) or bool(flags & cabi.F_GENERIC_SPT)
    cap = lds_cap(J, d) if generic else 16
    q = n_cus // V
    spw = min(cap, -(-B // q)) if q else cap
    if generic:
        return cabi.SPT_ANY, spw
    if not use_packed:
        return (cabi.SPT_STAGED if spw <= 8 else cabi.SPT_FRAGS), spw
    return cabi.SPT_PACKED, 1 << (spw - 1).bit_length()


def required_classes(engine, cap=None):
    """The (kernel, sequences per workgroup) pairs an engine's batches must reach."""
    if engine == "packed":
        return {(cabi.SPT_PACKED, s) for s in PACKED_SS}
    if engine == "native":
        return {(k, s) for k, spws in NATIVE_SPW.items() for s in spws}
    return {(cabi.SPT_ANY, s) for s in range(1, cap + 1)}


# ----------------------------------------------------------------------------- batches
def class_ranges(form_of, b_limit=20000):
    """{(kernel, spw): (first B, last B)} by walking B upwards through form_of(B) -> (kernel, spw).  The class of very large
    batches is open-ended: its range is cut 100 batches (three workgroups' worth of sequences, if that is more) after its first."""
    final = form_of(1 << 24)
    ranges, B = {}, 1
    while True:
        assert B <= b_limit, "the last class %r was not reached below B = %d" % (final, b_limit)
        c = form_of(B)
        assert c[0] >= 0, "mpl_spt_form failed at B = %d: %d" % (B, c[0])
        ranges[c] = (ranges.get(c, (B, B))[0], B)
        if c == final and B >= ranges[c][0] + max(100, 3 * c[1]):
            return ranges
        B += 1


def tail_batches(lo, hi, spw):
    """Batches of [lo, hi] whose last workgroup is full, holds one sequence and holds spw - 1 sequences: the first of each kind.
    A range of at least spw batches holds all three (V = 3 or 4 on a device of 64 or more CUs: CUs // V >= 16 batches per
    class); from a narrower one (V = 31: 8 batches per class at 256 CUs) the kinds it does not contain are left out.
    spw = 1: the first and the last batch of the range."""
    if spw == 1:
        return sorted({lo, hi})
    out = []
    for rem in (0, 1 % spw, spw - 1):
        hit = [B for B in range(lo, hi + 1) if B % spw == rem]
        if hit:
            out.append(hit[0])
    return sorted(set(out))


# ----------------------------------------------------------------------------- references
def make_inputs(B, flags, seed=ISEED):
    p, r, c = detrng.make_inputs(B, flags["num_views"], flags["num_joints"], seed=seed)
    return tuple([torch.from_numpy(x) for x in lst] for lst in (p, r, c))


def oracle_taps(sd, flags, inputs):
    """(fpt_in tap in float64 as (B, V * Df), the same in float32, the float64 poses) of one forward of the oracle.  Poses are
    independent: rows [0 : n] are the tap of the first n poses alone."""
    B = inputs[0][0].shape[0]
    t64, t32 = {}, {}
    out64 = mpl_oracle.forward(sd, flags, *inputs, dtype=torch.float64, taps=t64)
    mpl_oracle.forward(sd, flags, *inputs, dtype=torch.float32, taps=t32)
    return t64["fpt_in"].reshape(B, -1), t32["fpt_in"].reshape(B, -1), out64


def neighbour_confidence_gap(inputs):
    """Smallest mean |difference| between the confidences of a pose and of the next pose / of the same pose in the next view:
    O(0.1), so a kernel that reads the neighbouring sequence's confidence or another view's is far outside the bound."""
    P = inputs[0]
    c = torch.stack([p[:, :, 2] for p in P])               # (V, B, J)
    gaps = [float((c[:, 1:] - c[:, :-1]).abs().mean())] if c.shape[1] > 1 else []
    if c.shape[0] > 1:
        gaps.append(float((c[1:] - c[:-1]).abs().mean()))
    return min(gaps) if gaps else 0.0
