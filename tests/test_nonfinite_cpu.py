"""What the reference does with a NaN or an infinity in its inputs, and that the checker of tests/test_nonfinite_gpu.py can tell.

The survey: for every flag set of both tables of tests/forward_paths.py, every input channel and NaN, +inf, -inf, the oracle's
answer is binary -- the poisoned sample is NaN in every element of every output, or it has the bits of the clean run because
the flag set does not read the channel --, float32 and float64 give the same answer, and the neighbour is finite and unchanged
(oracle_verdict raises otherwise).  Which flags read which channel is restated here from the reference's forward
(multiview_mpl.py:352-396, :465-489) and compared with what the oracle did.

The checker: it accepts the correct result and rejects each constructed mistake.
"""
import numpy as np
import pytest
import torch

from tests import nonfinite_cases as nf
from tests.forward_paths import FLAG_MODELS, FORWARD_MODELS


def _flag_sets():
    sets = {}
    for table in (FORWARD_MODELS, FLAG_MODELS):
        for name, rec in sorted(table.items()):
            flags = rec[0]
            assert flags["depth"] <= 2 and flags["num_views"] <= 8, name
            sets.setdefault(nf._key(flags), name)
    return sorted((name, dict(key)) for key, name in sets.items())


def _reads(flags, channel):
    """the reference's forward, restated as which channel it touches"""
    f = flags.get
    if channel == "keypoint":
        return True                                                        # :359-364 the embedding of every flag set
    if channel == "confidence":
        return bool(f("confidence_input_as_third") or f("add_confidence_input") or f("mult_confidence_emb")
                    or f("confidence_as_attention_uncertainty_weight") or f("confidence_in_FPT"))
    # rays and centers only ever enter as ray - center: the geometric positional encoding (:389-396, :474-481) and the ray tokens
    return bool(not f("pose_3d_emb_learnable") or f("input_rays_as_token"))


@pytest.mark.parametrize("name,flags", _flag_sets(), ids=[n for n, _ in _flag_sets()])
def test_the_oracle_answers_nan_for_the_poisoned_sample_or_does_not_read_the_channel(name, flags):
    for channel in nf.CHANNELS:
        for value in nf.VALUES:
            wide = nf.expected(flags, channel, value)
            narrow = nf.oracle_verdict(flags, channel, value, torch.float32)
            what = "%s: %r in %s" % (name, value, channel)
            assert wide == narrow, what + ": float64 says %s, float32 says %s" % (wide, narrow)
            assert wide == _reads(flags, channel), what + ": the oracle says %s" % wide


def test_the_tables_reach_every_answer():
    """each channel is read by some flag set and ignored by another (keypoints by all): both branches of the contract are visited"""
    sets = [f for _, f in _flag_sets()]
    assert all(_reads(f, "keypoint") for f in sets)
    for channel in ("confidence", "ray", "center"):
        assert {_reads(f, channel) for f in sets} == {True, False}, channel


# --------------------------------------------------------------------------------------------------------------- the checker
def _clean_outputs():
    g = torch.Generator().manual_seed(3)
    return (torch.randn(5, 17, 3, generator=g), [torch.randn(5, 17, 3, generator=g), torch.randn(5, 17, 3, generator=g)])


def _correct(clean, victims, consumed):
    out = [t.clone() for t in nf.flatten(clean)]
    if consumed:
        for t in out:
            t[list(victims)] = float("nan")
    return (out[0], out[1:])


VICTIMS = (0, 4)


def test_the_checker_accepts_the_correct_result():
    clean = _clean_outputs()
    for consumed in (True, False):
        assert nf.check(clean, _correct(clean, VICTIMS, consumed), VICTIMS, consumed) == ""
        assert nf.check(clean[0], _correct(clean, VICTIMS, consumed)[0], VICTIMS, consumed) == ""
    assert nf.check(clean, _correct(clean, range(5), True), range(5), True) == ""


def _flip_bit(t, *index):
    t.view(torch.int32)[index] ^= 1


MISTAKES = {
    "a victim left finite": (True, lambda out, clean: out[1].__setitem__(4, clean[1][4]), "sample 4 (poisoned)"),
    "a victim NaN in all but one element": (True, lambda out, clean: out[2].__setitem__((0, 16, 2), 0.25), "sample 0 (poisoned): 1 of 51"),
    "a witness with one bit flipped": (True, lambda out, clean: _flip_bit(out[0], 2, 7, 1), "sample 2 (a witness): 1 of 51"),
    "a witness turned NaN": (True, lambda out, clean: out[1].__setitem__(3, float("nan")), "sample 3 (a witness): 51 of 51"),
    "an unconsumed channel whose victim changed": (False, lambda out, clean: _flip_bit(out[0], 4, 0, 0), "sample 4 (poisoned in a channel"),
    "an unconsumed channel whose victim is NaN": (False, lambda out, clean: out[0].__setitem__(0, float("nan")), "sample 0 (poisoned in a channel"),
}


@pytest.mark.parametrize("name", sorted(MISTAKES))
def test_the_checker_rejects(name):
    consumed, spoil, says = MISTAKES[name]
    clean = _clean_outputs()
    flat = nf.flatten(_correct(clean, VICTIMS, consumed))
    spoil(flat, nf.flatten(clean))
    verdict = nf.check(clean, (flat[0], flat[1:]), VICTIMS, consumed)
    assert says in verdict and len(verdict.splitlines()) == 1, verdict


def test_poison_hits_each_victim_at_its_own_site_and_copies():
    from openmpl_amd import detrng
    B, V, J = 5, 3, 17
    inputs = detrng.make_inputs(B, V, J, seed=nf.ISEED)
    sites = {0: (0, 0), 2: (V // 2, J // 2), 4: (V - 1, J - 1)}
    for channel in nf.CHANNELS:
        got = nf.poison(inputs, (0, 2, 4), channel, float("nan"))
        group = {"keypoint": 0, "confidence": 0, "ray": 1, "center": 2}[channel]
        for g, (mine, theirs) in enumerate(zip(got, inputs)):
            for v in range(V):
                hit = np.argwhere(np.isnan(mine[v]))
                assert np.isfinite(theirs[v]).all()                                   # the originals keep their values
                want = [b for b, (sv, _) in sites.items() if sv == v] if g == group else []
                assert sorted(hit[:, 0].tolist()) == want, (channel, g, v, hit)
                for b, j, k in hit:
                    assert channel == "center" or j == sites[b][1]
                    assert (k == 2) == (channel == "confidence") or channel in ("ray", "center")
