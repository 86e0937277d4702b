"""Run-level evaluator, CPU side: the restatement of tests/evaluate_cases.py is pinned on goldens that the reference's own
evaluate(), loss modules and AverageMeter produced (tests/golden/make_golden_evaluate.py); the GPU tests compare the kernels with both."""
import numpy as np
import pytest

from tests import evaluate_cases as ec


@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_restatement_matches_reference_evaluate(tag):
    g, arrays, kw = ec.golden_run(tag)
    res = ec.run(ec.cut(arrays, 0), **kw)
    ec.check_against_golden(res, g, rtol=1e-6, atol=1e-7)
    plain = ec.run(ec.cut(arrays, 0), **dict(kw, not_consider_kp=None))                    # evaluate() itself deletes no joint
    np.testing.assert_allclose(plain["absolute"]["mpjpe"], g["abs_mpjpe"], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(plain["relative"]["mpjpe"], g["rel_mpjpe"], rtol=1e-6, atol=1e-7)
    assert res["n_samples"] == g["out"].shape[0]
    if tag == "b":      # the fixture holds what it is there for: masked roots, and a joint masked in every sample
        assert (g["conf"][:, 0] <= 0).any() and np.isnan(g["abs_dist"][11]).all() and g["abs_pjpe"][11] == 0
    if tag == "c":      # one action absent, one with a single sample
        assert 7 not in res["absolute"]["per_group"] and res["absolute"]["per_group"][12]["n_samples"] == 1


@pytest.mark.parametrize("name", sorted(ec.E_CRITERIA))
def test_restatement_matches_reference_criteria(name):
    g = ec.golden("e")
    crit, wa = ec.E_CRITERIA[name]
    sizes = (g["splits_wa"] if name == "mpjpe_wa" else g["splits"]).tolist()
    res = ec.run(ec.cut(ec.golden_e_arrays(g), sizes), crit, g["weight_axis"] if wa else None, n_views=int(g["n_views"]))
    np.testing.assert_allclose(res["loss"], g["loss_" + name], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(res["loss_axis"], g["axis_" + name], rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("tag", ["b", "c"])
def test_restatement_does_not_depend_on_the_batching(tag):
    g, arrays, kw = ec.golden_run(tag)
    whole = ec.run(ec.cut(arrays, 0), **kw)
    for size in (1, 7, 64):
        ec.assert_same(ec.run(ec.cut(arrays, size), **kw), whole, rtol=1e-12)
    e = ec.golden("e")
    ea = ec.golden_e_arrays(e)
    for crit in ("weighted_mpjpe", "l1", "mse", "mpjpe_kadkhoda"):
        a = ec.run(ec.cut(ea, 0), crit, n_views=4)
        b = ec.run(ec.cut(ea, e["splits"].tolist()), crit, n_views=4)
        ec.assert_same(a, b, rtol=1e-12)
