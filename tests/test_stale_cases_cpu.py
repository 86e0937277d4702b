"""The table of the stale-weights check (tests/stale_cases.py), checked without a GPU: it covers MultiView_MPL._param_list() of
every model exactly, every change moves the float64 oracle by at least EFFECT x max|ref| (so a stale operand cannot hide under the
project's 1e-4 gate), the exemptions are tensors that provably do not move the poses, the kinds of change do to a module what the
table says, and the comparison helper tells a stale result from a fresh one."""
import pytest
import torch

from tests import stale_cases as S

WANTED = ("small_engine_b1", "team_rows16_direct", "team_whole_tile", "bf16_team", "j15_unpacked", "j15_bf16_any", "grid_d32",
          "grid_wide_head", "fp32_mfma", "linear_weighted_mean", "deep_head", "head_kadkhod", "multi_spt", "raytoken", "conf_fpt")

_CACHE = {}


def _model(model):
    """(module, tensor names, state dict, inputs, oracle poses): built once per model, never changed."""
    if model not in _CACHE:
        m = S.build_cpu(model)
        sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
        inp = S.inputs(model, S.CPU_BATCH)
        _CACHE[model] = (m, S.tensor_names(m), sd, inp, S.oracle_poses(model, sd, inp))
    return _CACHE[model]


def test_the_table_names_the_models_of_the_issue_and_no_row_is_dead():
    assert tuple(S.MODELS) == WANTED and set(S.FOLDED) == set(WANTED)
    assert S.CPU_BATCH <= 8
    used = set()
    for model in S.MODELS:
        used |= {S.rule_index(n) for n in _model(model)[1]}
    assert used == set(range(len(S.RULES))), "rows no model uses: %s" % [S.RULES[i][0] for i in set(range(len(S.RULES))) - used]
    for model, targets in S.KIND_TARGETS.items():
        names = _model(model)[1]
        assert all(t in names for t in targets), model
        classes = [S.fold_class(model, t) for t in targets]
        assert "inplace" in classes and ("fpt" in classes or "spt" in classes), (model, classes)
    every = [S.fold_class(mo, t) for mo, ts in S.KIND_TARGETS.items() for t in ts]
    assert {"fpt", "spt", "inplace", "buffer"} <= set(every)
    assert len(S.ROUTE_PAIRS) == 6


@pytest.mark.parametrize("model", WANTED)
def test_the_table_covers_the_param_list_exactly(model):
    m, names, sd, _, _ = _model(model)
    assert len(names) == len(m._param_list()) == len(set(names)), "a tensor is handed to the library twice or has no name"
    for n in names:
        op, mag = S.mutation(n)                    # AssertionError for a tensor without (or with more than) one row
        assert op in ("mul", "add") and n in sd
    # a parameter that is added later and matches no row fails, it is not skipped
    with pytest.raises(AssertionError, match="needs a row"):
        S.mutation("some_new_stage.weight")
    # every float tensor of the state dict is visited (num_batches_tracked is not read by an eval forward)
    assert set(names) == {k for k, v in sd.items() if v.is_floating_point()}


@pytest.mark.parametrize("model", WANTED)
def test_every_change_moves_the_float64_oracle(model, capsys):
    _, names, sd, inp, ref = _model(model)
    scale = float(ref.abs().max())
    weakest, exempt = (None, float("inf")), []
    for n in names:
        op, mag = S.mutation(n)
        after = dict(sd)
        after[n] = S.mutated(sd[n], op, mag)
        assert not torch.equal(after[n], sd[n])
        move = float((S.oracle_poses(model, after, inp) - ref).abs().max()) / scale
        reason = S.exempt(model, n)
        if reason is not None:
            assert move <= 1e-9, "%s %s is exempt (%s) but moves the oracle by %.3e" % (model, n, reason, move)
            exempt.append(n)
            continue
        assert move >= S.EFFECT, "%s %s: %s %g moves the float64 oracle by %.3e x max|ref| only (bound %g)" % (model, n, op, mag, move, S.EFFECT)
        if move < weakest[1]:
            weakest = (n, move)
    with capsys.disabled():
        print("\nstale cases %s: %d tensors, weakest move %.2e x max|ref| (%s); exempt: %s" % (model, len(names), weakest[1], weakest[0], exempt))


def test_the_comparison_rejects_a_stale_result_and_accepts_the_fresh_one():
    for model in ("small_engine_b1", "head_kadkhod"):
        _, names, sd, inp, before = _model(model)
        n = "blocks.1.mlp.fc1.weight"
        after = dict(sd)
        after[n] = S.mutated(sd[n], *S.mutation(n))
        fresh = S.oracle_poses(model, after, inp).float()
        S.assert_same_bits(fresh.clone(), fresh, "fresh")
        with pytest.raises(AssertionError, match="stale"):
            S.assert_same_bits(before.float(), fresh, "poses of the state dict before the change")
        one_ulp = fresh.clone()
        one_ulp.view(-1)[3] = torch.nextafter(one_ulp.view(-1)[3], torch.tensor(float("inf")))
        with pytest.raises(AssertionError, match="stale"):
            S.assert_same_bits(one_ulp, fresh, "one unit in the last place")


@pytest.mark.parametrize("kind", S.NOTICED + S.UNCHANGED + S.ALIAS)
def test_each_kind_of_change_does_what_the_table_says(kind):
    """On the CPU: a kind leaves the tensor with the new values (AdamW: with other values than before), touches no other tensor,
    and the alias kinds are exactly the ones that leave version counter and address of the parameter alone."""
    model = "deep_head"
    if kind.endswith("_fused") and not S.fused_optimizer_offered("cpu"):
        kind = kind[:-len("_fused")] + "_foreach"      # the fused variant is run where torch offers it for the device
    from openmpl_amd import multiview_mpl as M
    for name in S.KIND_TARGETS[model]:
        m = S.build_cpu(model)
        fused_steps = M._VALUE_GEN[0]
        if not S.applies(kind, m, name):
            continue
        before = {k: v.detach().clone() for k, v in m.state_dict().items()}
        p = S._get(m, name)
        new = S.mutated(p, *S.mutation(name))
        key = (p.data_ptr(), p._version)
        m = S.apply_kind(kind, m, name, new)
        if kind == "j_flat_vector":
            q = S._get(m, name)
            assert q.data_ptr() != key[0] and q.is_contiguous()
            key = (q.data_ptr(), q._version)
            S.write_through_flat_vector(m, name, new)
        q = S._get(m, name)
        after = m.state_dict()
        if kind in S.UNCHANGED:
            assert torch.equal(q, before[name]) and (q.data_ptr(), q._version) == key and not q.requires_grad
        elif kind.startswith("d_adamw"):
            assert not torch.equal(q, before[name]) and torch.isfinite(q).all()
        else:
            assert torch.allclose(q, new, rtol=1e-6, atol=0), (kind, name)
        assert all(torch.equal(after[k], before[k]) for k in before if k != name), "%s changed another tensor" % kind
        if kind in S.ALIAS:
            assert (q.data_ptr(), q._version) == key, "%s is noticed by address or version: it is no alias write" % kind
        elif kind.endswith("_fused"):
            # torch's fused optimizers bump no version counter: the module counts their steps through an optimizer hook instead
            assert M._OPT_HOOK_OK and M._VALUE_GEN[0] == fused_steps + 1
        elif kind in S.NOTICED and q is p:
            assert M._VALUE_GEN[0] == fused_steps, "only a fused optimizer step may move the fused-step count"
            assert (q.data_ptr(), q._version) != key, "%s leaves address and version alone: nothing could notice it" % kind
