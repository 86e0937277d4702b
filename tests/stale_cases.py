"""The closed table of the stale-weights check: which models it visits, how it changes each of their tensors, by which kinds of
update, and in which call sequences.  tests/test_stale_weights_gpu.py runs the table on the device against a FRESH module built
from the live module's state_dict after every single step; tests/test_stale_cases_cpu.py checks the table itself without a GPU:
it covers MultiView_MPL._param_list() of every model exactly, every change moves the float64 oracle by at least
EFFECT x max|ref|, and the comparison helper tells a stale result from a fresh one.  Importing this module needs no GPU.

What is being tested is the layer that decides which bytes the kernels read (openmpl_amd/multiview_mpl.py _marshal / _bind /
_forward_fast, csrc/torch_ext.cpp): structs of raw addresses, packed operands folded from the parameter VALUES, the extension
binding that holds copies of both, and three identity shortcuts in front of them.  A miss there gives finite poses of the old
weights and no error, so every step is compared bit for bit and every change is large enough that no tolerance could hide it.
"""
import copy
import io
import re

from tests.forward_paths import FLAG_MODELS, FORWARD_MODELS

EFFECT = 1e-3          # a change must move the float64 oracle by >= EFFECT x max|ref|: ten times the project's 1e-4 gate
CPU_BATCH = 2          # batch of the effectiveness check on the CPU (poses of a batch are independent in eval mode)

# ---------------------------------------------------------------------------------------------------------------- models
# name -> where the record (flags, precision, small-batch engine, stack form, SPT forms, batch) comes from; never restated here
_SOURCES = dict(small_engine_b1=FORWARD_MODELS, team_rows16_direct=FORWARD_MODELS, team_whole_tile=FORWARD_MODELS, bf16_team=FORWARD_MODELS,
                j15_unpacked=FORWARD_MODELS, j15_bf16_any=FORWARD_MODELS, grid_d32=FORWARD_MODELS, grid_wide_head=FORWARD_MODELS,
                fp32_mfma=FORWARD_MODELS, linear_weighted_mean=FORWARD_MODELS, deep_head=FORWARD_MODELS, head_kadkhod=FORWARD_MODELS,
                multi_spt=FLAG_MODELS, raytoken=FLAG_MODELS, conf_fpt=FLAG_MODELS)
MODELS = {name: src[name] for name, src in _SOURCES.items()}
assert all(rec[0]["depth"] == 2 for rec in MODELS.values())

# Which block tensors are folded into packed operands (derived data; every other tensor is read in place): (FPT blocks, SPT blocks).
# FPT: the fp16x2 split operands of the width-544 / 1088 models at "fp32" (mpl_pack_h2), one bf16 per element at "bf16" (tuned
# or BF16_ANY layout), the d32 operand of the joints x views grid at DIM 32 / 8 heads (mpl_d32_pack).  SPT: mpl_spt_pack for the tuned
# shape (17 joints, DIM 32, 8 heads) unless native fp32 was asked for.  The GPU test checks this table against what _marshal keyed.
FOLDED = dict(small_engine_b1=(True, True), team_rows16_direct=(True, True), team_whole_tile=(True, True), bf16_team=(True, True),
              j15_unpacked=(False, False), j15_bf16_any=(True, False), grid_d32=(True, True), grid_wide_head=(False, False),
              fp32_mfma=(False, False), linear_weighted_mean=(True, True), deep_head=(True, True), head_kadkhod=(True, True),
              multi_spt=(True, True), raytoken=(True, True), conf_fpt=(True, True))
STAGED = ("linear_weighted_mean", "deep_head", "head_kadkhod")        # tails composed from building blocks: no extension binding
ANCHORED = tuple(n for n, rec in MODELS.items() if rec[1] in ("fp32", "fp32_mfma"))      # fresh module vs float64 oracle at 1e-4

# ---------------------------------------------------------------------------------------------------------------- mutations
# (pattern of the state_dict name, op, magnitude).  "mul": t * magnitude.  "add": t + magnitude * ramp, ramp rising from 0.5 to 1.5
# over the elements: a constant shift of a bias would be removed exactly by the LayerNorm behind it.  Magnitudes were chosen on the
# float64 oracle (test_stale_cases_cpu.py asserts the move of every (model, tensor) pair); none comes from a kernel's output.
_BLK = r"(Spatial_blocks(\.\d+)?|blocks)\.\d+\."
RULES = [
    (_BLK + r"norm[12]\.weight", "mul", 1.5),
    (_BLK + r"norm[12]\.bias", "add", 0.5),
    (_BLK + r"attn\.qkv\.weight", "mul", 1.5),
    (_BLK + r"attn\.qkv\.bias", "add", 0.5),
    (_BLK + r"attn\.proj\.weight", "mul", 1.5),
    (_BLK + r"attn\.proj\.bias", "add", 0.5),
    (_BLK + r"mlp\.fc1\.weight", "mul", 1.5),
    (_BLK + r"mlp\.fc1\.bias", "add", 0.5),
    (_BLK + r"mlp\.fc2\.weight", "mul", 1.5),
    (_BLK + r"mlp\.fc2\.bias", "add", 0.5),
    (r"Spatial_patch_to_embedding(\.\d+)?\.weight", "mul", 1.5),
    (r"Spatial_patch_to_embedding(\.\d+)?\.bias", "add", 0.5),
    (r"Spatial_pos_embed(\.\d+)?", "add", 0.5),
    (r"Spatial_norm\.weight", "mul", 1.5),
    (r"Spatial_norm\.bias", "add", 0.5),
    (r"pos_3d_embed", "add", 0.5),
    (r"pos_3d_view_coding", "add", 0.5),
    (r"pos_3d_linear\.weight", "mul", 1.5),
    (r"pos_3d_linear\.bias", "add", 0.5),
    (r"View_norm\.weight", "mul", 1.5),
    (r"View_norm\.bias", "add", 0.5),
    (r"weighted_mean\.weight", "add", 0.5),          # (a common factor of the view weights is removed by the head's LayerNorm)
    (r"weighted_mean\.bias", "add", 0.5),
    (r"ray_to_embedding\.weight", "mul", 1.5),
    (r"ray_to_embedding\.bias", "add", 0.5),
    (r"confidence_to_embedding_FPT\.weight", "mul", 1.5),
    (r"confidence_to_embedding_FPT\.bias", "add", 0.5),
    (r"head\.[\d.]+\.weight", "mul", 1.5),
    (r"head\.[\d.]+\.bias", "add", 0.5),
    (r"head\.[\d.]+\.running_mean", "add", 0.5),
    (r"head\.[\d.]+\.running_var", "mul", 3.0),
]
_RULES = [(re.compile(p), op, mag) for p, op, mag in RULES]

# Tensors no change of which can move the poses of that model, with the reason.  The CPU test asserts that the
# oracle does NOT move for them (so an entry cannot hide a tensor that matters); the GPU test still updates them and holds the
# live module to the fresh one bit for bit, only "the poses changed" is not asked.
_UNREAD = "not read by this flag set: with pose_3d_emb_learnable the learnable pos_3d_embed is added (reference :474-481); pos_3d_linear is " \
          "its geometric alternative and pos_3d_view_coding the add_3D_pos_encoding_in_Spatial one"
_CONV_BIAS = "the one bias of Conv1d(V, 1, 1) shifts every fused feature alike, and the head's LayerNorm, the only reader, removes such a shift exactly"
EXEMPT = {}                 # (model, tensor) -> reason, beyond the two rules below: empty


def _exempt_reason(model, tensor):
    flags = MODELS[model][0]
    learnable = flags.get("pose_3d_emb_learnable") and not flags.get("add_3D_pos_encoding_in_Spatial")
    if learnable and (tensor.startswith("pos_3d_linear.") or tensor == "pos_3d_view_coding"):
        return _UNREAD
    if tensor == "weighted_mean.bias" and not flags.get("linear_weighted_mean") and not flags.get("head_kadkhod"):
        return _CONV_BIAS             # (the later stages of head_kadkhod read the fused features without a LayerNorm)
    return EXEMPT.get((model, tensor))


def exempt(model, tensor):
    """The reason why (model, tensor) is held to no effectiveness bound, or None."""
    return _exempt_reason(model, tensor)


def rule_index(tensor):
    hits = [i for i, (rx, _, _) in enumerate(_RULES) if rx.fullmatch(tensor)]
    assert len(hits) == 1, "%s: matched by %d rows of the mutation table (a new parameter needs a row of its own)" % (tensor, len(hits))
    return hits[0]


def mutation(tensor):
    """(op, magnitude) of the state_dict name `tensor`; AssertionError if the table has no (or more than one) row for it."""
    _, op, mag = _RULES[rule_index(tensor)]
    return op, mag


def mutated(t, op, mag):
    """The changed VALUES of tensor t (a new tensor, same dtype / device / shape)."""
    import torch
    if op == "mul":
        return t.detach() * mag
    assert op == "add"
    ramp = torch.linspace(0.5, 1.5, t.numel(), dtype=torch.float64).reshape(t.shape).to(device=t.device, dtype=t.dtype)
    return t.detach() + mag * ramp


def build_cpu(model):
    """The model of the table on the CPU, deterministic weights (the same fill as forward_paths._fresh_model)."""
    from openmpl_amd import detrng
    from openmpl_amd.multiview_mpl import MultiView_MPL
    m = detrng.fill_module_(MultiView_MPL(**MODELS[model][0]), seed=11)
    assert m._unsupported is None, m._unsupported
    return m.eval()


def tensor_names(m):
    """state_dict names of MultiView_MPL._param_list(), in its order."""
    by_id = {}
    for n, t in list(m.named_parameters(remove_duplicate=False)) + list(m.named_buffers(remove_duplicate=False)):
        by_id.setdefault(id(t), n)
    return [by_id[id(t)] for t in m._param_list()]


def fold_class(model, tensor):
    """"fpt" / "spt": folded into a packed operand of that stage; "buffer": BatchNorm statistics; "inplace": read where it lies."""
    fpt, spt = FOLDED[model]
    if tensor.startswith("blocks."):
        return "fpt" if fpt else "inplace"
    if tensor.startswith("Spatial_blocks."):
        return "spt" if spt else "inplace"
    return "buffer" if tensor.rsplit(".", 1)[-1] in ("running_mean", "running_var") else "inplace"


def flat(out):
    """Every pose tensor a forward returns as one tensor (head_kadkhod returns three)."""
    import torch
    if isinstance(out, tuple):
        return torch.stack([out[0]] + list(out[1]))
    return out


def inputs(model, batch, seed=5):
    from openmpl_amd import detrng
    flags = MODELS[model][0]
    return detrng.make_inputs(batch, flags["num_views"], flags["num_joints"], seed=seed)


def oracle_poses(model, sd, inp):
    """float64 oracle on a state dict (any device) and numpy inputs."""
    import torch
    from oracle import mpl_oracle
    sd = {k: v.detach().to("cpu", copy=True) for k, v in sd.items()}
    return flat(mpl_oracle.forward(sd, MODELS[model][0], *inp, dtype=torch.float64))


def assert_same_bits(live, fresh, what):
    """THE comparison of the stale-weights check: the live module gives the fresh module's poses bit for bit."""
    import torch
    live, fresh = flat(live), flat(fresh)
    assert live.shape == fresh.shape and live.dtype == fresh.dtype, "%s: %s %s vs %s %s" % (what, live.shape, live.dtype, fresh.shape, fresh.dtype)
    if not torch.equal(live, fresh):
        d = (live.double() - fresh.double()).abs().max().item()
        raise AssertionError("%s: the live module does not give the fresh module's bits (max |diff| %.3e of max|fresh| %.3e): it ran "
                             "on stale weights or operands" % (what, d, fresh.double().abs().max().item()))


# ---------------------------------------------------------------------------------------------------------------- kinds of change
# Every kind leaves `name` with the values `new` (AdamW: with SOME new values; the reference is the fresh module either way).
# NOTICED: what a forward notices by itself.  ALIAS: what it cannot notice (neither the version counter nor the address of the
# parameter changes); the documented contract is that weights_changed() follows such a write.
NOTICED = ("a_mul", "a_add", "a_copy", "b_detach", "c_data", "d_sgd", "d_sgd_foreach", "d_sgd_fused", "d_adamw", "d_adamw_foreach", "d_adamw_fused",
           "e_load", "e_load_assign", "f_parameter", "f_submodule", "g_swap", "h_cpu_roundtrip", "h_double_float")
UNCHANGED = ("i_requires_grad",)
ALIAS = ("j_data_mul", "j_data_copy", "j_foreach_data", "j_flat_vector")
KIND_MODELS = ("small_engine_b1", "j15_bf16_any", "grid_d32", "multi_spt", "deep_head")
# the tensors each kind is applied to: one per class (FPT operand, SPT / d32 operand, read in place, buffer)
KIND_TARGETS = dict(
    small_engine_b1=("blocks.1.norm2.weight", "Spatial_blocks.0.attn.qkv.weight", "head.1.weight"),
    j15_bf16_any=("blocks.0.attn.proj.weight", "Spatial_blocks.1.mlp.fc1.weight", "View_norm.weight"),
    grid_d32=("blocks.1.attn.qkv.weight", "Spatial_blocks.1.norm1.weight", "Spatial_norm.weight"),
    multi_spt=("blocks.0.mlp.fc2.weight", "Spatial_blocks.2.1.mlp.fc2.weight", "Spatial_patch_to_embedding.1.weight"),
    deep_head=("blocks.0.mlp.fc1.weight", "Spatial_blocks.0.attn.proj.weight", "head.4.weight", "head.5.running_var"),
)


def _owner(m, name):
    mod_name, _, leaf = name.rpartition(".")
    return (m.get_submodule(mod_name) if mod_name else m), leaf


def _get(m, name):
    owner, leaf = _owner(m, name)
    if leaf.isdigit():                      # an entry of a ParameterList
        return owner[int(leaf)]
    return getattr(owner, leaf)


def _set(m, name, value):
    owner, leaf = _owner(m, name)
    if leaf.isdigit():
        owner[int(leaf)] = value
    else:
        setattr(owner, leaf, value)


def applies(kind, m, name):
    """Optimizers, requires_grad_ and the flat parameter vector are about Parameters; a buffer has none of them."""
    import torch.nn as nn
    if isinstance(_get(m, name), nn.Parameter):
        return True
    return not (kind.startswith("d_") or kind in ("i_requires_grad", "j_flat_vector", "f_parameter"))


def fused_optimizer_offered(device):
    """torch offers fused=True for SGD and AdamW on this device (where it does not, the caller runs the foreach step instead)."""
    import torch
    try:
        for opt in (torch.optim.SGD, torch.optim.AdamW):
            p = torch.nn.Parameter(torch.zeros(2, device=device))
            p.grad = torch.ones_like(p)
            opt([p], lr=0.1, fused=True).step()
        return True
    except Exception:
        return False


def apply_kind(kind, m, name, new):
    """Update tensor `name` of module m to the values `new` by the given kind.  Returns the module to use from here on (the device
    round trips return the same object)."""
    import torch
    import torch.nn as nn
    p = _get(m, name)
    with torch.no_grad():
        if kind == "a_mul":
            p.mul_(_ratio(p, new))                                                           # lands on `new` up to one rounding
        elif kind == "a_add":
            p.add_(new - p)
        elif kind == "a_copy":
            p.copy_(new)
        elif kind == "b_detach":
            p.detach().copy_(new)
        elif kind == "c_data":
            p.data = new.clone()
        elif kind in ("d_sgd", "d_sgd_foreach", "d_sgd_fused"):
            _only_grad(m, p, p.detach() - new)                                               # p - 1.0 * grad = new
            kw = dict(fused=True) if kind.endswith("fused") else dict(foreach=kind.endswith("foreach"))
            torch.optim.SGD([q for q in m.parameters()], lr=1.0, **kw).step()
            m.zero_grad(set_to_none=True)
        elif kind in ("d_adamw", "d_adamw_foreach", "d_adamw_fused"):
            _only_grad(m, p, torch.sign(p.detach() - new) + (p.detach() == new))             # first step: p -= lr * sign(grad)
            lr = float((new - p).abs().max()) or 0.1
            kw = dict(fused=True) if kind.endswith("fused") else dict(foreach=kind.endswith("foreach"))
            torch.optim.AdamW([q for q in m.parameters()], lr=lr, weight_decay=0.0, **kw).step()
            m.zero_grad(set_to_none=True)
        elif kind in ("e_load", "e_load_assign"):
            sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
            sd[name] = new.clone()
            m.load_state_dict(sd, strict=True, assign=kind.endswith("assign"))
        elif kind == "f_parameter":
            _set(m, name, nn.Parameter(new.clone(), requires_grad=p.requires_grad))
        elif kind == "f_submodule":
            # a whole new Block for a block tensor, a whole new Linear / LayerNorm / BatchNorm otherwise
            parts = name.split(".")
            depth = next((i + 2 for i, s in enumerate(parts) if s in ("blocks", "Spatial_blocks")), len(parts) - 1)
            if parts[0] == "Spatial_blocks" and m.multiple_spatial_blocks:
                depth += 1
            sub_name = ".".join(parts[:depth])
            if not sub_name:                                                                 # a Parameter of the model itself
                _set(m, name, nn.Parameter(new.clone(), requires_grad=p.requires_grad))
                return m
            sub = copy.deepcopy(m.get_submodule(sub_name))
            _get(sub, ".".join(parts[depth:])).copy_(new)
            parent, leaf = _owner(m, sub_name)
            if leaf.isdigit():
                parent[int(leaf)] = sub
            else:
                setattr(parent, leaf, sub)
        elif kind == "g_swap":
            other = nn.Parameter(new.clone(), requires_grad=p.requires_grad) if isinstance(p, nn.Parameter) else new.clone()
            try:
                torch.utils.swap_tensors(p, other)
            except RuntimeError as e:
                # torch refuses to swap a tensor that something else references, and a live extension binding does reference the
                # parameters (csrc/torch_ext.cpp): the documented order is weights_changed() (which releases them), then the swap
                assert "use_count" in str(e), e
                m.weights_changed()
                torch.utils.swap_tensors(p, other)
        elif kind == "h_cpu_roundtrip":
            p.copy_(new)
            dev = p.device
            m = m.cpu().to(dev)
        elif kind == "h_double_float":
            p.copy_(new)
            m = m.double().float()
        elif kind == "i_requires_grad":
            p.requires_grad_(False)
        elif kind == "j_data_mul":
            p.data.mul_(_ratio(p, new))
        elif kind == "j_data_copy":
            p.data.copy_(new)
        elif kind == "j_foreach_data":
            others = [q for q in m.parameters() if q is not p][:2]                           # ride along unchanged (times one)
            torch._foreach_mul_([p.data] + [q.data for q in others], [_ratio(p, new)] + [torch.ones_like(q) for q in others])
        elif kind == "j_flat_vector":
            # the parameters become views into ONE flat buffer (what flattening for an optimizer or a collective does); the
            # write then goes through the buffer
            ps = [q for q in m.parameters()]
            flat_vec = torch.cat([q.detach().reshape(-1) for q in ps])
            off = 0
            for q in ps:
                q.data = flat_vec[off:off + q.numel()].view_as(q)
                off += q.numel()
            m.__dict__["_stale_cases_flat_vector"] = flat_vec
            return m
        else:
            raise AssertionError("unknown kind " + kind)
    return m


def write_through_flat_vector(m, name, new):
    """After apply_kind("j_flat_vector"): write `new` into the slice of the flat buffer that parameter `name` views."""
    import torch
    p = _get(m, name)
    vec = m.__dict__["_stale_cases_flat_vector"]
    off = p.storage_offset()
    with torch.no_grad():
        vec[off:off + p.numel()].copy_(new.reshape(-1))


def _ratio(p, new):
    """new / p elementwise (1 where p is 0): the factor of an in-place product that takes p to `new`."""
    import torch
    one = torch.ones_like(p)
    return torch.where(p == 0, one, new / torch.where(p == 0, one, p))


def _only_grad(m, p, grad):
    for q in m.parameters():
        q.grad = None
    p.requires_grad_(True)
    p.grad = grad.to(p.dtype).clone()


# ---------------------------------------------------------------------------------------------------------------- sequences
ROUTES = ("auto", True, False)
ROUTE_PAIRS = [(a, b) for a in ROUTES for b in ROUTES if a is not b]          # forward on a, change, forward on b, forward on a
ROUTE_MODELS = ("small_engine_b1", "j15_bf16_any", "grid_d32", "multi_spt")     # default tails: every route exists for them
ROUTE_CHANGES = ("a_copy", "c_data")                                          # a folded tensor updated in place; a moved storage


def copies_of(m):
    """(how, copy) of a module that has run a forward: copy.deepcopy, and torch.save / torch.load through memory."""
    import torch
    buf = io.BytesIO()
    torch.save(m, buf)
    buf.seek(0)
    return [("deepcopy", copy.deepcopy(m)), ("save_load", torch.load(buf, weights_only=False))]
