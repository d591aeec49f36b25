"""CPU: utils/param_groups.py -- GroupSpec composition, the de-duplicated group table, the chunk map against trainer.FlatParams' layout,
every refusal of resolve -- and the C ABI's declarations of the grouped optimizers (include/bubbleformer_hip.h, _lib.SIGNATURES)."""
import os
import re

import pytest
import torch

from tests.helpers import load_variant

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WD = 0.1


@pytest.fixture(scope="module")
def tiny():
    from bubbleformer_amd.models import get_model
    spec, _ = load_variant("tiny_d64")
    return get_model(spec["model"], time_window=spec["T"], drop_path=0.0, compute_dtype=torch.float32, **spec["cfg"])


def _is_1d(name, p):
    return sum(1 for d in p.shape if d > 1) <= 1 or name.endswith("relative_attention_bias.weight")


def test_specs_compose_in_list_order(tiny):
    """no_weight_decay + layer_decay(0.5) + freeze(blocks.0) on the two-block tiny FiLMAViT (L = 2): every parameter's triple is what the
    three rules say on their own -- decay 0 for the vectors and the bias tables, 0.5 ** (L + 1 - depth), frozen in block 0 -- a later
    spec overriding only the field it sets."""
    from bubbleformer_amd.utils import param_groups as PG
    specs = PG.no_weight_decay(tiny) + PG.layer_decay(tiny, 0.5) + PG.freeze(r"^blocks\.0\.")
    res = PG.resolve(tiny, specs, WD)
    names = [n for n, _ in tiny.named_parameters()]
    assert list(res.params) == names
    depth = lambda n: 0 if n.startswith(("embed.", "film_embed.")) else 3 if n.startswith("debed.") else int(n.split(".")[1]) + 1      # noqa: E731
    for n, p in tiny.named_parameters():
        assert res.params[n] == (0.5 ** (3 - depth(n)), 0.0 if _is_1d(n, p) else WD, n.startswith("blocks.0.")), n
    # the rule of no_weight_decay, on this model: every 1-D parameter, the (1, heads, 1, 1) scale factors and the 2-D bias tables
    for n, p in tiny.named_parameters():
        if p.ndim <= 1 or "attn_scale_factor" in n or n.endswith("relative_attention_bias.weight"):
            assert res.params[n][1] == 0.0, n
        else:
            assert p.ndim >= 2 and res.params[n][1] == WD, n
    # a later spec overrides only what it sets: the same lists in another order give the same triples here, and an explicit override wins
    again = PG.resolve(tiny, PG.freeze(r"^blocks\.0\.") + PG.layer_decay(tiny, 0.5) + PG.no_weight_decay(tiny), WD)
    assert again.params == res.params
    over = PG.resolve(tiny, specs + [PG.GroupSpec(r"^debed\.", weight_decay=0.3)], WD)
    assert over.params["debed.out_proj.1.bias"] == (1.0, 0.3, False) and over.params["debed.out_proj.0.weight"] == (1.0, 0.3, False)
    assert over.params["embed.in_proj.1.bias"] == res.params["embed.in_proj.1.bias"]


def test_group_table_is_deduplicated_and_group_zero_is_the_default(tiny):
    from bubbleformer_amd.utils import param_groups as PG
    specs = PG.no_weight_decay(tiny) + PG.layer_decay(tiny, 0.5) + PG.freeze(r"^blocks\.0\.")
    res = PG.resolve(tiny, specs, WD)
    assert res.table[0] == (1.0, WD, False) and res.names[0] == "default"
    assert len(set(res.table)) == len(res.table) == len(res.names) == len(res.members) == len(res) and len(set(res.names)) == len(res)
    # depth 0 (x decay or not), block 1 (x decay or not), debed (decayed = the default, or not), and ONE frozen group for all of block 0
    assert sorted(res.table) == sorted([(1.0, WD, False), (0.125, WD, False), (0.125, 0.0, False), (0.5, WD, False), (0.5, 0.0, False),
                                        (1.0, 0.0, False), (0.0, 0.0, True)])
    for k, (t, members) in enumerate(zip(res.table, res.members)):
        for n in members:
            assert res.group_of[n] == k and (t == PG.FROZEN if res.params[n][2] else t == res.params[n])
    assert sorted(n for m in res.members for n in m) == sorted(res.params)
    frozen = res.members[res.table.index(PG.FROZEN)]
    assert frozen and all(n.startswith("blocks.0.") for n in frozen) and len(frozen) == sum(n.startswith("blocks.0.") for n in res.params)
    # group 0 is the default triple even when no parameter is left in it
    every = PG.resolve(tiny, [PG.GroupSpec(".", lr_scale=0.5)], WD)
    assert every.table == [(1.0, WD, False), (0.5, WD, False)] and every.members[0] == [] and len(every.members[1]) == len(every.params)
    part = res.partition()
    assert [g["name"] for g in part] == res.names and all(set(g) == {"name", "lr_scale", "weight_decay", "frozen", "params"} for g in part)
    assert PG.same_partition(part, list(reversed(part))) and not PG.same_partition(part, every.partition())


def test_chunk_map_agrees_with_flat_params_offsets(tiny):
    """Every element of every parameter -- and the padding that rounds a parameter with numel % 64 != 0 up to its last chunk -- lies in a
    chunk that carries the parameter's group; the map has ceil(numel / 64) entries and FlatParams' alignment is the kernels' chunk."""
    import copy
    from bubbleformer_amd import _lib
    from bubbleformer_amd.trainer import FlatParams
    from bubbleformer_amd.utils import param_groups as PG
    model = copy.deepcopy(tiny)
    flat = FlatParams(model)
    hdr = open(os.path.join(REPO, "include", "bubbleformer_hip.h")).read()
    assert int(re.search(r"#define BF_OPT_CHUNK (\d+)", hdr).group(1)) == _lib.BF_OPT_CHUNK == PG.CHUNK == 64
    assert int(re.search(r"#define BF_OPT_MAX_GROUPS (\d+)", hdr).group(1)) == _lib.BF_OPT_MAX_GROUPS == PG.MAX_GROUPS == 64
    assert all(o % PG.CHUNK == 0 for o in flat.offsets) and flat.numel % PG.CHUNK == 0
    res = PG.resolve(model, PG.no_weight_decay(model) + PG.layer_decay(model, 0.5) + PG.freeze(r"^blocks\.0\."), WD)
    name_of = {id(p): n for n, p in model.named_parameters()}
    names = [name_of[id(p)] for p in flat.params]
    cmap = res.chunk_map(names, flat.offsets, flat.numel)
    assert cmap.dtype == torch.uint8 and cmap.shape == (flat.numel // PG.CHUNK,)
    per_element = cmap.repeat_interleave(PG.CHUNK)
    odd = 0
    for n, p, o in zip(names, flat.params, flat.offsets):
        padded = (p.numel() + PG.CHUNK - 1) // PG.CHUNK * PG.CHUNK
        assert (per_element[o:o + padded] == res.group_of[n]).all(), n
        odd += p.numel() % PG.CHUNK != 0
    assert odd >= 5                                    # film_net.0 (9), attn_scale_factor (2), the 32-channel norms
    assert int(cmap.max()) < len(res)
    # an unpadded tail: a buffer that ends inside a chunk still has an id for that chunk
    short = res.chunk_map(names[:2], flat.offsets[:2], flat.offsets[1] + 5)
    assert short.numel() == flat.offsets[1] // PG.CHUNK + 1 and short[-1] == res.group_of[names[1]]
    with pytest.raises(ValueError):
        res.chunk_map(names[:2], [0, 7], 128)
    with pytest.raises(ValueError):
        res.chunk_map(["nope"], [0], 64)


def test_resolve_refuses_what_it_cannot_represent(tiny):
    from bubbleformer_amd.utils import param_groups as PG
    with pytest.raises(ValueError, match="typo_stage"):
        PG.resolve(tiny, [PG.GroupSpec(r"^typo_stage\.", lr_scale=0.1)], WD)
    with pytest.raises(ValueError, match="my_rule"):
        PG.resolve(tiny, PG.no_weight_decay(tiny) + [PG.GroupSpec(lambda n, p: False, frozen=True, name="my_rule")], WD)
    with pytest.raises(ValueError, match="neg_scale"):
        PG.resolve(tiny, [PG.GroupSpec(".", lr_scale=-0.5, name="neg_scale")], WD)
    with pytest.raises(ValueError, match="neg_decay"):
        PG.resolve(tiny, [PG.GroupSpec(".", weight_decay=-1e-3, name="neg_decay")], WD)
    with pytest.raises(ValueError):
        PG.resolve(tiny, [], -0.1)
    names = [n for n, _ in tiny.named_parameters()]
    assert len(names) > 65
    many = [PG.GroupSpec("^" + re.escape(n) + "$", lr_scale=1.0 / (i + 2), name=f"one_of_many_{i}") for i, n in enumerate(names[:65])]
    with pytest.raises(ValueError, match="one_of_many_63"):           # the default and 63 more fill the 64 rows
        PG.resolve(tiny, many, WD)
    assert len(PG.resolve(tiny, many[:63], WD)) == 64
    with pytest.raises(ValueError):
        PG.layer_decay([("weight", torch.zeros(3))], 0.5)
    with pytest.raises(ValueError):
        PG.resolve(tiny, ["blocks"], WD)


def test_resolve_takes_named_parameters_and_callables():
    from bubbleformer_amd.utils import param_groups as PG
    named = [("a.weight", torch.zeros(4, 4)), ("a.bias", torch.zeros(4)), ("b.weight", torch.zeros(2, 2))]
    res = PG.resolve(named, [PG.GroupSpec(lambda n, p: p.ndim == 1, weight_decay=0.0, name="vectors"), PG.GroupSpec(r"^b\.", frozen=True)], 0.5)
    assert res.params == {"a.weight": (1.0, 0.5, False), "a.bias": (1.0, 0.0, False), "b.weight": (1.0, 0.5, True)}
    assert res.table == [(1.0, 0.5, False), (1.0, 0.0, False), PG.FROZEN] and res.names == ["default", "vectors", "frozen"]


def test_train_step_and_fit_take_param_groups():
    import inspect
    from bubbleformer_amd.fit import fit
    from bubbleformer_amd.trainer import FlatParams, TrainStep
    from bubbleformer_amd import _lib, ops
    assert inspect.signature(TrainStep.__init__).parameters["param_groups"].default is None
    assert inspect.signature(fit).parameters["param_groups"].default is None
    assert inspect.signature(FlatParams.__init__).parameters["align"].default == _lib.BF_OPT_CHUNK
    for fn in (ops.adamw_, ops.adam_, ops.lion_):
        assert inspect.signature(fn).parameters["groups"].default is None


def test_abi_declares_the_group_entry_points():
    """test_abi_exports.py compares the header, the library and _lib.SIGNATURES as sets; this names the group members of all three and holds
    every ctypes argument list to the header's parameter count.  The optimizers take their groups in the bf_opt_step record: one entry per
    optimizer with two parameters, and none of the nine entries that record replaced is declared any more."""
    from bubbleformer_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "bubbleformer_hip.h")).read(), flags=re.S)
    for opt in ("bf_adamw", "bf_adam", "bf_lion"):
        for family in ("_dev", "_avg", "_groups"):
            assert opt + family not in txt and opt + family not in _lib.SIGNATURES, opt + family
    new = ["bf_adamw", "bf_adam", "bf_lion", "bf_group_sumsq", "bf_group_sumsq_ws_doubles", "bf_group_clip_coef"]
    for name in new:
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, txt)
        assert m, name
        assert name in _lib.SIGNATURES, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
        assert not name.startswith(("bf_adam", "bf_lion")) or len(_lib.SIGNATURES[name][1]) == 2, name
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    h = _lib.lib()
    assert all(hasattr(h, n) for n in new)
    # 64 partials per slab, bf_grad_norm's slabs
    for n in (64, 4160, 1 << 30):
        assert h.bf_group_sumsq_ws_doubles(n) == 64 * h.bf_grad_norm_ws_doubles(n)
    # the argument checks come before any HIP call: no GPU needed
    assert h.bf_lion(None, None) != 0
    assert h.bf_group_clip_coef(None, None, 1, 1.0, 1.0, None, None, None) != 0


def test_grouped_step_refuses_a_reference_state_with_another_weight_decay(tmp_path):
    """A reference (torch.optim) state brings its weight decay along; a grouped step's default row was built from the step's own, so the
    two must agree -- refused before anything is written otherwise.  The same file loads into a grouped step built with its weight decay."""
    from bubbleformer_amd.trainer import TrainStep
    from bubbleformer_amd.utils.checkpoint import load_checkpoint
    from bubbleformer_amd.utils.param_groups import GroupSpec

    def make():
        torch.manual_seed(0)
        return torch.nn.Sequential(torch.nn.Linear(8, 8), torch.nn.Linear(8, 4))
    model = make()
    params = [torch.nn.Parameter(p.detach().clone()) for p in model.parameters()]
    opt = torch.optim.AdamW(params, lr=3e-4, weight_decay=0.05)
    for p in params:
        p.grad = torch.ones_like(p) * 1e-2
    opt.step()
    path = str(tmp_path / "ref.ckpt")
    torch.save({"global_step": 1, "state_dict": {"model." + k: v + 1.0 for k, v in model.state_dict().items()}, "optimizer_states": [opt.state_dict()],
                "lr_schedulers": [], "hyper_parameters": {"optim_cfg": {"name": "adamw"}}}, path)
    specs = [GroupSpec(r"bias$", weight_decay=0.0)]
    other = make()
    step = TrainStep(other, lr=1e-3, weight_decay=0.01, optimizer="adamw", param_groups=specs)
    before = step.flat.flat.clone()
    with pytest.raises(ValueError, match="weight_decay"):
        load_checkpoint(path, other, step)
    assert torch.equal(step.flat.flat, before) and step.step_no == 0 and not step.m.any()
    same = make()
    step = TrainStep(same, lr=1e-3, weight_decay=0.05, optimizer="adamw", param_groups=specs)
    load_checkpoint(path, same, step)
    assert step.step_no == 1 and step.m.any() and torch.equal(same[0].weight.detach(), model[0].weight.detach() + 1.0)
    assert step.resolved_groups.table == [(1.0, 0.05, False), (1.0, 0.0, False)] and step.groups.n_groups == 2
