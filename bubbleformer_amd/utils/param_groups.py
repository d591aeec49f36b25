"""Parameter groups for the fused flat optimizers: freeze parameters, scale their learning rate, give them their own weight decay.

The training step keeps every parameter in one flat fp32 buffer (trainer.FlatParams) in which every parameter starts on a multiple of
``CHUNK`` = 64 elements, so each 64-element chunk belongs to one parameter.  A one-byte group id per chunk then selects, inside the
optimizer kernel, the group's learning-rate scale, weight decay and frozen flag (csrc/optim_kernels.h).  This
module turns a list of ``GroupSpec`` into that table and map.  It is pure Python (torch only for the parameters' shapes and the map's
uint8 tensor) and runs without a GPU.

* ``GroupSpec``         -- one rule: which parameters, and which of the three fields it sets.
* ``resolve``           -- specs -> per-parameter triples, the de-duplicated group table, each group's members, the chunk map.
* ``no_weight_decay`` / ``layer_decay`` / ``freeze`` -- helpers that return spec lists; they compose by list concatenation.
* ``group_norms``       -- the per-group parameter and gradient norms of a grouped TrainStep, on demand.
"""
import re
from collections import OrderedDict
from dataclasses import dataclass
from typing import Callable, Dict, Iterable, List, Optional, Sequence, Tuple, Union

import torch

from .._lib import BF_OPT_CHUNK as CHUNK, BF_OPT_MAX_GROUPS as MAX_GROUPS

Triple = Tuple[float, float, bool]      # (lr_scale, weight_decay, frozen)
FROZEN: Triple = (0.0, 0.0, True)       # every frozen parameter is in one group, whatever its other two fields say


@dataclass(frozen=True)
class GroupSpec:
    """``match``: a regular expression searched (``re.search``) in the parameter's name, or a callable (name, parameter) -> bool.
    ``lr_scale`` (>= 0, multiplies the step's scheduled learning rate), ``weight_decay`` (>= 0, absolute) and ``frozen``: None leaves
    the field to the specs before this one.  Every spec that matches a parameter applies, in list order, and a later spec overrides
    only the fields it sets; a field no spec sets is scale 1, the step's weight decay, not frozen.  ``name`` labels the spec in error
    messages and in the names of the groups it shapes (default: the pattern, or the callable's __name__)."""
    match: Union[str, Callable]
    lr_scale: Optional[float] = None
    weight_decay: Optional[float] = None
    frozen: Optional[bool] = None
    name: Optional[str] = None

    @property
    def label(self) -> str:
        if self.name is not None:
            return self.name
        return self.match if isinstance(self.match, str) else getattr(self.match, "__name__", repr(self.match))

    def matches(self, name: str, param) -> bool:
        return bool(re.search(self.match, name)) if isinstance(self.match, str) else bool(self.match(name, param))


def _named(model_or_named_parameters) -> List[Tuple[str, object]]:
    src = model_or_named_parameters
    return list(src.named_parameters()) if hasattr(src, "named_parameters") else [(str(n), p) for n, p in src]


class ResolvedGroups:
    """What ``resolve`` returns.
      params   OrderedDict name -> (lr_scale, weight_decay, frozen) as the specs leave the parameter (a frozen one keeps its other fields here)
      table    the distinct triples; table[0] is always the default (1.0, weight_decay, False), members or not, and all frozen parameters
               share one group (0.0, 0.0, True)
      names    one label per group: "default", or the labels of the specs that shaped it joined by "+"
      members  the parameter names of every group, in the model's order
      group_of name -> index into table"""

    def __init__(self, params, table, names, members, group_of):
        self.params, self.table, self.names, self.members, self.group_of = params, table, names, members, group_of

    def __len__(self) -> int:
        return len(self.table)

    def chunk_map(self, names: Sequence[str], offsets: Sequence[int], numel: int) -> torch.Tensor:
        """The uint8 group id of every CHUNK-element chunk of a flat buffer of ``numel`` elements in which parameter names[i] starts at
        offsets[i] (ascending multiples of CHUNK, as trainer.FlatParams lays them out).  A parameter owns every chunk from its offset to
        the next parameter's: its last, partly filled chunk and any alignment padding behind it carry its group."""
        if len(names) != len(offsets):
            raise ValueError(f"chunk_map: {len(names)} names for {len(offsets)} offsets")
        out = torch.zeros((int(numel) + CHUNK - 1) // CHUNK, dtype=torch.uint8)
        ends = list(offsets[1:]) + [int(numel)]
        prev = 0
        for name, lo, hi in zip(names, offsets, ends):
            if name not in self.group_of:
                raise ValueError(f"chunk_map: parameter {name!r} was not resolved")
            if lo % CHUNK or lo < prev or hi < lo:
                raise ValueError(f"chunk_map: parameter {name!r} starts at {lo}: offsets must be ascending multiples of {CHUNK}")
            out[lo // CHUNK:(hi + CHUNK - 1) // CHUNK] = self.group_of[name]
            prev = lo
        return out

    def partition(self) -> List[dict]:
        """The groups as a checkpoint records them: [{name, lr_scale, weight_decay, frozen, params: [names]}]."""
        return [{"name": n, "lr_scale": t[0], "weight_decay": t[1], "frozen": t[2], "params": list(m)}
                for n, t, m in zip(self.names, self.table, self.members)]


def same_partition(a: List[dict], b: List[dict]) -> bool:
    """Two ``partition()`` lists describe the same groups (labels and order aside; groups without members aside)."""
    def key(part):
        return sorted((float(g["lr_scale"]), float(g["weight_decay"]), bool(g["frozen"]), tuple(g["params"])) for g in part if g["params"])
    return key(a) == key(b)


def resolve(model_or_named_parameters, specs: Sequence[GroupSpec], weight_decay: float) -> ResolvedGroups:
    """Applies ``specs`` to every parameter of a module (or of an iterable of (name, parameter)) -> ResolvedGroups.  ``weight_decay`` is
    the step's, the fallback of a parameter no spec gives its own.  ValueError, naming the spec: a spec that matches no parameter, a
    negative lr_scale or weight_decay; and more than 64 distinct triples (the kernels' table size)."""
    if not weight_decay >= 0:
        raise ValueError(f"resolve: weight_decay {weight_decay!r} must be >= 0")
    specs = list(specs)
    for s in specs:
        if not isinstance(s, GroupSpec):
            raise ValueError(f"param_groups must be a list of GroupSpec, got {s!r}")
        for field in ("lr_scale", "weight_decay"):
            v = getattr(s, field)
            if v is not None and not float(v) >= 0:
                raise ValueError(f"GroupSpec {s.label!r}: {field} {v!r} must be >= 0")
    default: Triple = (1.0, float(weight_decay), False)
    params, labels, hit = OrderedDict(), {}, [False] * len(specs)
    for name, p in _named(model_or_named_parameters):
        scale, wd, frozen = default
        used = []
        for i, s in enumerate(specs):
            if not s.matches(name, p):
                continue
            hit[i] = True
            used.append(s.label)
            scale = scale if s.lr_scale is None else float(s.lr_scale)
            wd = wd if s.weight_decay is None else float(s.weight_decay)
            frozen = frozen if s.frozen is None else bool(s.frozen)
        params[name] = (scale, wd, frozen)
        labels[name] = used
    for s, h in zip(specs, hit):
        if not h:
            raise ValueError(f"GroupSpec {s.label!r} matches no parameter")
    table, names, members, group_of = [default], ["default"], [[]], {}
    for name, t in params.items():
        key = FROZEN if t[2] else t
        if key not in table:
            table.append(key)
            label = "frozen" if key[2] else "+".join(dict.fromkeys(labels[name])) or "default"
            names.append(label if label not in names else f"{label}#{len(table) - 1}")
            members.append([])
        k = table.index(key)
        members[k].append(name)
        group_of[name] = k
    if len(table) > MAX_GROUPS:
        culprit = labels[members[MAX_GROUPS][0]]
        raise ValueError(f"param_groups give {len(table)} distinct (lr_scale, weight_decay, frozen) triples, the optimizers hold {MAX_GROUPS}; "
                         f"the first one past the limit comes from GroupSpec {culprit[-1] if culprit else 'default'!r}")
    return ResolvedGroups(params, table, names, members, group_of)


# ------------------------------------------------------------------------------------------------ helpers that return spec lists
def _is_vector_or_bias_table(name: str, p) -> bool:
    return sum(1 for d in p.shape if d > 1) <= 1 or name.endswith("relative_attention_bias.weight")


def no_weight_decay(model_or_named_parameters=None) -> List[GroupSpec]:
    """Weight decay 0 for exactly these parameters: every parameter with at most one dimension longer than 1 -- all scalars and vectors
    (``ndim <= 1``: biases, InstanceNorm / LayerNorm affines, the layer scales ``gamma*``, ``*_freq_scalar``) and the
    (1, heads, 1, 1) ``attn_scale_factor*`` -- and every ``relative_attention_bias.weight`` table (the relative-position biases, 2-D).
    Matrices and convolution kernels keep the step's weight decay.  The argument is not needed (the rule reads names and shapes only)."""
    return [GroupSpec(_is_vector_or_bias_table, weight_decay=0.0, name="no_weight_decay")]


def layer_decay(model_or_named_parameters, decay: float) -> List[GroupSpec]:
    """Layer-wise learning-rate decay for the axial models (FiLMAViT / AViT): with L processor blocks, ``embed`` and ``film_embed`` have
    depth 0, ``blocks.i`` depth i + 1 and ``debed`` depth L + 1, and a parameter of depth d gets lr_scale = decay ** (L + 1 - d) -- timm's
    ``lr_scale`` convention: the scale multiplies the scheduled learning rate."""
    if not decay > 0:
        raise ValueError(f"layer_decay: decay {decay!r} must be > 0")
    blocks = {int(m.group(1)) for n, _ in _named(model_or_named_parameters) for m in [re.match(r"blocks\.(\d+)\.", n)] if m}
    if not blocks:
        raise ValueError("layer_decay: the model has no `blocks.<i>.` parameters (it works on the axial models)")
    L = max(blocks) + 1
    specs = [GroupSpec(r"^(embed|film_embed)\.", lr_scale=float(decay) ** (L + 1), name="layer_decay[0]")]
    specs += [GroupSpec(r"^blocks\.%d\." % i, lr_scale=float(decay) ** (L - i), name=f"layer_decay[{i + 1}]") for i in sorted(blocks)]
    return specs + [GroupSpec(r"^debed\.", lr_scale=1.0, name=f"layer_decay[{L + 1}]")]


def freeze(pattern: Union[str, Callable]) -> List[GroupSpec]:
    """The parameters ``pattern`` matches (a regular expression or a callable, as GroupSpec.match) are frozen: the optimizer neither reads
    nor writes them, their moments or their average."""
    return [GroupSpec(pattern, frozen=True, name=f"freeze({pattern if isinstance(pattern, str) else getattr(pattern, '__name__', 'callable')})")]


def group_norms(step) -> Dict[str, Tuple[float, float]]:
    """{group name: (||p||, ||g||)} of a grouped TrainStep: the 2-norms of the flat parameter buffer and of the flat gradient buffer as it
    stands (the raw sum of the last step's micro-batches, not scaled), per group, from two ops.group_sumsq calls.  Synchronises."""
    if getattr(step, "groups", None) is None:
        raise RuntimeError("group_norms: this TrainStep has no param_groups")
    p = step.ops.group_sumsq(step.flat.flat, step.groups).sqrt().tolist()
    g = step.ops.group_sumsq(step.flat.grad, step.groups).sqrt().tolist()
    return {name: (p[k], g[k]) for k, name in enumerate(step.resolved_groups.names)}
