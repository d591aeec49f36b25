"""The drop-in boundary against the reference: `bubbleformer_amd.install_into_reference()` puts the native
classes into the reference's own registry, so `bubbleformer.models.get_model("filmavit", ...)` -- what `ForecastModule.__init__`
(bubbleformer/modules.py:51-54) and scripts/inference.py:202 call -- returns the native class with the reference class's state_dict
keys, shapes and dtypes, and a reference checkpoint loads as it stands.

The reference side is recorded data: tests/golden/reference_boundary.json (oracle/gen_golden.py --only-boundary) holds the reference
registry's model names and, per model and configuration, the reference class's state_dict layout and first module names.  The registry
that `install_into_reference()` writes into is `bubbleformer.models._api`, stood in for by a fresh copy of this package's own registry
module (the same contract as the reference's: models/_api.py:5-40), holding the recorded names."""
import importlib.util
import json
import os
import sys
import types

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "reference_boundary.json")


def _stand_in_registry(monkeypatch, names):
    spec = importlib.util.spec_from_file_location("bubbleformer.models._api", os.path.join(REPO, "bubbleformer_amd", "models", "_api.py"))
    api = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(api)
    for n in names:
        api.MODELS[n] = lambda **cfg: None          # the reference's own entries; the native install replaces two of them
    pkg, models = types.ModuleType("bubbleformer"), types.ModuleType("bubbleformer.models")
    pkg.__path__, models.__path__ = [], []
    pkg.models, models._api = models, api
    models.get_model, models.list_models = api.get_model, api.list_models
    for name, mod in (("bubbleformer", pkg), ("bubbleformer.models", models), ("bubbleformer.models._api", api)):
        monkeypatch.setitem(sys.modules, name, mod)
    return models


def test_install_into_reference_registers_native_classes_with_reference_state_dict(monkeypatch):
    with open(GOLDEN) as f:
        ref = json.load(f)
    ref_models = _stand_in_registry(monkeypatch, ref["registry"])
    import bubbleformer_amd
    from bubbleformer_amd.models import axial_vit as native
    bubbleformer_amd.install_into_reference()
    for name, extra in (("filmavit", dict(num_fluid_params=9)), ("avit", {})):
        for cname, cfg in ref["configs"].items():
            want = ref["models"][f"{name}/{cname}"]
            m = ref_models.get_model(name.upper() if cname == "tiny" else name, **cfg, **extra)   # the registry lower-cases (models/_api.py:35)
            assert type(m) is getattr(native, want["class"]), type(m)
            a = m.state_dict()
            assert list(a.keys()) == [k for k, _, _ in want["state_dict"]], (name, cname, set(a) ^ {k for k, _, _ in want["state_dict"]})
            for k, shape, dtype in want["state_dict"]:
                assert list(a[k].shape) == shape and a[k].dtype == getattr(torch, dtype), (name, cname, k)
            b = {k: torch.full(shape, 0.5, dtype=getattr(torch, dtype)) for k, shape, dtype in want["state_dict"]}
            m.load_state_dict(b)                                       # a reference checkpoint loads as it stands
            assert all(torch.equal(v, b[k]) for k, v in m.state_dict().items())
            assert [n for n, _ in m.named_modules()][:4] == want["first_modules"]
    assert ref_models.list_models() == ref["registry"] == ["avit", "filmavit", "unet_classic", "unet_modern"]
