"""CPU: the ModernUnet baseline (unet_modern) -- registry, reference state_dict layout, the drop-in install into the reference's registry,
and the fp64 restatement the GPU parity tests are measured against, checked against the goldens generated from the reference
(tools/gen_unet_golden.py)."""
import json
import os

import pytest
import torch

from tests import unet_restatement as U
from tests.test_reference_boundary import _stand_in_registry

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUT = os.path.join(REPO, "tests", "golden", "unet_modern_layout.json")
NAMES = ["h16_m122", "h16_m122_nonorm", "h8_m12", "h8_m0"]


def _layout():
    with open(LAYOUT) as f:
        return json.load(f)


def test_get_model_builds_unet_modern():
    from bubbleformer_amd.models import get_model
    from bubbleformer_amd.models.unets import ModernUnet
    m = get_model("unet_modern", time_window=2, input_fields=4, output_fields=3, hidden_channels=8, ch_mults=[1, 2])
    assert type(m) is ModernUnet
    assert type(get_model("UNET_MODERN", hidden_channels=8)) is ModernUnet
    assert m.compute_dtype == torch.float32


def test_state_dict_matches_reference_layout_and_loads():
    from bubbleformer_amd.models import get_model
    ref = _layout()
    with torch.device("meta"):
        m = get_model("unet_modern", **ref["config"])
    sd = m.state_dict()
    assert [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in sd.items()] == ref["state_dict"]
    assert sum(p.numel() for p in m.parameters()) == ref["params"] == 566750816
    small = get_model("unet_modern", time_window=2, input_fields=4, output_fields=3, hidden_channels=8, ch_mults=[1, 2])
    ck = {k: torch.full_like(v, 0.25) for k, v in small.state_dict().items()}
    small.load_state_dict(ck)
    assert all(torch.equal(v, ck[k]) for k, v in small.state_dict().items())


def test_constructor_errors():
    from bubbleformer_amd.models import get_model
    with pytest.raises(ValueError):        # GroupNorm(8) cannot divide 12 channels
        get_model("unet_modern", hidden_channels=12, ch_mults=[1])
    m = get_model("unet_modern", time_window=2, input_fields=4, output_fields=3, hidden_channels=8, ch_mults=[1, 2, 2])
    with pytest.raises(ValueError):        # 2^(3-1) = 4 does not divide 10
        m._check_input(torch.zeros(1, 2, 4, 8, 10))
    m._check_input(torch.zeros(1, 2, 4, 8, 12))
    assert len(get_model("unet_modern", hidden_channels=8, ch_mults=[]).up) == 0


def test_install_into_reference_registers_unet_modern(monkeypatch):
    with open(os.path.join(REPO, "tests", "golden", "reference_boundary.json")) as f:
        names = json.load(f)["registry"]
    ref_models = _stand_in_registry(monkeypatch, names)
    import bubbleformer_amd
    from bubbleformer_amd.models.unets import ModernUnet
    bubbleformer_amd.install_into_reference()
    m = ref_models.get_model("unet_modern", time_window=2, input_fields=4, output_fields=3, hidden_channels=8, ch_mults=[1])
    assert type(m) is ModernUnet
    assert ref_models.list_models() == names


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference_goldens(name):
    spec, z, sd = U.load_golden(name)
    pred, loss, dx, grads = U.run(torch.from_numpy(z["x"]), torch.from_numpy(z["y"]), sd, spec["cfg"])
    rel = lambda a, b: float((a - b).norm() / b.norm())
    assert rel(pred, torch.from_numpy(z["pred"])) <= 1e-12
    assert abs(float(loss) - float(z["loss"])) <= 1e-12 * abs(float(z["loss"]))
    assert rel(dx, torch.from_numpy(z["dx"])) <= 1e-12
    assert set(grads) == set(sd)
    errs = U.golden_grad_errors(grads, z)
    assert max(errs.values()) <= 1e-12, max(errs.items(), key=lambda kv: kv[1])
