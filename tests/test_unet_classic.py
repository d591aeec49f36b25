"""CPU: the ClassicUnet baseline (unet_classic) -- registry, reference state_dict layout (BatchNorm buffers included), the drop-in install
into the reference's registry, input checks, no CPU fallback, and the fp64 restatement the GPU parity tests are measured against, checked
against the goldens generated from the reference (tools/gen_unet_classic_golden.py)."""
import json
import os

import pytest
import torch

from tests import unet_classic_restatement as U
from tests.test_reference_boundary import _stand_in_registry

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUT = os.path.join(REPO, "tests", "golden", "unet_classic_layout.json")
NAMES = ["h8_c1", "h16_c8", "h8_c8_b3"]
SMALL = dict(time_window=2, input_fields=4, output_fields=3, hidden_channels=8)


def _layout():
    with open(LAYOUT) as f:
        return json.load(f)


def test_get_model_builds_unet_classic():
    from bubbleformer_amd.models import get_model
    from bubbleformer_amd.models.unets import ClassicUnet
    m = get_model("unet_classic", **SMALL)
    assert type(m) is ClassicUnet
    assert type(get_model("UNET_CLASSIC", hidden_channels=8)) is ClassicUnet
    assert m.compute_dtype == torch.float32
    assert get_model("unet_classic", compute_dtype=torch.bfloat16, **SMALL).compute_dtype == torch.bfloat16
    assert isinstance(m.encoder1.norm1, torch.nn.BatchNorm2d) and m.encoder1.conv1.bias is None


def test_state_dict_matches_reference_layout_and_loads():
    from bubbleformer_amd.models import get_model
    ref = _layout()
    assert ref["config"] == dict(time_window=16, input_fields=4, output_fields=4, hidden_channels=32)
    with torch.device("meta"):
        m = get_model("unet_classic", **ref["config"])
    sd = m.state_dict()
    assert [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in sd.items()] == ref["state_dict"]
    assert len(sd) == 118 and sum(1 for k in sd if k.endswith("num_batches_tracked")) == 18
    assert sum(p.numel() for p in m.parameters()) == ref["params"] == 7782688
    # a reference-layout state_dict (buffers included) loads
    small = get_model("unet_classic", **SMALL)
    ck = {k: (torch.full_like(v, 3) if v.dtype == torch.int64 else torch.full_like(v, 0.25)) for k, v in small.state_dict().items()}
    small.load_state_dict(ck)
    assert all(torch.equal(v, ck[k]) for k, v in small.state_dict().items())


def test_list_models_unchanged():
    from bubbleformer_amd.models import list_models
    assert list_models() == ["avit", "filmavit"]


def test_install_into_reference_registers_unet_classic(monkeypatch):
    with open(os.path.join(REPO, "tests", "golden", "reference_boundary.json")) as f:
        names = json.load(f)["registry"]
    ref_models = _stand_in_registry(monkeypatch, names)
    import bubbleformer_amd
    from bubbleformer_amd.models.unets import ClassicUnet
    bubbleformer_amd.install_into_reference()
    assert type(ref_models.get_model("unet_classic", **SMALL)) is ClassicUnet
    assert ref_models.list_models() == names


def test_input_errors_and_no_cpu_fallback():
    from bubbleformer_amd import _lib
    from bubbleformer_amd.models import get_model
    m = get_model("unet_classic", **SMALL)
    with pytest.raises(ValueError, match="divisible by 16"):
        m(torch.zeros(2, 2, 4, 16, 24))
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        m(torch.zeros(1, 2, 4, 16, 16))
    with pytest.raises(ValueError):
        m(torch.zeros(2, 3, 4, 16, 16))            # wrong time window
    m.eval()
    with pytest.raises(_lib.BubbleformerHipError):
        m(torch.zeros(1, 2, 4, 16, 16))            # one pixel per channel is fine in eval, but there is no CPU path
    m.train()
    with pytest.raises(_lib.BubbleformerHipError):
        m(torch.randn(2, 2, 4, 16, 16))
    with pytest.raises(_lib.BubbleformerHipError):
        m.forward_loss(torch.randn(2, 2, 4, 16, 16), torch.randn(2, 2, 3, 16, 16))


def test_unsupported_batchnorm_settings():
    from bubbleformer_amd.layers import ClassicUnetBlock
    from bubbleformer_amd.layers.conv_layers import bn_args
    b = ClassicUnetBlock(4, 8)
    b.norm1.momentum = None
    with pytest.raises(NotImplementedError):
        bn_args(b.norm1)
    assert bn_args(b.norm2)[3:] == (1e-5, 0.1, True)


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference_goldens(name):
    from tests.unet_restatement import golden_grad_errors       # the goldens' whole / sketched gradient comparison
    spec, z, p = U.load_golden(name)
    T = spec["cfg"]["time_window"]
    buf = U.fresh_buffers(p)
    pred, loss, dx, grads = U.run(torch.from_numpy(z["x"]), torch.from_numpy(z["y"]), p, buf, T)
    rel = lambda a, b: float((a - b).norm() / b.norm())
    assert rel(pred, torch.from_numpy(z["pred"])) <= 1e-12
    assert abs(float(loss) - float(z["loss"])) <= 1e-12 * abs(float(z["loss"]))
    assert rel(dx, torch.from_numpy(z["dx"])) <= 1e-12
    assert set(grads) == set(p)
    errs = golden_grad_errors(grads, z)
    assert max(errs.values()) <= 1e-12, max(errs.items(), key=lambda kv: kv[1])
    # BatchNorm buffers after the training forward: all 4 * 9 running statistics moved, every counter at 1
    want = U.golden_buffers(z, "b:")
    assert set(want) == set(buf) and len(want) == 54
    for k, v in want.items():
        if v.dtype == torch.int64:
            assert int(buf[k]) == int(v) == 1, k
        else:
            assert rel(buf[k], v) <= 1e-12, k
    # eval mode with seeded running statistics
    ev = U.golden_buffers(z, "e:")
    pe = U.eval_forward(torch.from_numpy(z["x"]), p, ev, T)
    assert rel(pe, torch.from_numpy(z["pred_eval"])) <= 1e-12
    assert rel(pe, pred) > 1e-3             # the eval statistics are not the batch statistics


def test_checkpoint_round_trips_batchnorm_buffers(tmp_path):
    from bubbleformer_amd.models import get_model
    from bubbleformer_amd.utils.checkpoint import load_checkpoint, save_checkpoint
    m = get_model("unet_classic", **SMALL)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for k, v in m.state_dict().items():
            v.copy_(torch.randint(1, 1000, v.shape, generator=g) if v.dtype == torch.int64 else torch.rand(v.shape, generator=g) + 0.5)
    path = str(tmp_path / "classic.ckpt")
    save_checkpoint(path, m, hyper_parameters=dict(SMALL))
    fresh = get_model("unet_classic", **SMALL)
    load_checkpoint(path, fresh)
    a, b = m.state_dict(), fresh.state_dict()
    assert list(a) == list(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
    assert b["decoder1.norm2.num_batches_tracked"].dtype == torch.int64


def test_operands_off_the_input_device_are_refused_before_any_launch():
    """The classic functions validate every weight, BatchNorm parameter and buffer against the input's device before their first launch
    (a host address handed to a kernel faults).  The validation itself runs on the CPU: a CPU model against a GPU device is refused."""
    from bubbleformer_amd import _lib, ops
    from bubbleformer_amd.layers import ClassicUnetBlock
    from bubbleformer_amd.layers.conv_layers import bn_args
    blk = ClassicUnetBlock(4, 8)
    gpu = torch.device("cuda", 0)
    with pytest.raises(_lib.BubbleformerHipError, match="conv1_weight is on cpu"):
        ops._check_operands(gpu, skip=None, conv1_weight=blk.conv1.weight, conv2_weight=blk.conv2.weight)
    with pytest.raises(_lib.BubbleformerHipError, match="weight is on cpu"):
        ops._check_bn(gpu, 8, blk.norm1.weight, blk.norm1.bias, bn_args(blk.norm1))
    # the buffers are checked as well as the parameters
    n = blk.norm2
    args = bn_args(n)
    with pytest.raises(_lib.BubbleformerHipError, match="running_var is on meta"):
        ops._check_bn(torch.device("cpu"), 8, n.weight, n.bias, (args[0], torch.empty(8, device="meta")) + args[2:])
    with pytest.raises(_lib.BubbleformerHipError, match="num_batches_tracked is on meta"):
        ops._check_bn(torch.device("cpu"), 8, n.weight, n.bias, args[:2] + (torch.empty((), dtype=torch.int64, device="meta"),) + args[3:])
    # on the matching device the same operands pass; wrong dtypes / sizes do not
    ops._check_operands(torch.device("cpu"), conv1_weight=blk.conv1.weight)
    ops._check_bn(torch.device("cpu"), 8, n.weight, n.bias, args)
    with pytest.raises(_lib.BubbleformerHipError, match="running_mean"):
        ops._check_bn(torch.device("cpu"), 8, n.weight, n.bias, (n.running_mean.double(),) + args[1:])
    with pytest.raises(_lib.BubbleformerHipError, match="num_batches_tracked"):
        ops._check_bn(torch.device("cpu"), 8, n.weight, n.bias, args[:2] + (n.num_batches_tracked.float(),) + args[3:])
    with pytest.raises(_lib.BubbleformerHipError, match="contiguous"):
        ops._check_act(torch.float32, x=torch.zeros(2, 4, 4, 8).permute(0, 3, 1, 2))
