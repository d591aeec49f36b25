"""bubbleformer_amd -- MI355X-native (gfx950) FiLMAViT forward/backward path behind the
HPCForge/Bubbleformer ``bubbleformer.models`` / ``bubbleformer.layers`` nn.Module API.

    from bubbleformer_amd.models import get_model
    model = get_model("filmavit", **cfg).cuda()

The compute path is hand-written HIP (``csrc/``) behind a C ABI (``include/bubbleformer_hip.h``); there is no
CPU or eager-PyTorch fallback -- importing works anywhere, running needs the built library and a ROCm GPU.
"""
from . import _lib  # noqa: F401

__version__ = "0.1.0"


def install_into_reference() -> None:
    """Register the native models in an importable reference checkout's registry so that the reference's own
    ``scripts/train.py`` / ``scripts/inference.py`` pick them up unchanged, and put the native criterion in place of the reference's:
    ``LpLoss`` and ``eikonal_loss`` in ``bubbleformer.utils.losses``, and the name ``LpLoss`` that ``bubbleformer.modules`` bound at its
    import, if it has been imported.  A checkout whose ``bubbleformer.utils`` cannot be imported keeps the models."""
    import importlib
    import sys
    import bubbleformer.models._api as ref_api  # the user's reference checkout
    from .models import axial_vit, unets
    from .utils import losses
    ref_api.MODELS["filmavit"] = axial_vit.FiLMConditionedAViT
    ref_api.MODELS["avit"] = axial_vit.AViT
    ref_api.MODELS["unet_modern"] = unets.ModernUnet
    ref_api.MODELS["unet_classic"] = unets.ClassicUnet
    try:
        ref_losses = importlib.import_module("bubbleformer.utils.losses")
    except ImportError:
        ref_losses = None
    if ref_losses is not None:
        ref_losses.LpLoss = losses.LpLoss
        ref_losses.eikonal_loss = losses.eikonal_loss
    ref_modules = sys.modules.get("bubbleformer.modules")
    if ref_modules is not None and hasattr(ref_modules, "LpLoss"):
        ref_modules.LpLoss = losses.LpLoss
