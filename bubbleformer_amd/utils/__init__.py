from .lr_schedulers import CosineWarmupLR  # noqa: F401
from .losses import LpLoss, eikonal_loss  # noqa: F401
