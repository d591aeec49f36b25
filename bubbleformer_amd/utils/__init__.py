from .lr_schedulers import CosineWarmupLR  # noqa: F401
from .losses import LpLoss, eikonal_loss  # noqa: F401
from .physics import BubbleCensus, BubbleSpec, HeaterSpec, bubble_census, heatflux_series, kde_kl_divergence  # noqa: F401
