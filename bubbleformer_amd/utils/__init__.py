from .lr_schedulers import CosineWarmupLR  # noqa: F401
from .losses import InterfaceLpLoss, LpLoss, SpectralLpLoss, eikonal_loss  # noqa: F401
from .noise import NoiseSpec, add_gaussian_noise  # noqa: F401
from .augment import AugmentSpec, augment_plan  # noqa: F401
from .physics import BubbleCensus, BubbleMatch, BubbleSpec, BubbleTracks, HeaterSpec, bubble_census, bubble_match, bubble_tracks, heatflux_series, kde_kl_divergence  # noqa: F401
from .physics import RedistanceSpec, redistance  # noqa: F401
from .physics import ErrorSpec, FieldErrors, field_errors, shell_count  # noqa: F401
from .physics import EnsembleScores, EnsembleSpec, ensemble_scores  # noqa: F401
from .physics import FlowConsistency, FlowSpec, flow_consistency  # noqa: F401
from .plot_utils import RenderLayout, RenderSpec, plot_bubbleml, render_panels, render_strip, sdf_strip, temp_strip, vel_strip  # noqa: F401
from .png import read_png, write_apng, write_png  # noqa: F401
