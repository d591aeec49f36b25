# same export list as the reference's bubbleformer/layers/__init__.py:1-5, plus the U-Net blocks (conv_layers.py:5-141)
from .positional_encoding import ContinuousPositionBias1D, RelativePositionBias
from .linear_layers import GeluMLP, SirenMLP, FiLMMLP
from .patching import HMLPEmbed, HMLPDebed
from .attention import AxialAttentionBlock, AttentionBlock
from .conv_layers import ResidualBlock, MiddleBlock, ClassicUnetBlock
