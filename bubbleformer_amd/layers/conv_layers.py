"""ResidualBlock and MiddleBlock -- mirror of bubbleformer/layers/conv_layers.py:5-86 (the ModernUnet blocks) -- and ClassicUnetBlock
(conv_layers.py:96-141, the ClassicUnet block).

Constructor signatures, sub-module names and ``state_dict`` keys are the reference's; the sub-modules only hold the parameters.
``forward`` takes the reference's (B, C, H, W) tensor; inside the U-Net the blocks exchange channels-last (B, H, W, C) tensors in the
compute dtype through ``forward_cl`` (ops.res_block: GroupNorm statistics, then two implicit-GEMM 3x3 convs with the GroupNorm affine +
GELU applied while the operand is staged, shortcut and residual add in the second conv's epilogue).
"""
import torch
import torch.nn as nn

from .. import ops

__all__ = ["ResidualBlock", "MiddleBlock", "ClassicUnetBlock"]


def _check_gelu(activation) -> None:
    if not (isinstance(activation, nn.GELU) and activation.approximate == "none"):
        raise NotImplementedError("the native blocks implement nn.GELU() (exact erf), the reference's only activation")


def _cl(x: torch.Tensor) -> torch.Tensor:
    return x.permute(0, 2, 3, 1).contiguous()


class ResidualBlock(nn.Module):
    def __init__(self, in_channels: int, out_channels: int, activation: nn.Module = nn.GELU(), norm: bool = True, n_groups: int = 8):
        super().__init__()
        _check_gelu(activation)
        if n_groups != ops.GN_GROUPS:
            raise NotImplementedError(f"n_groups={n_groups}: the native GroupNorm uses {ops.GN_GROUPS} groups, as every reference block does")
        if norm and (in_channels % n_groups or out_channels % n_groups):
            raise ValueError(f"GroupNorm({n_groups}) cannot divide {in_channels} / {out_channels} channels")
        self.activation = activation
        self.conv1 = nn.Conv2d(in_channels, out_channels, kernel_size=(3, 3), padding=(1, 1))
        self.conv2 = nn.Conv2d(out_channels, out_channels, kernel_size=(3, 3), padding=(1, 1))
        self.shortcut = nn.Conv2d(in_channels, out_channels, kernel_size=(1, 1)) if in_channels != out_channels else nn.Identity()
        if norm:
            self.norm1 = nn.GroupNorm(n_groups, in_channels)
            self.norm2 = nn.GroupNorm(n_groups, out_channels)
        else:
            self.norm1 = nn.Identity()
            self.norm2 = nn.Identity()

    def forward_cl(self, x: torch.Tensor, skip: torch.Tensor = None) -> torch.Tensor:
        """x, skip: (B, H, W, C) channels-last; the block's input is cat(x, skip) along channels (never materialised)."""
        n1, n2 = self.norm1, self.norm2
        gn = isinstance(n1, nn.GroupNorm)
        sc = self.shortcut if isinstance(self.shortcut, nn.Conv2d) else None
        return ops.res_block(x, skip, n1.weight if gn else None, n1.bias if gn else None, self.conv1.weight, self.conv1.bias,
                             n2.weight if gn else None, n2.bias if gn else None, self.conv2.weight, self.conv2.bias,
                             sc.weight if sc is not None else None, sc.bias if sc is not None else None)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x: (B, in_ch, H, W) -> (B, out_ch, H, W) (a permuted view of channels-last memory)."""
        return self.forward_cl(_cl(x)).permute(0, 3, 1, 2)


class MiddleBlock(nn.Module):
    def __init__(self, in_channels: int, activation: nn.Module = nn.GELU(), norm: bool = True):
        super().__init__()
        self.res1 = ResidualBlock(in_channels=in_channels, out_channels=in_channels, activation=activation, norm=norm)
        self.res2 = ResidualBlock(in_channels=in_channels, out_channels=in_channels, activation=activation, norm=norm)

    def forward_cl(self, x: torch.Tensor) -> torch.Tensor:
        return self.res2.forward_cl(self.res1.forward_cl(x))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.forward_cl(_cl(x)).permute(0, 3, 1, 2)


def bn_args(norm: nn.BatchNorm2d):
    """(running_mean, running_var, num_batches_tracked, eps, momentum, training) of a BatchNorm2d, as ops' classic functions take them."""
    if not (norm.affine and norm.track_running_stats):
        raise NotImplementedError("the native BatchNorm2d needs affine=True and track_running_stats=True, as the reference builds it")
    if norm.momentum is None:
        raise NotImplementedError("BatchNorm2d(momentum=None) (cumulative moving average) is not implemented; the reference uses 0.1")
    return (norm.running_mean, norm.running_var, norm.num_batches_tracked, float(norm.eps), float(norm.momentum), norm.training)


class ClassicUnetBlock(nn.Module):
    """conv1 (3x3, no bias) -> norm1 (BatchNorm2d) -> act1 (GELU) -> conv2 -> norm2 -> act2.  The norms are real nn.BatchNorm2d modules:
    train() / eval() select batch or running statistics, and training forwards update the running buffers on the device.

    Inside the U-Net the block is split in two (ops.classic_conv / ops.classic_act or ops.classic_final): ``forward_conv`` returns the raw
    conv2 output and the consumer applies norm2 + act2 -- materialised with the encoders' 2x2 max pool, or as the final conv's prologue."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.conv1 = nn.Conv2d(in_channels=in_channels, out_channels=out_channels, kernel_size=3, padding=1, bias=False)
        self.norm1 = nn.BatchNorm2d(num_features=out_channels)
        self.act1 = nn.GELU()
        self.conv2 = nn.Conv2d(in_channels=out_channels, out_channels=out_channels, kernel_size=3, padding=1, bias=False)
        self.norm2 = nn.BatchNorm2d(num_features=out_channels)
        self.act2 = nn.GELU()

    def forward_conv(self, x, skip=None, skip_port=None, compute_dtype=None, nchw=False):
        """x (B, H, W, C) channels-last (or, with nchw, the (B, T, C, H, W) fp32 clip), skip: the decoder's skip activation, concatenated
        after x.  -> raw conv2 output (B, H, W, out_channels)."""
        _check_gelu(self.act1)
        dt = compute_dtype if compute_dtype is not None else x.dtype
        return ops.classic_conv(x, skip, skip_port, self.conv1.weight, self.norm1.weight, self.norm1.bias, self.conv2.weight,
                                bn_args(self.norm1), dt, nchw)

    def act(self, c, pool=False):
        """norm2 + act2 of forward_conv's output -> (a, port) or (a, port, maxpool2x2(a))."""
        _check_gelu(self.act2)
        return ops.classic_act(c, self.norm2.weight, self.norm2.bias, bn_args(self.norm2), pool)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x: (B, in_ch, H, W) -> (B, out_ch, H, W) (a permuted view of channels-last memory)."""
        return self.act(self.forward_conv(_cl(x)))[0].permute(0, 3, 1, 2)
