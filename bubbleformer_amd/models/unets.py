"""Upsample, Downsample, ModernUnet and ClassicUnet (mirror of bubbleformer/models/unets.py:10-320) on the native conv kernels
(csrc/conv.hip) and, for ClassicUnet's BatchNorm / GELU / max pool, csrc/bn.hip.

Constructor signatures, sub-module names and ``state_dict`` keys are the reference's.  One extra keyword, ``compute_dtype``, selects the
activation storage / MFMA type as in axial_vit.py: torch.float32 (default) is the exact-fp32 parity mode, torch.bfloat16 the throughput
mode.  Between layers the activations are channels-last (B, H, W, C); the clip is read and the prediction written in the reference's
(B, T, C, H, W) fp32 layout by the first and last conv.  ``forward_loss`` fuses the relative-L2 loss of modules.py:50.
"""
from typing import List

import torch
import torch.nn as nn

from .. import ops
from ..layers import ClassicUnetBlock, MiddleBlock, ResidualBlock
from ..layers.conv_layers import _check_gelu, _cl, bn_args
from ._api import register_model

__all__ = ["ModernUnet", "ClassicUnet", "Upsample", "Downsample"]


class Upsample(nn.Module):
    """ConvTranspose2d(C, C, 4, stride 2, pad 1): (B, C, H, W) -> (B, C, 2H, 2W)."""

    def __init__(self, in_channels: int):
        super().__init__()
        self.conv = nn.ConvTranspose2d(in_channels=in_channels, out_channels=in_channels, kernel_size=4, stride=2, padding=1)

    def forward_cl(self, x: torch.Tensor) -> torch.Tensor:
        return ops.unet_up(x, self.conv.weight, self.conv.bias)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.forward_cl(_cl(x)).permute(0, 3, 1, 2)


class Downsample(nn.Module):
    """Conv2d(C, C, 3, stride 2, pad 1): (B, C, H, W) -> (B, C, H/2, W/2)."""

    def __init__(self, in_channels: int):
        super().__init__()
        self.conv = nn.Conv2d(in_channels=in_channels, out_channels=in_channels, kernel_size=3, stride=2, padding=1)

    def forward_cl(self, x: torch.Tensor) -> torch.Tensor:
        return ops.unet_down(x, self.conv.weight, self.conv.bias)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.forward_cl(_cl(x)).permute(0, 3, 1, 2)


@register_model("unet_modern", listed=False)
class ModernUnet(nn.Module):
    def __init__(self, time_window: int = 5, input_fields: int = 4, output_fields: int = 4, hidden_channels: int = 32,
                 ch_mults: List[int] = [], norm: bool = True, compute_dtype=None):
        super().__init__()
        self.time_window = time_window
        self.input_fields = input_fields
        self.output_fields = output_fields
        self.hidden_channels = hidden_channels
        self.ch_mults = list(ch_mults)
        self.compute_dtype = compute_dtype if compute_dtype is not None else torch.float32
        ops._dt(self.compute_dtype)          # fp32 or bf16 only

        self.activation = nn.GELU()
        in_channels = input_fields * time_window
        final_out = output_fields * time_window
        self.image_proj = nn.Conv2d(in_channels, hidden_channels, kernel_size=1)
        n_resolutions = len(ch_mults)
        down = []
        out_channels = in_channels = hidden_channels
        for i in range(n_resolutions):
            out_channels = in_channels * ch_mults[i]
            for _ in range(2):
                down.append(ResidualBlock(in_channels, out_channels))
                in_channels = out_channels
            if i < n_resolutions - 1:
                down.append(Downsample(in_channels))
        self.down = nn.ModuleList(down)
        self.middle = MiddleBlock(out_channels)
        up = []
        in_channels = out_channels
        for i in reversed(range(n_resolutions)):
            out_channels = in_channels
            for _ in range(2):
                up.append(ResidualBlock(in_channels + out_channels, out_channels))
            out_channels = in_channels // ch_mults[i]
            up.append(ResidualBlock(in_channels + out_channels, out_channels))
            in_channels = out_channels
            if i > 0:
                up.append(Upsample(in_channels))
        self.up = nn.ModuleList(up)
        if norm:
            if in_channels % ops.GN_GROUPS:
                raise ValueError(f"GroupNorm({ops.GN_GROUPS}) cannot divide {in_channels} channels")
            self.norm = nn.GroupNorm(8, in_channels)
        else:
            self.norm = nn.Identity()
        self.final = nn.Conv2d(in_channels, final_out, kernel_size=1)
        # the reference's ResidualBlocks are built with norm=True whatever `norm` says (unets.py:107-138); only the final norm follows it
        _check_gelu(self.activation)

    def _check_input(self, x: torch.Tensor) -> None:
        if x.dim() != 5 or x.shape[1] != self.time_window or x.shape[2] != self.input_fields:
            raise ValueError(f"expected (B, {self.time_window}, {self.input_fields}, H, W), got {tuple(x.shape)}")
        div = 2 ** max(len(self.ch_mults) - 1, 0)
        if x.shape[3] % div or x.shape[4] % div:
            raise ValueError(f"H and W must be divisible by 2^(len(ch_mults)-1) = {div}; got {x.shape[3]} x {x.shape[4]}")

    def _trunk(self, x: torch.Tensor) -> torch.Tensor:
        self._check_input(x)
        x = ops.unet_proj(x, self.image_proj.weight, self.image_proj.bias, self.compute_dtype)
        h = [x]
        for m in self.down:
            x = m.forward_cl(x)
            h.append(x)
        x = self.middle.forward_cl(x)
        for m in self.up:
            if isinstance(m, Upsample):
                x = m.forward_cl(x)
            else:
                x = m.forward_cl(x, h.pop())
        return x

    def _final(self, x, target=None):
        gn = isinstance(self.norm, nn.GroupNorm)
        return ops.unet_final(x, self.time_window, self.norm.weight if gn else None, self.norm.bias if gn else None, self.final.weight,
                              self.final.bias, target)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x: (B, T, C, H, W) -> (B, T, C_out, H, W) fp32."""
        pred, _ = self._final(self._trunk(x))
        return pred

    def forward_loss(self, x: torch.Tensor, target: torch.Tensor):
        """Fused final conv + relative-L2 loss (LpLoss d=2, p=2, mean B, mean T, sum C; modules.py:50): (loss, prediction)."""
        pred, loss = self._final(self._trunk(x), target)
        return loss, pred.detach()


@register_model("unet_classic", listed=False)
class ClassicUnet(nn.Module):
    """Classic U-Net (Ronneberger et al. 2015): four encoders with 2x2 max pooling, a bottleneck, four ConvTranspose2d(k2, s2) + decoder
    stages on channel-concatenated skips, and a 1x1 conv.  Each block is conv -> BatchNorm2d -> GELU twice.

    Batch statistics: in train() mode every BatchNorm2d normalises with the statistics of the local batch and updates its running buffers
    on the device; under data parallelism (trainer.TrainStep) each rank does so with its own batch, which is the reference's DDP without
    SyncBatchNorm.  The buffers are never exchanged: checkpoints are written from rank 0, whose buffers have only seen rank 0's batches, as
    under DDP's broadcast_buffers.  In eval() mode the running statistics are used and the forward never synchronises with the host."""

    def __init__(self, time_window: int = 5, input_fields: int = 4, output_fields: int = 4, hidden_channels: int = 32, compute_dtype=None):
        super().__init__()
        self.time_window = time_window
        self.input_fields = input_fields
        self.output_fields = output_fields
        self.hidden_channels = hidden_channels
        self.compute_dtype = compute_dtype if compute_dtype is not None else torch.float32
        ops._dt(self.compute_dtype)          # fp32 or bf16 only
        h = hidden_channels
        self.encoder1 = ClassicUnetBlock(in_channels=input_fields * time_window, out_channels=h)
        self.pool1 = nn.MaxPool2d(kernel_size=2, stride=2)
        self.encoder2 = ClassicUnetBlock(in_channels=h, out_channels=h * 2)
        self.pool2 = nn.MaxPool2d(kernel_size=2, stride=2)
        self.encoder3 = ClassicUnetBlock(in_channels=h * 2, out_channels=h * 4)
        self.pool3 = nn.MaxPool2d(kernel_size=2, stride=2)
        self.encoder4 = ClassicUnetBlock(in_channels=h * 4, out_channels=h * 8)
        self.pool4 = nn.MaxPool2d(kernel_size=2, stride=2)
        self.bottleneck = ClassicUnetBlock(in_channels=h * 8, out_channels=h * 16)
        self.upconv4 = nn.ConvTranspose2d(in_channels=h * 16, out_channels=h * 8, kernel_size=2, stride=2)
        self.decoder4 = ClassicUnetBlock(in_channels=h * 16, out_channels=h * 8)
        self.upconv3 = nn.ConvTranspose2d(in_channels=h * 8, out_channels=h * 4, kernel_size=2, stride=2)
        self.decoder3 = ClassicUnetBlock(in_channels=h * 8, out_channels=h * 4)
        self.upconv2 = nn.ConvTranspose2d(in_channels=h * 4, out_channels=h * 2, kernel_size=2, stride=2)
        self.decoder2 = ClassicUnetBlock(in_channels=h * 4, out_channels=h * 2)
        self.upconv1 = nn.ConvTranspose2d(in_channels=h * 2, out_channels=h, kernel_size=2, stride=2)
        self.decoder1 = ClassicUnetBlock(in_channels=h * 2, out_channels=h)
        self.conv = nn.Conv2d(in_channels=h, out_channels=output_fields * time_window, kernel_size=1)

    def _check_input(self, x: torch.Tensor) -> None:
        if x.dim() != 5 or x.shape[1] != self.time_window or x.shape[2] != self.input_fields:
            raise ValueError(f"expected (B, {self.time_window}, {self.input_fields}, H, W), got {tuple(x.shape)}")
        if x.shape[3] % 16 or x.shape[4] % 16:
            raise ValueError(f"H and W must be divisible by 16 (four 2x2 poolings); got {x.shape[3]} x {x.shape[4]}")
        if self.training and x.shape[0] * (x.shape[3] // 16) * (x.shape[4] // 16) == 1:
            raise ValueError("Expected more than 1 value per channel when training, got input size "
                             f"{[1, self.hidden_channels * 16, 1, 1]}")

    def _trunk(self, x: torch.Tensor) -> torch.Tensor:
        """-> the raw conv2 output of decoder1 (its norm2 + act2 are the final conv's prologue)."""
        self._check_input(x)
        ops._require_gpu(x)
        dt = self.compute_dtype
        x = x.contiguous().float()
        skips = []
        h = None
        for i, enc in enumerate((self.encoder1, self.encoder2, self.encoder3, self.encoder4)):
            c = enc.forward_conv(x, compute_dtype=dt, nchw=True) if i == 0 else enc.forward_conv(h, compute_dtype=dt)
            a, port, h = enc.act(c, pool=True)
            skips.append((a, port))
        a, port = self.bottleneck.act(self.bottleneck.forward_conv(h, compute_dtype=dt))
        for up, dec in ((self.upconv4, self.decoder4), (self.upconv3, self.decoder3), (self.upconv2, self.decoder2),
                        (self.upconv1, self.decoder1)):
            u = ops.unet_upconv2(a, up.weight, up.bias, port)
            s, sport = skips.pop()
            c = dec.forward_conv(u, s, sport, compute_dtype=dt)
            if dec is not self.decoder1:
                a, port = dec.act(c)
        return c

    def _final(self, c, target=None):
        n = self.decoder1.norm2
        _check_gelu(self.decoder1.act2)
        return ops.classic_final(c, self.time_window, n.weight, n.bias, bn_args(n), self.conv.weight, self.conv.bias, target)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x: (B, T, C, H, W) -> (B, T, C_out, H, W) fp32."""
        pred, _ = self._final(self._trunk(x))
        return pred

    def forward_loss(self, x: torch.Tensor, target: torch.Tensor):
        """Fused final conv + relative-L2 loss (LpLoss d=2, p=2, mean B, mean T, sum C; modules.py:50): (loss, prediction)."""
        pred, loss = self._final(self._trunk(x), target)
        return loss, pred.detach()
