"""The normal-map U-Net of the reference's modules/nmodel/model.py (UNet3D, UNet3DLight): the model
that predicts a contrast difference map from an NCCT slice.

The classes restate the reference's layer structure so that their ``state_dict`` keys and shapes
are the reference's and its checkpoints load with ``load_state_dict``.  Their ``forward`` is plain
ATen: the CPU path and the test oracle.  On the GPU the inference path does not call it; it runs
the folded 2-D form below on the HIP kernels (modules/hip/unet.py).

Inference feeds the model one slice at a time, a [1,1,1,H,W] tensor, so every layer degenerates:
a Conv3d(k=3, padding=1) sees only its centre depth tap, BatchNorm3d in eval mode is a per-channel
affine map, MaxPool3d((1,2,2)) a 2x2 max pool, the trilinear (1,2,2) upsample a bilinear one.
``fold`` extracts that form once per model and ``forward_folded`` runs it with ATen; the device
path consumes the same ``Folded`` record.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F


def _conv_bn_relu(cin: int, cout: int) -> List[nn.Module]:
    return [nn.Conv3d(cin, cout, kernel_size=3, padding=1, bias=False), nn.BatchNorm3d(cout), nn.ReLU(inplace=True)]


class DoubleConv(nn.Module):
    """Two rounds of 3x3x3 convolution, BatchNorm and ReLU (cin -> mid -> cout)."""

    def __init__(self, in_channels: int, out_channels: int, mid_channels: int = None):
        super().__init__()
        mid = mid_channels or out_channels
        self.double_conv = nn.Sequential(*_conv_bn_relu(in_channels, mid), *_conv_bn_relu(mid, out_channels))

    def forward(self, x):
        return self.double_conv(x)


class Down(nn.Module):
    """In-plane 2x2 max pool (depth untouched), then a DoubleConv."""

    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        self.maxpool_conv = nn.Sequential(nn.MaxPool3d(kernel_size=(1, 2, 2), stride=(1, 2, 2)),
                                          DoubleConv(in_channels, out_channels))

    def forward(self, x):
        return self.maxpool_conv(x)


class Up(nn.Module):
    """In-plane x2 upsample of the deeper map, centred inside the skip's size by zero padding,
    concatenated behind the skip, then a DoubleConv."""

    def __init__(self, in_channels: int, out_channels: int, trilinear: bool = True):
        super().__init__()
        if trilinear:
            self.up = nn.Upsample(scale_factor=(1, 2, 2), mode="trilinear", align_corners=True)
            self.conv = DoubleConv(in_channels, out_channels, in_channels // 2)
        else:
            self.up = nn.ConvTranspose3d(in_channels, in_channels // 2, kernel_size=(1, 2, 2), stride=(1, 2, 2))
            self.conv = DoubleConv(in_channels, out_channels)

    def forward(self, deep, skip):
        deep = self.up(deep)
        pads = []
        for axis in (4, 3, 2):  # F.pad lists the last axis first
            d = skip.size(axis) - deep.size(axis)
            pads += [d // 2, d - d // 2]
        return self.conv(torch.cat([skip, F.pad(deep, pads)], dim=1))


class OutConv(nn.Module):
    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        self.conv = nn.Conv3d(in_channels, out_channels, kernel_size=1)

    def forward(self, x):
        return self.conv(x)


class _UNet(nn.Module):
    """inc, down1..downN, up1..upN, outc; the deepest Down halves its width when ``trilinear``."""
    DOWNS = 0

    def __init__(self, n_channels: int, n_classes: int, trilinear: bool, base_channels: int):
        super().__init__()
        self.n_channels, self.n_classes, self.trilinear = n_channels, n_classes, trilinear
        self.base_channels = base_channels
        n, b, factor = self.DOWNS, base_channels, 2 if trilinear else 1
        self.inc = DoubleConv(n_channels, b)
        for i in range(1, n + 1):
            cout = (b << i) // factor if i == n else b << i
            setattr(self, f"down{i}", Down(b << (i - 1), cout))
        for i in range(1, n + 1):
            cin = b << (n - i + 1)
            cout = b if i == n else (cin // 2) // factor
            setattr(self, f"up{i}", Up(cin, cout, trilinear))
        self.outc = OutConv(b, n_classes)

    def forward(self, x):
        skips = [self.inc(x)]
        for i in range(1, self.DOWNS + 1):
            skips.append(getattr(self, f"down{i}")(skips[-1]))
        x = skips.pop()
        for i in range(1, self.DOWNS + 1):
            x = getattr(self, f"up{i}")(x, skips.pop())
        return self.outc(x)


class UNet3D(_UNet):
    """The full model: 4 downs, base 32 by default."""
    DOWNS = 4

    def __init__(self, n_channels=1, n_classes=1, trilinear=True, base_channels=32):
        super().__init__(n_channels, n_classes, trilinear, base_channels)


class UNet3DLight(_UNet):
    """The light model: 3 downs, base 16 by default."""
    DOWNS = 3

    def __init__(self, n_channels=1, n_classes=1, trilinear=True, base_channels=16):
        super().__init__(n_channels, n_classes, trilinear, base_channels)


# ---------------------------------------------------------------------------------------
# the folded 2-D form of a one-slice forward
# ---------------------------------------------------------------------------------------
@dataclass
class FoldedConv:
    """One conv + BatchNorm + ReLU: ``weight`` [Cout,Cin,3,3] is the centre depth tap, the BatchNorm is
    relu(y * scale + shift) per channel with scale = gamma / sqrt(var + eps) (either sign) and
    shift = beta - mean * scale."""
    weight: torch.Tensor
    scale: torch.Tensor
    shift: torch.Tensor


@dataclass
class Folded:
    enc: List[Tuple[FoldedConv, FoldedConv]]   # inc, down1 .. downN
    dec: List[Tuple[FoldedConv, FoldedConv]]   # up1 .. upN
    out_weight: torch.Tensor                   # [Cout, C] of the 1x1 convolution
    out_bias: torch.Tensor                     # [Cout]

    @property
    def downs(self) -> int:
        return len(self.dec)


def check_slice_size(downs: int, H: int, W: int) -> None:
    """A slice must keep at least one pixel per axis through every pool."""
    if H >> downs < 1 or W >> downs < 1:
        raise ValueError(f"a {H}x{W} slice does not survive {downs} 2x2 pools (at least {1 << downs} pixels per axis)")


def _fold_conv(conv: nn.Conv3d, bn: nn.BatchNorm3d, dtype) -> FoldedConv:
    if tuple(conv.kernel_size) != (3, 3, 3) or tuple(conv.padding) != (1, 1, 1) or conv.bias is not None:
        raise ValueError("fold: 3x3x3 convolutions with padding 1 and no bias expected")
    if bn.running_mean is None or bn.running_var is None:
        raise ValueError("fold: BatchNorm without running statistics")
    f64 = lambda t: t.detach().to(torch.float64)
    gamma = f64(bn.weight) if bn.weight is not None else torch.ones_like(f64(bn.running_var))
    beta = f64(bn.bias) if bn.bias is not None else torch.zeros_like(gamma)
    scale = gamma / torch.sqrt(f64(bn.running_var) + bn.eps)
    shift = beta - f64(bn.running_mean) * scale
    return FoldedConv(conv.weight.detach()[:, :, 1].to(dtype).contiguous(), scale.to(dtype).contiguous(),
                      shift.to(dtype).contiguous())


def _fold_double(dc: DoubleConv, dtype) -> Tuple[FoldedConv, FoldedConv]:
    s = dc.double_conv
    return _fold_conv(s[0], s[1], dtype), _fold_conv(s[3], s[4], dtype)


def fold(model: _UNet, dtype=torch.float32) -> Folded:
    """The one-slice form of ``model`` (eval-mode BatchNorm), its tensors on the model's device in
    ``dtype``; scale and shift are formed in float64 first.  ``trilinear`` models only."""
    if not getattr(model, "trilinear", True):
        raise ValueError("fold: the ConvTranspose3d up path (trilinear=False) has no folded form here")
    n = model.DOWNS
    enc = [_fold_double(model.inc, dtype)] + [_fold_double(getattr(model, f"down{i}").maxpool_conv[1], dtype)
                                             for i in range(1, n + 1)]
    dec = [_fold_double(getattr(model, f"up{i}").conv, dtype) for i in range(1, n + 1)]
    oc = model.outc.conv
    return Folded(enc, dec, oc.weight.detach().reshape(oc.out_channels, oc.in_channels).to(dtype).contiguous(),
                  oc.bias.detach().to(dtype).contiguous())


def forward_folded(f: Folded, x: torch.Tensor) -> torch.Tensor:
    """``model(x[:, :, None])[:, :, 0]`` of a [N,Cin,H,W] batch of slices from the folded record, with
    ATen: centre-tap convolution, folded affine + ReLU, 2x2 pool, bilinear align_corners upsample,
    the pad split, concatenation behind the skip, 1x1 projection."""
    check_slice_size(f.downs, x.shape[-2], x.shape[-1])

    def double(x, pair):
        for c in pair:
            x = F.conv2d(x, c.weight, padding=1)
            x = F.relu(x * c.scale.view(1, -1, 1, 1) + c.shift.view(1, -1, 1, 1))
        return x

    skips = [double(x, f.enc[0])]
    for pair in f.enc[1:]:
        skips.append(double(F.max_pool2d(skips[-1], 2), pair))
    x = skips.pop()
    for pair in f.dec:
        skip = skips.pop()
        x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
        dh, dw = skip.shape[-2] - x.shape[-2], skip.shape[-1] - x.shape[-1]
        x = F.pad(x, [dw // 2, dw - dw // 2, dh // 2, dh - dh // 2])
        x = double(torch.cat([skip, x], dim=1), pair)
    return F.conv2d(x, f.out_weight[:, :, None, None], f.out_bias)
