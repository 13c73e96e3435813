"""The normal-map U-Net's one-slice forward and the difference-map tail on the device
(csrc/unet.hip, dcs_unet_*; the 3x3 convolutions on the rows pass, dcs_conv_rows).

``plan_for(model)`` folds a modules/nmodel U-Net once (centre depth tap of every Conv3d, BatchNorm
as per-channel scale / shift; modules/nmodel/model.py::fold) and keeps the packed weights with it;
``forward`` runs a chunk of slices through it.  Activations are NHWC float32.  Per level:

    conv1 -> conv2 (prologue: affine + ReLU of conv1's output) -> affine + ReLU + 2x2 pool, which
    writes the skip into the leading channels of the level's concatenated tensor and the pooled map;
    on the way up the bilinear x2 upsample (affine + ReLU of its source on the fly, the pad split)
    writes the trailing channels, and the next conv reads one contiguous tensor.

Operand mode: the one of modules/hip/ops.py, through the mode its passes without a range record
run (ops._fallback: bf16x6 under the default f16x3, bf16 under f16; f32 stays f32).  An f16x3
range record is one power-of-two scale per call, so with it the result of a slice would depend on
the slices it shares a chunk with; the record-free modes keep every slice's result its own, and
BatchNorm scales of either sign need no derived record.

No CPU fallback: host tensors and unsupported models raise.
"""
from __future__ import annotations

import contextlib
import ctypes
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import lib
from .ops import ConvGeom, Src, _p, _stream

CHUNK_BYTES = 512 << 20  # the largest activation of a chunk (level 0's concatenated tensor)
TIMES = None  # scripts/bench_nmodel.py: a list that collects (label, start event, end event) per launch


@contextlib.contextmanager
def timed(label: str):
    """HIP events around one launch while ``TIMES`` is a list (the per-kernel table of the benchmark)."""
    if TIMES is None:
        yield
        return
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    yield
    b.record()
    TIMES.append((label, a, b))


class _Geom(ConvGeom):
    """A U-Net 3x3 conv on the plain rows pass: tap-major K order, no window-kernel planes."""
    kslice = property(lambda self: False)
    win = property(lambda self: False)


@dataclass
class _Conv:
    geom: _Geom
    weight: torch.Tensor          # [Cout,Cin,3,3], owner of the pack cache
    scale: torch.Tensor           # [Cout]
    shift: torch.Tensor
    cin_pad: Optional[int] = None

    @property
    def cout(self) -> int:
        return self.geom.cout


@dataclass
class Plan:
    enc: List[Tuple[_Conv, _Conv]]
    dec: List[Tuple[_Conv, _Conv]]
    out_weight: torch.Tensor      # [C]
    out_bias: float
    stamp: tuple

    @property
    def downs(self) -> int:
        return len(self.dec)


def _stamp(model, device) -> tuple:
    return (str(device),) + tuple((t.data_ptr(), t._version) for t in model.state_dict(keep_vars=True).values())


def plan_for(model, device) -> Plan:
    """The folded, device-resident form of ``model``, built once and kept on the model until its
    parameters or buffers change."""
    from ..nmodel.model import fold
    device = torch.device(device)
    stamp = _stamp(model, device)
    plan = getattr(model, "_dcs_unet_plan", None)
    if plan is not None and plan.stamp == stamp:
        return plan
    if not getattr(model, "trilinear", True):
        raise ValueError("the HIP path covers trilinear=True models only (no ConvTranspose3d up path)")
    if getattr(model, "n_channels", 1) != 1 or getattr(model, "n_classes", 1) != 1:
        raise ValueError("the HIP path covers one input channel and one output channel")
    f = fold(model, torch.float32)

    def conv(c, first=False):
        cout, cin = int(c.weight.shape[0]), int(c.weight.shape[1])
        if cout % 4 or cout <= 4 or (cin % 4 and not first):
            raise ValueError(f"the HIP path needs channel counts that are multiples of 4 and above 4 (got {cin} -> {cout})")
        return _Conv(_Geom(cin, cout, 3, 1, (1, 1, 1, 1), lib.DCS_PAD_ZERO), c.weight.to(device).contiguous(),
                     c.scale.to(device).contiguous(), c.shift.to(device).contiguous(), 4 if first else None)

    enc = [(conv(a, first=(i == 0)), conv(b)) for i, (a, b) in enumerate(f.enc)]
    dec = [(conv(a), conv(b)) for a, b in f.dec]
    for j, (a, _) in enumerate(dec):  # the concatenated tensor: skip channels, then the deeper level's
        skip_c = enc[len(dec) - 1 - j][1].cout
        deep_c = (enc[-1][1] if j == 0 else dec[j - 1][1]).cout
        if a.geom.cin != skip_c + deep_c:
            raise ValueError("up path: the conv's input channels are not skip + upsampled channels")
    plan = Plan(enc, dec, f.out_weight.reshape(-1).to(device).contiguous(), float(f.out_bias.reshape(-1)[0]), stamp)
    model._dcs_unet_plan = plan
    return plan


def default_chunk(plan: Plan, D: int, H: int, W: int) -> int:
    """Slices per call: every layer is per-slice, so this is a throughput and memory knob only."""
    per_slice = H * W * plan.dec[-1][0].geom.cin * 4
    return max(1, min(D, CHUNK_BYTES // max(per_slice, 1)))


# ---------------------------------------------------------------------------------------
# kernel wrappers
# ---------------------------------------------------------------------------------------
def _dev_f32(t: torch.Tensor, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name}: device tensor required (no CPU fallback)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name}: float32 required, got {t.dtype}")
    return t.contiguous()


def normalize_hu(hu: torch.Tensor, pad4: bool = False) -> torch.Tensor:
    """modules/nmodel/inference.py::normalize_hu of a float32 device tensor, bit for bit.  pad4: the
    result as [..., 4] pixels with zero channels 1..3 (the first convolution's source)."""
    hu = _dev_f32(hu, "normalize_hu")
    if hu.numel() == 0:
        raise ValueError("normalize_hu: empty tensor")
    out = torch.empty(hu.shape + ((4,) if pad4 else ()), dtype=torch.float32, device=hu.device)
    lib.call("dcs_unet_normalize_hu", _p(hu), hu.numel(), 4 if pad4 else 1, _p(out), _stream())
    return out


def affine_relu_pool(y: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, skip: Optional[torch.Tensor] = None):
    """a = relu(y * scale + shift) of an NHWC tensor and its 2x2 max pool (floor sizes) in one pass.
    ``skip``: an [N,H,W,Cs >= C] tensor whose leading C channels receive a (default: a new dense
    tensor).  Returns (skip, pooled)."""
    y, scale, shift = _dev_f32(y, "affine_relu_pool"), _dev_f32(scale, "affine_relu_pool"), _dev_f32(shift, "affine_relu_pool")
    N, H, W, C = y.shape
    if scale.numel() != C or shift.numel() != C:
        raise ValueError("affine_relu_pool: one scale / shift per channel")
    if skip is None:
        skip = torch.empty_like(y)
    if not skip.is_cuda or skip.dtype != torch.float32 or not skip.is_contiguous() or skip.dim() != 4 or \
            tuple(skip.shape[:3]) != (N, H, W) or skip.shape[3] < C:
        raise ValueError("affine_relu_pool: skip must be a contiguous float32 [N,H,W,>=C] device tensor")
    if H < 2 or W < 2:
        raise ValueError(f"affine_relu_pool: a {H}x{W} map has no 2x2 pool")
    pooled = torch.empty(N, H // 2, W // 2, C, dtype=torch.float32, device=y.device)
    lib.call("dcs_unet_affine_relu_pool", _p(y), _p(scale), _p(shift), N, H, W, C, _p(skip), skip.shape[3], _p(pooled),
             _stream())
    return skip, pooled


def upsample2_pad(x: torch.Tensor, size: Tuple[int, int], scale: Optional[torch.Tensor] = None,
                  shift: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, channel_offset: int = 0):
    """Bilinear x2 align_corners=True upsample of an NHWC tensor, centred in ``size`` = (Ho, Wo) by
    zero padding (size // 2 of the difference first).  scale / shift: read the source as
    relu(x * scale + shift).  ``out``: an [N,Ho,Wo,Cs] tensor receiving channels
    [channel_offset, channel_offset + C) (default: a new dense [N,Ho,Wo,C])."""
    x = _dev_f32(x, "upsample2_pad")
    N, h, w, C = x.shape
    Ho, Wo = int(size[0]), int(size[1])
    if Ho < 2 * h or Wo < 2 * w:
        raise ValueError("upsample2_pad: the target is smaller than the upsampled map")
    if (scale is None) != (shift is None):
        raise ValueError("upsample2_pad: scale and shift come together")
    if scale is not None:
        scale, shift = _dev_f32(scale, "upsample2_pad"), _dev_f32(shift, "upsample2_pad")
        if scale.numel() != C or shift.numel() != C:
            raise ValueError("upsample2_pad: one scale / shift per channel")
    if out is None:
        out, channel_offset = torch.empty(N, Ho, Wo, C, dtype=torch.float32, device=x.device), 0
    if not out.is_cuda or out.dtype != torch.float32 or not out.is_contiguous() or out.dim() != 4 or \
            tuple(out.shape[:3]) != (N, Ho, Wo) or channel_offset < 0 or channel_offset % 4 or \
            channel_offset + C > out.shape[3]:
        raise ValueError("upsample2_pad: out must be a contiguous float32 [N,Ho,Wo,Cs] device tensor with room for "
                         "C channels at a channel offset that is a multiple of 4")
    dst = ctypes.c_void_p(out.data_ptr() + 4 * channel_offset)
    lib.call("dcs_unet_upsample2_pad", _p(x), _p(scale), _p(shift), N, h, w, C, Ho, Wo, dst, out.shape[3], _stream())
    return out


def out_diffmap(y: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, weight: torch.Tensor, bias: float,
                threshold: float = 8, volume: Optional[torch.Tensor] = None, want_diff: bool = False):
    """The tail in one pass: affine + ReLU of the last conv output y [..., C], the 1x1 projection,
    denormalize_diff, and (with ``volume``, float32, one element per pixel of y) the threshold, uint8
    cast and add INTO ``volume``.  Returns the float difference map (un-thresholded, y's pixel shape)
    when ``want_diff``, else None."""
    y = _dev_f32(y, "out_diffmap")
    C = y.shape[-1]
    P = y.numel() // C
    scale, shift, weight = (_dev_f32(t, "out_diffmap") for t in (scale, shift, weight))
    if scale.numel() != C or shift.numel() != C or weight.numel() != C:
        raise ValueError("out_diffmap: one scale / shift / weight per channel")
    if volume is not None:
        if not volume.is_cuda or volume.dtype != torch.float32 or not volume.is_contiguous() or volume.numel() != P:
            raise ValueError("out_diffmap: volume must be a contiguous float32 device tensor, one element per pixel")
    elif not want_diff:
        raise ValueError("out_diffmap: nothing to compute")
    diff = torch.empty(y.shape[:-1], dtype=torch.float32, device=y.device) if want_diff else None
    lib.call("dcs_unet_out_diffmap", _p(y), _p(scale), _p(shift), _p(weight), float(bias), P, C,
             float(np.float32(threshold)), _p(volume), _p(volume), _p(diff), _stream())
    return diff


def apply_diffmap(volume: torch.Tensor, diff: torch.Tensor, threshold: float = 8) -> torch.Tensor:
    """modules/postprocess.py::apply_diffmap of two float32 device tensors -> a new float32 tensor."""
    volume, diff = _dev_f32(volume, "apply_diffmap"), _dev_f32(diff, "apply_diffmap")
    if volume.shape != diff.shape or volume.numel() == 0:
        raise ValueError("apply_diffmap: volume and diff must have one non-empty shape")
    out = torch.empty_like(volume)
    lib.call("dcs_unet_apply_diffmap", _p(diff), diff.numel(), float(np.float32(threshold)), _p(volume), _p(out),
             _stream())
    return out


# ---------------------------------------------------------------------------------------
# the forward
# ---------------------------------------------------------------------------------------
def _conv(c: _Conv, x: torch.Tensor, pro: Optional[_Conv] = None) -> torch.Tensor:
    """3x3 zero-pad conv of an NHWC tensor on the rows pass; ``pro``: the producing layer, whose
    affine + ReLU is applied to x while it is gathered."""
    N, H, W, Cs = x.shape
    g = c.geom
    wp = g.pack_fwd(c.weight, c.cin_pad)
    d = g._desc_fwd(Src.nhwc(x), wp.shape[1], lib.ACT_RELU if pro is not None else lib.ACT_NONE, lib.ACT_NONE)
    out = torch.empty(N, H, W, g.cout, dtype=torch.float32, device=x.device)
    psc = psh = None
    if pro is not None:  # the rows pass reads its prologue per (image, channel)
        psc, psh = pro.scale.expand(N, -1).contiguous(), pro.shift.expand(N, -1).contiguous()
    with timed(f"conv3x3 {Cs if c.cin_pad else g.cin}->{g.cout} @{H}x{W}" + (" +prologue" if pro is not None else "")):
        lib.call("dcs_conv_rows", ctypes.byref(d), _p(x), None, _p(wp), None, _p(psc), _p(psh), _p(out), _stream())
    return out


@torch.no_grad()
def forward(plan: Plan, x4: torch.Tensor):
    """A chunk of normalised slices [N,H,W,4] (normalize_hu(pad4=True)) through the U-Net up to its
    last 3x3 conv: returns (y [N,H,W,C], that layer's _Conv); the tail is ``out_diffmap``."""
    from ..nmodel.model import check_slice_size
    N, H, W, _ = x4.shape
    L = plan.downs
    check_slice_size(L, H, W)
    cats, cur = [], x4
    for lvl, (a, b) in enumerate(plan.enc):
        y = _conv(b, _conv(a, cur), pro=a)
        if lvl == L:
            break
        h, w = y.shape[1], y.shape[2]
        cat = torch.empty(N, h, w, plan.dec[L - 1 - lvl][0].geom.cin, dtype=torch.float32, device=y.device)
        with timed(f"affine+relu+pool {y.shape[3]} @{h}x{w}"):
            _, cur = affine_relu_pool(y, b.scale, b.shift, skip=cat)
        cats.append(cat)
    last = plan.enc[-1][1]
    for a, b in plan.dec:
        cat = cats.pop()
        with timed(f"upsample+pad {y.shape[3]} ->{cat.shape[1]}x{cat.shape[2]}"):
            upsample2_pad(y, cat.shape[1:3], last.scale, last.shift, out=cat, channel_offset=cat.shape[3] - y.shape[3])
        y = _conv(b, _conv(a, cat), pro=a)
        last = b
    return y, last
