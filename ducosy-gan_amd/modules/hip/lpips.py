"""LPIPS (lpips 0.1.4, net='alex') on the device: csrc/lpips.hip (dcs_lpips_*) for the first layer
and for the pass between the convolutions, the rows pass (dcs_conv_rows) for layers 2-5.

``plan_for(weights, device)`` folds the scaling layer into the first layer once and keeps the
device copies and packed weights with the LpipsWeights object; ``tap_sums`` runs both volumes
through the trunk in chunks of slices.  Per chunk and layer: one convolution launch over the
2n maps of both volumes (bias + ReLU in its epilogue), then one launch that reads that output
once for the tap's per-slice float64 sums and the max-pooled maps of the next layer.

Operand mode: bf16x6 (``MMA``), fixed here and independent of ops.set_mma.  An f16x3 range record
is one power-of-two scale per call, so with it a slice's value would depend on the slices it
shares a chunk with.  bf16x6 splits every fp32 operand into three bf16 parts that keep fp32's
exponent, so it needs no record and has no per-call state, as exact f32 has none; its error against
float64 is at or below the exact-f32 MFMA pass's (tests/test_gpu_mma.py) and its convolutions take
0.6 of the time (the patient's LPIPS 14.6 ms against 22.1 ms).  Every kernel
here reduces in an order that depends on the map size alone, so the chunk size is a memory knob only.

No CPU fallback: host tensors raise.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch

from .. import lpips_weights as LW
from . import lib
from .ops import ConvGeom, Src, _p, _stream
from .unet import timed

MMA = lib.MMA_BF16X6
CHUNK_BYTES = 512 << 20  # the feature maps of one chunk of both volumes


class _Geom(ConvGeom):
    """A trunk conv on the plain rows pass: tap-major K order, no window-kernel planes."""
    kslice = property(lambda self: False)
    win = property(lambda self: False)


@dataclass
class Plan:
    wx: torch.Tensor     # [121,64]: the first layer's weights of the image channel, tap-major
    cb: torch.Tensor     # [16,64]: bias + the constant channel's in-image tap sums per border class
    convs: List[Tuple[_Geom, torch.Tensor, torch.Tensor]]   # layers 2-5: geometry, weight, bias
    lins: List[torch.Tensor]
    stamp: tuple


def _stamp(weights, device) -> tuple:
    return (str(device),) + tuple((t.data_ptr(), t._version) for t in weights.tensors())


def _stem_tables(weights) -> Tuple[torch.Tensor, torch.Tensor]:
    """(wx [121,64], cb [16,64]) of dcs_lpips_stem in float32, folded and summed in float64."""
    wx, wc = LW.stem_fold(weights, torch.float64)
    bias = weights.convs[0][1].to(torch.float64)
    k = wx.shape[-1]
    spans = (slice(2, k), slice(0, k), slice(0, k - 1), slice(0, k - 2))   # the kernel rows / columns inside the image
    cb = torch.stack([bias + wc[:, ry, rx].sum((1, 2)) for ry in spans for rx in spans])
    return wx.reshape(wx.shape[0], -1).t().contiguous().float(), cb.contiguous().float()


def plan_for(weights, device) -> Plan:
    """The device-resident form of ``weights``, built once and kept on the object until its tensors change."""
    device = torch.device(device)
    stamp = _stamp(weights, device)
    plans = weights.__dict__.setdefault("_dcs_lpips_plans", {})
    plan = plans.get(str(device))
    if plan is not None and plan.stamp == stamp:
        return plan
    wx, cb = _stem_tables(weights)
    convs = []
    for (co, ci, k, _, pad, _), (w, b) in zip(LW.CONVS[1:], weights.convs[1:]):
        convs.append((_Geom(ci, co, k, 1, (pad,) * 4, lib.DCS_PAD_ZERO), w.to(device).contiguous(), b.to(device).contiguous()))
    plan = Plan(wx.to(device), cb.to(device), convs, [l.to(device).contiguous() for l in weights.lins], stamp)
    plans[str(device)] = plan
    return plan


def _dev_f32(t, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name}: device tensor required (no CPU fallback)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name}: float32 required, got {t.dtype}")
    return t.contiguous()


def stem(x: torch.Tensor, off: float, div: float, plan: Plan, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The first layer + ReLU of slices x [N,H,W] read as ((x - off) / div) * 2 - 1: [N,Ho,Wo,64]."""
    x = _dev_f32(x, "lpips stem")
    if x.dim() != 3 or min(x.shape[1:]) < 11 or x.shape[0] == 0:
        raise ValueError("lpips stem: [N,H,W] slices with sides of at least 11 are required")
    N, H, W = x.shape
    Ho, Wo = (H - 7) // 4 + 1, (W - 7) // 4 + 1
    if out is None:
        out = torch.empty(N, Ho, Wo, 64, dtype=torch.float32, device=x.device)
    assert out.is_contiguous() and tuple(out.shape) == (N, Ho, Wo, 64)
    with timed(f"stem 11x11/4 (x,1)->64 @{Ho}x{Wo}"):
        lib.call("dcs_lpips_stem", _p(x), N, H, W, float(off), float(div), _p(plan.wx), _p(plan.cb), _p(out), _stream())
    return out


def tap(f: torch.Tensor, lin: torch.Tensor, pool: bool = False):
    """One tap of the ReLU maps f [2N,h,w,C] of both volumes (the first volume's N slices, then the
    second's): (float64 [N] sums over the pixels of the ``lin``-weighted squared difference of the
    unit-normalised features, the 3x3 stride-2 max pool of f with floor sizes, or None unless
    ``pool``).  One read of f gives both."""
    f, lin = _dev_f32(f, "lpips tap"), _dev_f32(lin, "lpips tap")
    if f.dim() != 4 or f.shape[0] % 2 or f.numel() == 0 or lin.numel() != f.shape[3]:
        raise ValueError("lpips tap: [2N,h,w,C] maps of both volumes and one lin weight per channel are required")
    N, h, w, C = f.shape[0] // 2, f.shape[1], f.shape[2], f.shape[3]
    if pool and (h < 3 or w < 3):
        raise ValueError(f"lpips tap: a {h}x{w} map has no 3x3 pool")
    pooled = torch.empty(2 * N, (h - 3) // 2 + 1, (w - 3) // 2 + 1, C, dtype=torch.float32, device=f.device) if pool else None
    nws = lib.query("dcs_lpips_tap_workspace_size", N, h, w)
    ws = torch.empty(max(nws // 8, 1), dtype=torch.float64, device=f.device)
    out = torch.empty(N, dtype=torch.float64, device=f.device)
    with timed(f"tap {C} @{h}x{w}" + (" +pool" if pool else "")):
        lib.call("dcs_lpips_tap", _p(f[:N]), _p(f[N:]), N, h, w, C, _p(lin), _p(pooled[:N]) if pool else None,
                 _p(pooled[N:]) if pool else None, _p(out), _p(ws), nws, _stream())
    return out, pooled


def _conv(geom: _Geom, weight: torch.Tensor, bias: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """conv + bias + ReLU of an NHWC tensor on the rows pass, operand mode ``MMA``."""
    N, H, W, _ = x.shape
    wp = geom.pack_fwd(weight)
    d = geom._desc_fwd(Src.nhwc(x), wp.shape[1], lib.ACT_NONE, lib.ACT_RELU)
    d.mma = MMA
    out = torch.empty(N, H, W, geom.cout, dtype=torch.float32, device=x.device)
    with timed(f"conv{geom.k}x{geom.k} {geom.cin}->{geom.cout} @{H}x{W}"):
        lib.call("dcs_conv_rows", ctypes.byref(d), _p(x), None, _p(wp), _p(bias), None, None, _p(out), _stream())
    return out


def default_chunk(D: int, H: int, W: int) -> int:
    """Slices per pass: a memory knob only (a slice's value does not depend on it)."""
    per_slice = 2 * 4 * sum(h * w * c for (h, w), c in zip(LW.out_sizes(H, W), LW.CHANNELS))
    return max(1, min(D, CHUNK_BYTES // per_slice))


@torch.no_grad()
def tap_sums(a: torch.Tensor, b: torch.Tensor, affine, weights, chunk: Optional[int] = None) -> torch.Tensor:
    """float64 device [5,D]: per tap and slice the SUM over the map of the tap's distance (the mean
    divides by the map's pixels, LW.out_sizes).  a, b: float32 [D,H,W] device volumes, read as
    ((x - off) / div) * 2 - 1 with ``affine`` = (a_off, a_div, b_off, b_div)."""
    a, b = _dev_f32(a, "lpips"), _dev_f32(b, "lpips")
    if a.dim() != 3 or a.shape != b.shape or a.device != b.device or min(a.shape[1:]) < LW.MIN_SIDE:
        raise ValueError(f"lpips: two [D,H,W] volumes of one shape with sides of at least {LW.MIN_SIDE} are required")
    plan = plan_for(weights, a.device)
    D, H, W = a.shape
    n = default_chunk(D, H, W) if chunk is None else max(1, int(chunk))
    out = torch.empty(len(plan.lins), D, dtype=torch.float64, device=a.device)
    Ho, Wo = LW.out_sizes(H, W)[0]
    for i in range(0, D, n):
        m = min(n, D - i)
        f = torch.empty(2 * m, Ho, Wo, 64, dtype=torch.float32, device=a.device)   # both volumes: one conv launch per layer
        stem(a[i:i + m], affine[0], affine[1], plan, f[:m])
        stem(b[i:i + m], affine[2], affine[3], plan, f[m:])
        for k, lin in enumerate(plan.lins):
            if k:
                f = _conv(*plan.convs[k - 1], x)
            pool = k + 1 < len(LW.CONVS) and LW.CONVS[k + 1][5]
            out[k, i:i + m], pooled = tap(f, lin, pool)
            x = pooled if pool else f
    return out
