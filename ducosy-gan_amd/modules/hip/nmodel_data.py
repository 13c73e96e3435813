"""Device wrapper of the training-target kernel of the normal-map U-Net (csrc/nmodel_data.hip,
dcs_nmodel_targets): modules/nmodel/prepare.py::residual_targets on resident series.

Conventions of modules/hip/slices.py: device tensors only (no CPU fallback), a bad argument raises
before anything is launched, the kernels go to the current stream, ``with torch.cuda.device(...)``
is left to the caller.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import lib
from .lib import ptr as _p, stream as _stream

NSTATS = lib.NMODEL_NSTATS


def _stored(t, unsigned: bool, name: str):
    """(the 16-bit series as a contiguous int16 tensor, unsigned flag)"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"residual_targets: {name}: device tensor required (no CPU fallback)")
    if hasattr(torch, "uint16") and t.dtype == torch.uint16:
        t, unsigned = t.view(torch.int16), True
    if t.dtype != torch.int16:
        raise RuntimeError(f"residual_targets: {name}: unsupported dtype {t.dtype} (int16, or uint16 bits, required)")
    if t.dim() != 3 or t.numel() == 0:
        raise ValueError(f"residual_targets: {name}: non-empty [D,H,W] series required")
    return t.contiguous(), bool(unsigned)


def _per_slice(v, D: int, device, name: str) -> torch.Tensor:
    v = torch.as_tensor(v).to(device=device, dtype=torch.float32).reshape(-1).contiguous()
    if v.numel() != D:
        raise ValueError(f"residual_targets: {name}: one value per slice")
    return v


def residual_targets(ncct: torch.Tensor, ncct_slopes, ncct_intercepts, cect: torch.Tensor, cect_slopes,
                     cect_intercepts, merged: Optional[torch.Tensor] = None, threshold: float = 8.0,
                     ncct_unsigned: bool = False, cect_unsigned: bool = False):
    """``modules/nmodel/prepare.py::residual_targets`` in one kernel pass.

    ncct, cect: int16 [D,H,W] device tensors (the bits of a uint16 series with its ``*_unsigned``
    flag; a torch.uint16 tensor sets the flag itself).  Slopes / intercepts: one per slice, any
    tensor or sequence, read as float32.  merged: float32 [D,H,W] on the same device or None; it is
    only read.  Returns (vue float32 [D,H,W], diff float32 [D,H,W], stats float64 [D,11]) on the
    device; vue and diff equal the host function's bit for bit."""
    ncct, nu = _stored(ncct, ncct_unsigned, "ncct")
    cect, cu = _stored(cect, cect_unsigned, "cect")
    if ncct.shape != cect.shape:
        raise ValueError(f"residual_targets: the series differ in shape: ncct {tuple(ncct.shape)}, "
                         f"cect {tuple(cect.shape)}")
    if cect.device != ncct.device:
        raise ValueError("residual_targets: operands on different devices")
    D, H, W = ncct.shape
    if merged is not None:
        if not isinstance(merged, torch.Tensor) or not merged.is_cuda:
            raise RuntimeError("residual_targets: merged: device tensor required (no CPU fallback)")
        if merged.dtype != torch.float32:
            raise RuntimeError(f"residual_targets: merged: float32 required, got {merged.dtype}")
        if merged.shape != ncct.shape:
            raise ValueError(f"residual_targets: merged {tuple(merged.shape)} differs in shape from the series "
                             f"{tuple(ncct.shape)}")
        if merged.device != ncct.device:
            raise ValueError("residual_targets: operands on different devices")
        merged = merged.contiguous()
    dev = ncct.device
    sn, in_ = _per_slice(ncct_slopes, D, dev, "ncct_slopes"), _per_slice(ncct_intercepts, D, dev, "ncct_intercepts")
    sc, ic = _per_slice(cect_slopes, D, dev, "cect_slopes"), _per_slice(cect_intercepts, D, dev, "cect_intercepts")
    nbytes = lib.query("dcs_nmodel_targets_workspace_size", D, H, W)
    if nbytes == 0:
        raise ValueError(f"residual_targets: unsupported volume shape {(D, H, W)}")
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    vue = torch.empty((D, H, W), dtype=torch.float32, device=dev)
    diff = torch.empty((D, H, W), dtype=torch.float32, device=dev)
    stats = torch.empty((D, NSTATS), dtype=torch.float64, device=dev)
    lib.call("dcs_nmodel_targets", _p(ncct), int(nu), _p(sn), _p(in_), _p(cect), int(cu), _p(sc), _p(ic), _p(merged),
             D, H, W, float(threshold), _p(vue), _p(diff), _p(stats), _p(ws), nbytes, _stream())
    return vue, diff, stats
