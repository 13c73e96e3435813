"""Device wrappers of the slice-series kernels (csrc/slices.hip): the antialiased and nearest
resizes of [N,C,H,W] float32 tensors and the fused model-output -> stored-value -> merge kernels
(the HU-range merge and the enhancement-difference merge).

Conventions of modules/hip/volume.py: device tensors only (no CPU fallback), a bad argument
raises, kernels go to the current stream, ``with torch.cuda.device(...)`` is left to the caller.
``aa_tables`` is pure numpy and needs no GPU.
"""
from __future__ import annotations

from functools import lru_cache
from typing import Optional, Tuple

import numpy as np
import torch

from . import lib
from .lib import ptr as _p, stream as _stream

MAX_TAPS = lib.RESIZE_MAX_TAPS
MAX_RATIO = 8  # in/out above this needs more than MAX_TAPS taps


@lru_cache(maxsize=64)
def aa_tables(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Taps of the antialiased bilinear (triangle) filter that takes ``in_size`` samples to
    ``out_size`` (torch's F.interpolate(mode="bilinear", align_corners=False, antialias=True)
    along one axis), in float32: (start int32 [out], count int32 [out], weights float32
    [out, taps]) with taps = count.max(); a row's weights beyond its count are 0.  Output i is
    sum_j weights[i, j] * x[start[i] + j], accumulated in tap order."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError("aa_tables: sizes must be positive")
    if in_size > MAX_RATIO * out_size:
        raise ValueError(f"aa_tables: in/out = {in_size}/{out_size} above {MAX_RATIO} is not supported")
    f = np.float32
    scale = f(in_size / out_size)
    support = scale if scale >= 1 else f(1)
    inv = f(1) / scale if scale >= 1 else f(1)
    center = scale * (np.arange(out_size, dtype=f) + f(0.5))
    start = np.maximum((center - support + f(0.5)).astype(np.int64), 0)
    count = np.minimum((center + support + f(0.5)).astype(np.int64), in_size) - start
    taps = int(count.max())
    if count.min() < 1 or taps > MAX_TAPS:
        raise ValueError(f"aa_tables: tap counts {int(count.min())}..{taps} outside 1..{MAX_TAPS}")
    w = np.zeros((out_size, taps), f)
    total = np.zeros(out_size, f)
    for j in range(taps):
        x = ((f(j) + start.astype(f)) - center + f(0.5)) * inv
        w[:, j] = np.where(j < count, np.maximum(f(0), f(1) - np.abs(x)), f(0))
        total = total + w[:, j]      # the sequential float32 sum
    w /= total[:, None]
    out = (start.astype(np.int32), count.astype(np.int32), w)
    for a in out:  # the cache hands the same arrays to every caller
        a.setflags(write=False)
    return out


def _nchw(x, name: str) -> torch.Tensor:
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError(f"{name}: device tensor required (no CPU fallback)")
    if x.dtype != torch.float32:
        raise RuntimeError(f"{name}: unsupported dtype {x.dtype} (float32 required)")
    if x.dim() != 4:
        raise ValueError(f"{name}: [N,C,H,W] tensor required")
    if x.numel() == 0:
        raise ValueError(f"{name}: empty tensor")
    return x


def _size(size, name: str) -> Tuple[int, int]:
    oh, ow = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
    if oh < 1 or ow < 1:
        raise ValueError(f"{name}: output size must be positive")
    return oh, ow


@lru_cache(maxsize=None)
def _device_tables(in_size: int, out_size: int, device):
    """aa_tables on ``device``, kept for the life of the process (a few KiB per size pair), so no
    table is ever freed under a kernel that still reads it."""
    s, c, w = aa_tables(in_size, out_size)
    return (torch.from_numpy(s.copy()).to(device), torch.from_numpy(c.copy()).to(device),
            torch.from_numpy(w.copy()).to(device), int(w.shape[1]))


def resize_aa(x: torch.Tensor, size) -> torch.Tensor:
    """F.interpolate(x, size, mode="bilinear", align_corners=False, antialias=True) of a float32
    [N,C,H,W] device tensor (torchvision's Resize(antialias=True)); agrees with ATen on the host to
    about one float32 ulp of the data.  Equal sizes return ``x`` itself."""
    x = _nchw(x, "resize_aa")
    oh, ow = _size(size, "resize_aa")
    N, C, H, W = x.shape
    if (oh, ow) == (H, W):
        return x
    if H > MAX_RATIO * oh or W > MAX_RATIO * ow:
        raise ValueError(f"resize_aa: {H}x{W} -> {oh}x{ow}: in/out above {MAX_RATIO} is not supported")
    x = x.contiguous()
    xs = xc = xw = ys = yc = yw = None
    xt = yt = 0
    if W != ow:
        xs, xc, xw, xt = _device_tables(W, ow, x.device)
    if H != oh:
        ys, yc, yw, yt = _device_tables(H, oh, x.device)
    tmp = torch.empty(N, C, H, ow, dtype=torch.float32, device=x.device) if (W != ow and H != oh) else None
    out = torch.empty(N, C, oh, ow, dtype=torch.float32, device=x.device)
    lib.call("dcs_resize_aa", _p(x), _p(out), _p(tmp), N * C, H, W, oh, ow, _p(xs), _p(xc), _p(xw), xt,
             _p(ys), _p(yc), _p(yw), yt, _stream())
    return out


def resize_nearest(x: torch.Tensor, size) -> torch.Tensor:
    """F.interpolate(x, size, mode="nearest") of a float32 [N,C,H,W] device tensor, exactly.
    Equal sizes return ``x`` itself."""
    x = _nchw(x, "resize_nearest")
    oh, ow = _size(size, "resize_nearest")
    N, C, H, W = x.shape
    if (oh, ow) == (H, W):
        return x
    x = x.contiguous()
    out = torch.empty(N, C, oh, ow, dtype=torch.float32, device=x.device)
    lib.call("dcs_resize_nearest", _p(x), _p(out), N * C, H, W, oh, ow, _stream())
    return out


def translate_merge(raw: torch.Tensor, slope: torch.Tensor, intercept: torch.Tensor, y_soft: torch.Tensor,
                    y_lung: torch.Tensor, soft_range: Tuple[float, float], lung_range: Tuple[float, float],
                    unsigned: bool = False, want_soft: bool = False, want_lung: bool = False,
                    want_merged: bool = False, want_f32: bool = True):
    """modules/inference.py::stored_from_output of both Generators' outputs and ``synthesize`` on
    every slice, in one kernel.  raw: [D,H,W] stored values (int16 tensor; ``unsigned``: the bits
    are uint16); y_soft / y_lung: float32 [D,H,W] in [-1, 1]; slope / intercept: float32 [D].
    Returns (soft stored, lung stored, merged stored, merged as float32), None where not wanted.
    Values that do not fit the stored dtype are not pinned (numpy's cast is undefined there)."""
    for t, dt, name in ((raw, torch.int16, "raw"), (y_soft, torch.float32, "y_soft"),
                        (y_lung, torch.float32, "y_lung")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"translate_merge: {name}: device tensor required (no CPU fallback)")
        if t.dtype != dt:
            raise RuntimeError(f"translate_merge: {name}: unsupported dtype {t.dtype}")
    if raw.dim() != 3 or raw.numel() == 0:
        raise ValueError("translate_merge: [D,H,W] volume required")
    D, H, W = raw.shape
    if y_soft.numel() != raw.numel() or y_lung.numel() != raw.numel():
        raise ValueError("translate_merge: the model outputs differ in size from the raw series")
    if y_soft.device != raw.device or y_lung.device != raw.device:
        raise ValueError("translate_merge: operands on different devices")
    if not (want_soft or want_lung or want_merged or want_f32):
        raise ValueError("translate_merge: nothing to compute")
    raw, y_soft, y_lung = raw.contiguous(), y_soft.contiguous(), y_lung.contiguous()
    slope = slope.to(device=raw.device, dtype=torch.float32).reshape(-1).contiguous()
    intercept = intercept.to(device=raw.device, dtype=torch.float32).reshape(-1).contiguous()
    if slope.numel() != D or intercept.numel() != D:
        raise ValueError("translate_merge: one slope/intercept per slice")
    stored = lambda want: torch.empty_like(raw) if want else None
    so, lo, mo = stored(want_soft), stored(want_lung), stored(want_merged)
    mf = torch.empty(raw.shape, dtype=torch.float32, device=raw.device) if want_f32 else None
    f = lambda v: float(np.float32(v))
    (slo, shi), (llo, lhi) = soft_range, lung_range
    # hi - lo is formed before the float32 rounding, as stored_from_output's (hu_max - hu_min)
    lib.call("dcs_vol_translate_merge", _p(raw), lib.VOL_U16 if unsigned else lib.VOL_I16, _p(slope), _p(intercept),
             _p(y_soft), _p(y_lung), D, H, W, f(slo), f(shi), f(shi - slo), f(llo), f(lhi), f(lhi - llo),
             _p(so), _p(lo), _p(mo), _p(mf), _stream())
    return so, lo, mo, mf


def translate_enhance(raw: torch.Tensor, slope: torch.Tensor, intercept: torch.Tensor, y_soft: torch.Tensor,
                      y_lung: torch.Tensor, soft_range: Tuple[float, float], lung_range: Tuple[float, float],
                      threshold: float = 5.0, min_hu: float = -400.0, unsigned: bool = False,
                      want_stored: bool = False):
    """modules/inference.py::stored_from_output of both Generators' outputs and
    ``synthesize_enhancement`` of the resulting stored values on every slice, in one kernel.
    Operands as ``translate_merge``.  Returns (soft stored, lung stored, merged as float32); the two
    stored series are None without ``want_stored``."""
    for t, dt, name in ((raw, torch.int16, "raw"), (y_soft, torch.float32, "y_soft"),
                        (y_lung, torch.float32, "y_lung")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"translate_enhance: {name}: device tensor required (no CPU fallback)")
        if t.dtype != dt:
            raise RuntimeError(f"translate_enhance: {name}: unsupported dtype {t.dtype}")
    if raw.dim() != 3 or raw.numel() == 0:
        raise ValueError("translate_enhance: [D,H,W] volume required")
    D, H, W = raw.shape
    if y_soft.numel() != raw.numel() or y_lung.numel() != raw.numel():
        raise ValueError("translate_enhance: the model outputs differ in size from the raw series")
    if y_soft.device != raw.device or y_lung.device != raw.device:
        raise ValueError("translate_enhance: operands on different devices")
    raw, y_soft, y_lung = raw.contiguous(), y_soft.contiguous(), y_lung.contiguous()
    slope = slope.to(device=raw.device, dtype=torch.float32).reshape(-1).contiguous()
    intercept = intercept.to(device=raw.device, dtype=torch.float32).reshape(-1).contiguous()
    if slope.numel() != D or intercept.numel() != D:
        raise ValueError("translate_enhance: one slope/intercept per slice")
    so = torch.empty_like(raw) if want_stored else None
    lo = torch.empty_like(raw) if want_stored else None
    mf = torch.empty(raw.shape, dtype=torch.float32, device=raw.device)
    f = lambda v: float(np.float32(v))
    (slo, shi), (llo, lhi) = soft_range, lung_range
    # hi - lo is formed before the float32 rounding, as stored_from_output's (hu_max - hu_min)
    lib.call("dcs_vol_translate_enhance", _p(raw), lib.VOL_U16 if unsigned else lib.VOL_I16, _p(slope), _p(intercept),
             _p(y_soft), _p(y_lung), D, H, W, f(slo), f(shi - slo), f(llo), f(lhi - llo), f(threshold), f(min_hu),
             _p(so), _p(lo), _p(mf), _stream())
    return so, lo, mf
