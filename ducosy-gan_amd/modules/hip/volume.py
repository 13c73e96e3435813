"""Device wrappers of the volume post-processing kernels (csrc/volume.hip, dcs_vol_*).

Every function takes and returns dense [D,H,W] device tensors.  Results are bit-identical to the
scipy / numpy calls named in each docstring (tests/test_gpu_postprocess.py).  No CPU fallback:
a host tensor or a bad argument raises.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import numpy as np
import torch

from . import lib
from .lib import ptr as _p, stream as _stream

MAX_RADIUS = lib.VOL_MAX_RADIUS
MAX_MEDIAN = lib.VOL_MAX_MEDIAN
_FDT = {torch.float32: lib.VOL_F32, torch.float64: lib.VOL_F64}


def _vol(t: torch.Tensor, name: str, dtypes) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name}: device tensor required (no CPU fallback)")
    if t.dtype not in dtypes:
        raise RuntimeError(f"{name}: unsupported dtype {t.dtype}")
    if t.dim() != 3:
        raise ValueError(f"{name}: [D,H,W] volume required")
    return t.contiguous()


def gaussian_radius(sigma: float, truncate: float = 4.0) -> int:
    """scipy.ndimage.gaussian_filter1d's kernel radius."""
    return int(truncate * float(sigma) + 0.5)


def gaussian_weights(sigma: float, radius: Optional[int] = None) -> np.ndarray:
    """The 2r+1 normalised weights of scipy.ndimage.gaussian_filter1d (order 0), by the same
    numpy expression (scipy/ndimage/_filters.py::_gaussian_kernel1d), so bit-identical."""
    sigma = float(sigma)
    r = gaussian_radius(sigma) if radius is None else int(radius)
    sigma2 = sigma * sigma
    x = np.arange(-r, r + 1)
    phi_x = np.exp(-0.5 / sigma2 * x ** 2)
    return phi_x / phi_x.sum()


def gaussian_filter1d(x: torch.Tensor, sigma: float, axis: int, out_dtype: Optional[torch.dtype] = None,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """scipy.ndimage.gaussian_filter1d(x, sigma, axis, mode='reflect') of a float32 / float64
    volume.  out_dtype=torch.float64 on a float32 input filters x.astype(float64)."""
    x = _vol(x, "gaussian_filter1d", _FDT)
    out_dtype = out_dtype or x.dtype
    if out_dtype not in _FDT:
        raise RuntimeError(f"gaussian_filter1d: unsupported output dtype {out_dtype}")
    if axis < 0:
        axis += 3
    w = np.ascontiguousarray(gaussian_weights(sigma), dtype=np.float64)
    r = (w.size - 1) // 2
    if out is None:
        out = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    elif out.shape != x.shape or out.dtype != out_dtype or not out.is_contiguous() or out.device != x.device:
        raise ValueError("gaussian_filter1d: out must be a contiguous tensor of the result's shape and dtype")
    D, H, W = x.shape
    lib.call("dcs_vol_gauss1d", _p(x), _FDT[x.dtype], _p(out), _FDT[out_dtype], D, H, W, int(axis), r,
             w.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), _stream())
    return out


def median_filter_z(x: torch.Tensor, kernel_size: int) -> torch.Tensor:
    """scipy.ndimage.median_filter(x, size=(kernel_size, 1, 1)) of a float32 volume."""
    x = _vol(x, "median_filter_z", (torch.float32,))
    out = torch.empty_like(x)
    D, H, W = x.shape
    lib.call("dcs_vol_median_z", _p(x), _p(out), D, H, W, int(kernel_size), _stream())
    return out


def kalman_gains(n: int, process_variance: float, measurement_variance: float) -> np.ndarray:
    """The gain sequence of modules/postprocess.py::_kalman_columns (initial covariance 1)."""
    g = np.empty(n, np.float64)
    p = 1.0
    for k in range(n):
        pp = p + process_variance
        g[k] = pp / (pp + measurement_variance)
        p = (1 - g[k]) * pp
    return g


def kalman_filter_z(x: torch.Tensor, process_variance: float, measurement_variance: float) -> torch.Tensor:
    """modules/postprocess.py::apply_kalman_filter of a float32 volume -> float64."""
    x = _vol(x, "kalman_filter_z", (torch.float32,))
    D, H, W = x.shape
    gain = torch.from_numpy(kalman_gains(D, process_variance, measurement_variance)).to(x.device)
    out = torch.empty(x.shape, dtype=torch.float64, device=x.device)
    lib.call("dcs_vol_kalman_z", _p(x), _p(gain), _p(out), D, H, W, _stream())
    return out


def minmax(x: torch.Tensor) -> torch.Tensor:
    """float32 [2] device tensor: (x.min(), x.max()) of a float32 tensor of finite values."""
    if not x.is_cuda or x.dtype != torch.float32:
        raise RuntimeError("minmax: float32 device tensor required")
    x = x.contiguous()
    out = torch.empty(2, dtype=torch.float32, device=x.device)
    ws = torch.empty(2 * lib.VOL_MINMAX_PARTS, dtype=torch.float32, device=x.device)
    lib.call("dcs_vol_minmax", _p(x), x.numel(), _p(out), _p(ws), _stream())
    return out


def unsharp_finish(sm: torch.Tensor, blur_sm: torch.Tensor, blur_og: torch.Tensor, original: torch.Tensor,
                   mm: torch.Tensor, amount: float, hu_threshold: float, out: torch.Tensor) -> torch.Tensor:
    """postprocess.unsharp_mask given the two in-plane blurs, then ``out[keep] = original[keep]``
    and astype(int16), on any number of whole slices.  mm: minmax(original volume)."""
    n = sm.numel()
    for t, dt in ((blur_sm, torch.float64), (blur_og, torch.float64), (original, torch.float32),
                  (out, torch.int16)):
        if not t.is_cuda or t.dtype != dt or t.numel() != n or not t.is_contiguous():
            raise ValueError("unsharp_finish: operands must be contiguous device tensors of one size")
    if not sm.is_cuda or sm.dtype not in _FDT or not sm.is_contiguous():
        raise ValueError("unsharp_finish: sm must be a contiguous float32 / float64 device tensor")
    amount = float(amount)
    lib.call("dcs_vol_unsharp_finish", _p(sm), _FDT[sm.dtype], _p(blur_sm), _p(blur_og), _p(original), _p(mm), n,
             1 - amount, amount, float(np.float32(hu_threshold)), _p(out), _stream())
    return out


def finish(sm: torch.Tensor, original: torch.Tensor, hu_threshold: float) -> torch.Tensor:
    """``sm[original >= hu_threshold] = original[...]`` and astype(int16)."""
    sm = _vol(sm, "finish", _FDT)
    original = _vol(original, "finish", (torch.float32,))
    if original.shape != sm.shape:
        raise ValueError("finish: shapes differ")
    out = torch.empty(sm.shape, dtype=torch.int16, device=sm.device)
    lib.call("dcs_vol_finish", _p(sm), _FDT[sm.dtype], _p(original), sm.numel(), float(np.float32(hu_threshold)),
             _p(out), _stream())
    return out


def merge_hu_ranges(raw: torch.Tensor, soft: torch.Tensor, lung: torch.Tensor, slope: torch.Tensor,
                    intercept: torch.Tensor, soft_range: Tuple[float, float], lung_range: Tuple[float, float],
                    unsigned: bool = False, want_stored: bool = True, want_f32: bool = False):
    """modules/inference.py::synthesize on every slice of three stored-value volumes (int16
    tensors; ``unsigned``: the bits are uint16).  slope / intercept: float32 [D] device tensors.
    Returns (merged stored values or None, merged values as float32 or None)."""
    raw = _vol(raw, "merge_hu_ranges", (torch.int16,))
    soft = _vol(soft, "merge_hu_ranges", (torch.int16,))
    lung = _vol(lung, "merge_hu_ranges", (torch.int16,))
    D, H, W = raw.shape
    if soft.shape != raw.shape or lung.shape != raw.shape:
        raise ValueError("merge_hu_ranges: the three series differ in shape")
    slope = slope.to(device=raw.device, dtype=torch.float32).reshape(-1).contiguous()
    intercept = intercept.to(device=raw.device, dtype=torch.float32).reshape(-1).contiguous()
    if slope.numel() != D or intercept.numel() != D:
        raise ValueError("merge_hu_ranges: one slope/intercept per slice")
    if not (want_stored or want_f32):
        raise ValueError("merge_hu_ranges: nothing to compute")
    out = torch.empty_like(raw) if want_stored else None
    f32 = torch.empty(raw.shape, dtype=torch.float32, device=raw.device) if want_f32 else None
    f = lambda v: float(np.float32(v))
    lib.call("dcs_vol_merge", _p(raw), _p(soft), _p(lung), lib.VOL_U16 if unsigned else lib.VOL_I16, _p(slope),
             _p(intercept), D, H, W, f(soft_range[0]), f(soft_range[1]), f(lung_range[0]), f(lung_range[1]),
             _p(out), _p(f32), _stream())
    return out, f32


def merge_enhancement(raw: torch.Tensor, soft: torch.Tensor, lung: torch.Tensor, slope: torch.Tensor,
                      intercept: torch.Tensor, threshold: float = 5.0, min_hu: float = -400.0,
                      unsigned: bool = False) -> torch.Tensor:
    """modules/inference.py::synthesize_enhancement on every slice of three stored-value volumes
    (int16 tensors; ``unsigned``: the bits are uint16), all three read with the NCCT's rescale pair.
    slope / intercept: float32 [D] device tensors.  Returns the merged values as float32."""
    raw = _vol(raw, "merge_enhancement", (torch.int16,))
    soft = _vol(soft, "merge_enhancement", (torch.int16,))
    lung = _vol(lung, "merge_enhancement", (torch.int16,))
    D, H, W = raw.shape
    if soft.shape != raw.shape or lung.shape != raw.shape:
        raise ValueError("merge_enhancement: the three series differ in shape")
    if soft.device != raw.device or lung.device != raw.device:
        raise ValueError("merge_enhancement: operands on different devices")
    if raw.numel() == 0:
        raise ValueError("merge_enhancement: empty volume")
    slope = slope.to(device=raw.device, dtype=torch.float32).reshape(-1).contiguous()
    intercept = intercept.to(device=raw.device, dtype=torch.float32).reshape(-1).contiguous()
    if slope.numel() != D or intercept.numel() != D:
        raise ValueError("merge_enhancement: one slope/intercept per slice")
    out = torch.empty(raw.shape, dtype=torch.float32, device=raw.device)
    f = lambda v: float(np.float32(v))
    lib.call("dcs_vol_merge_enhance", _p(raw), _p(soft), _p(lung), lib.VOL_U16 if unsigned else lib.VOL_I16,
             _p(slope), _p(intercept), D, H, W, f(threshold), f(min_hu), _p(out), _stream())
    return out
