"""Device wrappers of the evaluation-metric kernels (csrc/metrics.hip, dcs_met_*).

Every function takes float32 [D,H,W] device tensors and returns float64 device tensors with one
row per slice (tests/test_gpu_metrics.py compares them with modules/metrics.py).  No CPU
fallback: a host tensor, another dtype or mismatched shapes raise before anything is launched.
``affine`` is ``(a_off, a_div, b_off, b_div)``: the kernels read ``(x - off) / div`` in float32
(0 where div is 0) in place of x; None reads the volumes as they are.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import torch

from . import lib
from .lib import ptr as _p, stream as _stream

NSTATS = lib.MET_NSTATS
TILE_X, TILE_Y = lib.MET_TILE_X, lib.MET_TILE_Y
# columns of pair_stats
SUM_ABS, SUM_SQ, SUM_AB, SUM_AA, SUM_BB, MIN_A, MAX_A, MIN_B, MAX_B = range(9)


def _vol(t, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name}: device tensor required (no CPU fallback)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name}: float32 required, got {t.dtype}")
    if t.dim() != 3 or t.numel() == 0:
        raise ValueError(f"{name}: non-empty [D,H,W] volume required")
    return t.contiguous()


def _pair(a, b, name: str):
    a, b = _vol(a, name), _vol(b, name)
    if a.shape != b.shape or a.device != b.device:
        raise ValueError(f"{name}: the two volumes differ in shape or device")
    return a, b


def _affine(affine: Optional[Sequence[float]]):
    if affine is None:
        return None
    if len(affine) != 4:
        raise ValueError("affine: (a_off, a_div, b_off, b_div)")
    return (ctypes.c_float * 4)(*[float(v) for v in affine])


def _workspace(a: torch.Tensor):
    D, H, W = a.shape
    n = lib.query("dcs_met_workspace_size", D, H, W)
    if n == 0:
        raise ValueError(f"metrics: unsupported volume shape {tuple(a.shape)}")
    return torch.empty(n // 8, dtype=torch.float64, device=a.device), n


def pair_stats(a: torch.Tensor, b: torch.Tensor, affine=None) -> torch.Tensor:
    """float64 [D,9]: sum|a-b|, sum (a-b)^2 (float32 squares), sum ab, sum a^2, sum b^2, min a,
    max a, min b, max b of every slice, from one pass over both volumes."""
    a, b = _pair(a, b, "pair_stats")
    D, H, W = a.shape
    ws, n = _workspace(a)
    out = torch.empty((D, NSTATS), dtype=torch.float64, device=a.device)
    lib.call("dcs_met_pair_stats", _p(a), _p(b), D, H, W, _affine(affine), _p(out), _p(ws), n, _stream())
    return out


def ssim_sums(a: torch.Tensor, b: torch.Tensor, data_range: float, affine=None) -> torch.Tensor:
    """float64 [D]: the sum of the SSIM map over the interior of every slice (the mean divides by
    (H-6)(W-6))."""
    a, b = _pair(a, b, "ssim")
    D, H, W = a.shape
    if H < 7 or W < 7:
        raise ValueError("ssim: win_size exceeds image extent: both sides of a slice must be at least 7")
    ws, n = _workspace(a)
    out = torch.empty(D, dtype=torch.float64, device=a.device)
    lib.call("dcs_met_ssim", _p(a), _p(b), D, H, W, _affine(affine), float(data_range), _p(out), _p(ws), n, _stream())
    return out


def sobel_ts(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """float64 [D,3]: sum|g1-g2|, max g1, max g2 of the Sobel magnitudes of every slice."""
    a, b = _pair(a, b, "sobel_ts")
    D, H, W = a.shape
    ws, n = _workspace(a)
    out = torch.empty((D, 3), dtype=torch.float64, device=a.device)
    lib.call("dcs_met_sobel_ts", _p(a), _p(b), D, H, W, _p(out), _p(ws), n, _stream())
    return out


def ed_sums(a: torch.Tensor, b: torch.Tensor, stats: torch.Tensor) -> torch.Tensor:
    """float64 [D]: sum (a_n - b_n)^2 with every slice normalised by its own min / max;
    stats: pair_stats(a, b) without affine."""
    a, b = _pair(a, b, "ed")
    D, H, W = a.shape
    if (not isinstance(stats, torch.Tensor) or stats.device != a.device or stats.dtype != torch.float64
            or tuple(stats.shape) != (D, NSTATS) or not stats.is_contiguous()):
        raise ValueError("ed: stats must be the contiguous float64 [D,9] result of pair_stats on this pair")
    ws, n = _workspace(a)
    out = torch.empty(D, dtype=torch.float64, device=a.device)
    lib.call("dcs_met_ed", _p(a), _p(b), D, H, W, _p(stats), _p(out), _p(ws), n, _stream())
    return out


def sorted_l1(a: torch.Tensor, b: torch.Tensor, affine=None) -> torch.Tensor:
    """float64 [D]: sum|a_n - b_n| of two volumes whose slices are sorted."""
    a, b = _pair(a, b, "sorted_l1")
    D, H, W = a.shape
    ws, n = _workspace(a)
    out = torch.empty(D, dtype=torch.float64, device=a.device)
    lib.call("dcs_met_sorted_l1", _p(a), _p(b), D, H, W, _affine(affine), _p(out), _p(ws), n, _stream())
    return out


def msssim_level_sums(a: torch.Tensor, b: torch.Tensor, window: Sequence[float], c1: float, c2: float) -> torch.Tensor:
    """float64 [D,2]: the sums of the SSIM map and of its contrast-structure factor over the
    (H-10) x (W-10) windows inside every slice of one MS-SSIM level (the means divide by that
    count).  window: the eleven float64 taps of the separable filter."""
    a, b = _pair(a, b, "msssim_level")
    D, H, W = a.shape
    if len(window) != lib.MET_MSSSIM_TAPS:
        raise ValueError(f"msssim_level: a window of {lib.MET_MSSSIM_TAPS} taps is required")
    if H < lib.MET_MSSSIM_TAPS or W < lib.MET_MSSSIM_TAPS:
        raise ValueError("msssim_level: the 11x11 window exceeds the image")
    ws, n = _workspace(a)
    out = torch.empty((D, 2), dtype=torch.float64, device=a.device)
    win = (ctypes.c_double * lib.MET_MSSSIM_TAPS)(*[float(v) for v in window])
    lib.call("dcs_met_msssim_level", _p(a), _p(b), D, H, W, win, float(c1), float(c2), _p(out), _p(ws), n, _stream())
    return out


def pool2(a: torch.Tensor, b: torch.Tensor):
    """The 2x2 averages of both volumes, float32 [D,H//2,W//2] each (the sum of four in float64)."""
    a, b = _pair(a, b, "pool2")
    D, H, W = a.shape
    if H < 2 or W < 2:
        raise ValueError("pool2: both sides of a slice must be at least 2")
    oa = torch.empty((D, H // 2, W // 2), dtype=torch.float32, device=a.device)
    ob = torch.empty_like(oa)
    lib.call("dcs_met_pool2", _p(a), _p(b), _p(oa), _p(ob), D, H, W, _stream())
    return oa, ob


def _region_vols(name: str, *vols):
    """The float32 series of a region call: device, dtype, shape and contiguity are checked and
    nothing is copied, so the kernels read what the caller holds; every fault is a ValueError."""
    for t in vols:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"{name}: device tensor required (no CPU fallback)")
        if t.dtype != torch.float32:
            raise ValueError(f"{name}: float32 required, got {t.dtype}")
        if t.dim() != 3 or t.numel() == 0:
            raise ValueError(f"{name}: non-empty [D,H,W] volume required")
        if t.shape != vols[0].shape or t.device != vols[0].device:
            raise ValueError(f"{name}: the volumes differ in shape or device")
        if not t.is_contiguous():
            raise ValueError(f"{name}: contiguous volumes required")
    return vols


def _region_workspace(a: torch.Tensor):
    D, H, W = a.shape
    n = lib.query("dcs_met_region_workspace_size", D, H, W)
    if n == 0:
        raise ValueError(f"metrics: unsupported volume shape {tuple(a.shape)}")
    return torch.empty(n // 8, dtype=torch.float64, device=a.device), n


def region_sums(vue: torch.Tensor, std: torch.Tensor, gen: torch.Tensor, ranges: Sequence[float], with_map: bool = True):
    """(float64 [D,21], uint8 [D,H,W] or None): modules/metrics.py::region_sums of every slice from
    one pass over the three series, and the region byte of every voxel (owner 0 lung, 1 soft,
    2 rest, | 4 inside the true enhancement) that region_ssim_sums reads.  ranges: (lung_min,
    lung_max, soft_min, soft_max, thr, min_hu)."""
    vue, std, gen = _region_vols("region_sums", vue, std, gen)
    if len(ranges) != 6:
        raise ValueError("region_sums: ranges is (lung_min, lung_max, soft_min, soft_max, thr, min_hu)")
    D, H, W = std.shape
    ws, n = _region_workspace(std)
    out = torch.empty((D, lib.MET_REGION_NSUMS), dtype=torch.float64, device=std.device)
    rmap = torch.empty((D, H, W), dtype=torch.uint8, device=std.device) if with_map else None
    rng = (ctypes.c_float * 6)(*[float(v) for v in ranges])
    lib.call("dcs_met_region_sums", _p(vue), _p(std), _p(gen), D, H, W, rng, _p(out), _p(rmap), _p(ws), n, _stream())
    return out, rmap


def region_ssim_sums(std: torch.Tensor, gen: torch.Tensor, region_map: torch.Tensor, data_range: float) -> torch.Tensor:
    """float64 [D,8]: per region (lung, soft, rest, true enhancement) the number of its pixels in
    the interior cropped by 3 and the sum over them of the map ssim_sums adds up; region_map is
    region_sums' second result for the same series."""
    std, gen = _region_vols("region_ssim", std, gen)
    D, H, W = std.shape
    if H < 7 or W < 7:
        raise ValueError("region_ssim: win_size exceeds image extent: both sides of a slice must be at least 7")
    if (not isinstance(region_map, torch.Tensor) or region_map.device != std.device or region_map.dtype != torch.uint8
            or region_map.shape != std.shape or not region_map.is_contiguous()):
        raise ValueError("region_ssim: region_map must be the contiguous uint8 [D,H,W] result of region_sums")
    ws, n = _region_workspace(std)
    out = torch.empty((D, lib.MET_REGION_NSSIM), dtype=torch.float64, device=std.device)
    lib.call("dcs_met_region_ssim", _p(std), _p(gen), _p(region_map), D, H, W, float(data_range), _p(out), _p(ws), n,
             _stream())
    return out


def normalize(x: torch.Tensor, off: float, div: float) -> torch.Tensor:
    """(x - off) / div in float32, zeros where div is 0."""
    x = _vol(x, "normalize")
    out = torch.empty_like(x)
    lib.call("dcs_met_normalize", _p(x), x.numel(), float(off), float(div), _p(out), _stream())
    return out
