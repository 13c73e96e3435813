"""modules/postprocess.py::postprocess_ct_volume on the MI355X (csrc/volume.hip).

Same keyword names, defaults and result as the host function, bit for bit: the kernels run
scipy's correlate1d and numpy's elementwise chain in the host's operation order and storage
dtypes (float32 between the axes of a float32 ``gaussian_filter``; float64 for 'adaptive',
'kalman' and the unsharp stage; axes with sigma <= 1e-15 skipped).  What the kernels do not
cover ('interpolation', a non-float32 volume, a Gaussian radius above 16, a median size that is
even or above 9) runs on the host implementation, see ``gpu_supported``.
"""
from __future__ import annotations

import numpy as np
import torch

from .postprocess import METHODS, postprocess_ct_volume

GPU_METHODS = ("gaussian", "gaussian3d", "adaptive", "median", "kalman")
UNSHARP_CHUNK_BYTES = 64 << 20   # float64 bytes per temporary of one unsharp slice chunk


def _radius(sigma):
    return int(4.0 * float(sigma) + 0.5)


def _sigma_ok(sigma, skippable):
    """A sigma the Gaussian kernel takes: radius <= 16; ``skippable`` axes (scipy's
    gaussian_filter) may also have sigma <= 1e-15, which scipy skips."""
    try:
        s = float(sigma)
    except (TypeError, ValueError):
        return False
    if not np.isfinite(s) or s < 0:
        return False
    if s <= 1e-15:
        return skippable
    return _radius(s) <= 16


def gpu_supported(method, dtype, **kwargs) -> bool:
    """True when postprocess_ct_volume_gpu runs (method, volume dtype, keyword arguments of
    postprocess_ct_volume, ``enhance_sharpness`` included) on the device kernels."""
    if method not in GPU_METHODS:
        return False
    try:
        if np.dtype(dtype) != np.float32:
            return False
    except TypeError:
        if dtype is not torch.float32:
            return False
    if method == "gaussian":
        ok = _sigma_ok(kwargs.get("sigma", 1.0), False)
    elif method == "gaussian3d":
        ok = _sigma_ok(kwargs.get("sigma_z", 2.0), True) and _sigma_ok(kwargs.get("sigma_xy", 0.5), True)
    elif method == "adaptive":
        ok = _sigma_ok(kwargs.get("base_sigma", 1.5), False) and _sigma_ok(kwargs.get("max_sigma", 3.0), True)
    elif method == "median":
        k = kwargs.get("kernel_size", 3)
        ok = isinstance(k, (int, np.integer)) and not isinstance(k, bool) and 1 <= k <= 9 and k % 2 == 1
    else:
        ok = True
    if ok and kwargs.get("enhance_sharpness", True):
        ok = _sigma_ok(kwargs.get("sharpen_radius", 1.0), False)
    return bool(ok)


def _gaussian_filter(x, sigmas, out_dtype=None):
    """scipy.ndimage.gaussian_filter(x, sigma=sigmas): the axes in order, skipping sigma <= 1e-15;
    None when no pass ran (the result is then x itself).  A radius-0 pass (sigma < 0.125: the
    one-tap kernel [1.0]) that keeps the dtype is skipped too, since x * 1.0 stored as x's dtype
    is x."""
    from .hip import volume as V
    cur = None
    for axis, s in enumerate(sigmas):
        src = x if cur is None else cur
        if float(s) <= 1e-15 or (V.gaussian_radius(s) == 0 and (out_dtype or src.dtype) == src.dtype):
            continue
        cur = V.gaussian_filter1d(src, s, axis, out_dtype=out_dtype)
    return cur


def _smooth(vol, method, kw):
    from .hip import volume as V
    if method == "gaussian":
        return V.gaussian_filter1d(vol, kw.get("sigma", 1.0), 0)
    if method == "gaussian3d":
        sxy = kw.get("sigma_xy", 0.5)
        out = _gaussian_filter(vol, (kw.get("sigma_z", 2.0), sxy, sxy))
        return vol if out is None else out
    if method == "adaptive":
        out = V.gaussian_filter1d(vol, kw.get("base_sigma", 1.5), 0, out_dtype=torch.float64)
        nxt = _gaussian_filter(out, (kw.get("max_sigma", 3.0), 0.3, 0.3))
        return out if nxt is None else nxt
    if method == "median":
        return V.median_filter_z(vol, kw.get("kernel_size", 3))
    return V.kalman_filter_z(vol, kw.get("process_variance", 1e-5), kw.get("measurement_variance", 1e-2))


def _blur_f64(x, radius):
    """gaussian_filter(x.astype(float64), sigma=(0, radius, radius)) of a slice chunk."""
    return _gaussian_filter(x, (0.0, radius, radius), out_dtype=torch.float64)


def postprocess_ct_volume_device(vol, method="gaussian3d", enhance_sharpness=True, hu_threshold=750, **kw):
    """The device part of postprocess_ct_volume_gpu: float32 [D,H,W] device tensor -> int16 device
    tensor, no transfer and no host fallback (an unsupported case raises ValueError)."""
    from .hip import volume as V
    if not (isinstance(vol, torch.Tensor) and vol.is_cuda and vol.dim() == 3 and vol.numel() > 0) or \
            not gpu_supported(method, vol.dtype, enhance_sharpness=enhance_sharpness, **kw):
        raise ValueError("postprocess_ct_volume_device: not a case the volume kernels cover (gpu_supported)")
    vol = vol.contiguous()
    sm = _smooth(vol, method, kw)
    if not enhance_sharpness:
        return V.finish(sm, vol, hu_threshold)
    amount, radius = kw.get("sharpen_amount", 0.5), kw.get("sharpen_radius", 1.0)
    mm = V.minmax(vol)
    D, H, W = vol.shape
    out = torch.empty(vol.shape, dtype=torch.int16, device=vol.device)
    # the unsharp stage has no z coupling: slice chunks keep its float64 temporaries small
    step = max(1, min(D, UNSHARP_CHUNK_BYTES // (H * W * 8)))
    for z0 in range(0, D, step):
        s, o = sm[z0:z0 + step], vol[z0:z0 + step]
        bs, bo = _blur_f64(s, radius), _blur_f64(o, radius)
        V.unsharp_finish(s, bs, bo, o, mm, amount, hu_threshold, out[z0:z0 + step])
    return out


def apply_diffmap_device(vol, diff, threshold=8):
    """modules/postprocess.py::apply_diffmap on the device for a caller that already holds a
    difference map: float32 device tensors of one shape -> a new float32 device tensor equal to
    ``vol + (diff with values below threshold zeroed).astype(uint8)``; ``diff`` is left unchanged
    (csrc/unet.hip).  No host fallback."""
    from .hip import unet as U
    with torch.cuda.device(vol.device):
        return U.apply_diffmap(vol, diff, threshold)


def postprocess_ct_volume_gpu(volume, method="gaussian3d", enhance_sharpness=True, hu_threshold=750, device="cuda",
                              **kwargs):
    """postprocess_ct_volume on ``device``: [slices, H, W] numpy array or device tensor -> int16
    numpy array, equal to the host function's.  Unsupported cases (gpu_supported) run there."""
    is_tensor = isinstance(volume, torch.Tensor)
    dtype = volume.dtype if is_tensor else np.asarray(volume).dtype
    ndim = volume.dim() if is_tensor else np.asarray(volume).ndim
    size = volume.numel() if is_tensor else np.asarray(volume).size
    plain_thr = isinstance(hu_threshold, (int, float)) and not isinstance(hu_threshold, bool)
    if method not in METHODS or ndim != 3 or size == 0 or not plain_thr or not gpu_supported(
            method, dtype, enhance_sharpness=enhance_sharpness, **kwargs):
        host = volume.detach().cpu().numpy() if is_tensor else volume
        return postprocess_ct_volume(host, method=method, enhance_sharpness=enhance_sharpness,
                                     hu_threshold=hu_threshold, **kwargs)
    dev = torch.device(device) if not (is_tensor and volume.is_cuda) else volume.device
    with torch.cuda.device(dev):
        vol = volume.to(dev) if is_tensor else torch.from_numpy(np.ascontiguousarray(volume)).to(dev)
        return postprocess_ct_volume_device(vol, method, bool(enhance_sharpness), hu_threshold,
                                            **kwargs).cpu().numpy()
