"""Inference with the normal-map U-Net: the reference's modules/nmodel/inference.py (load_model,
predict_volume) with the forward on the MI355X kernels (modules/hip/unet.py).

The reference normalises the HU volume, runs the model on one [1,1,1,H,W] slice at a time and
denormalises the output to difference-map units.  Here the slices go through the folded 2-D form
of the model in chunks, on the device; every layer is per-slice, so the chunk size changes the
throughput and nothing else.  Training the U-Net and the reference's PNG writers are not part of
this module.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch

from .model import UNet3D, UNet3DLight

HU_MIN, HU_MAX = -1024, 3071   # normalize_hu's range
DIFF_MAX = 4000                # denormalize_diff's range [0, DIFF_MAX]


def normalize_hu(volume: np.ndarray) -> np.ndarray:
    """HU -> [-1, 1] in float32: clip to [-1024, 3071], (v + 1024) / 4095, then * 2 - 1, one float32
    rounding per step (csrc/unet.hip runs the same chain)."""
    v = np.clip(np.asarray(volume, dtype=np.float32), np.float32(HU_MIN), np.float32(HU_MAX))
    v = (v - np.float32(HU_MIN)) / np.float32(HU_MAX - HU_MIN)
    return v * np.float32(2) - np.float32(1)


def denormalize_diff(y: np.ndarray) -> np.ndarray:
    """Model output in [-1, 1] -> difference-map units [0, 4000] in float32: (y + 1) / 2 * 4000."""
    y = np.asarray(y, dtype=np.float32)
    return (y + np.float32(1)) / np.float32(2) * np.float32(DIFF_MAX)


def diffmap_tail(volume: np.ndarray, y: np.ndarray, threshold=8) -> np.ndarray:
    """The host form of the device tail: denormalize_diff, then modules/postprocess.py::apply_diffmap
    on a float32 volume."""
    from ..postprocess import apply_diffmap
    return apply_diffmap(np.asarray(volume, dtype=np.float32), denormalize_diff(y), threshold)


def load_model(checkpoint_path, device="cuda"):
    """The reference's rules: the checkpoint is a dict with 'model_state_dict'; keys that name
    'down4' select UNet3D, else UNet3DLight; base / input / output channels come from
    checkpoint['config'] (defaults 16, 1, 1) or, without it, from the first convolution's shape with
    one output channel.  Returns (model in eval mode on ``device``, config) where config carries
    base_channels, in_channels and out_channels.  Read with weights_only=True."""
    ckpt = torch.load(checkpoint_path, map_location="cpu", weights_only=True)
    if not isinstance(ckpt, dict) or "model_state_dict" not in ckpt:
        raise ValueError(f"{checkpoint_path}: a checkpoint dict with 'model_state_dict' expected")
    sd = ckpt["model_state_dict"]
    cls = UNet3D if any("down4" in k for k in sd) else UNet3DLight
    cfg = ckpt.get("config")
    if cfg is not None:
        get = cfg.get if isinstance(cfg, dict) else (lambda k, d: getattr(cfg, k, d))
        base, cin, cout = get("base_channels", 16), get("in_channels", 1), get("out_channels", 1)
    else:
        first = sd["inc.double_conv.0.weight"]
        base, cin, cout = first.shape[0], first.shape[1], 1
    model = cls(n_channels=int(cin), n_classes=int(cout), base_channels=int(base))
    # BatchNorm's step counter plays no part in eval mode: a checkpoint may carry it or not
    bad = model.load_state_dict(sd, strict=False)
    wrong = [k for k in list(bad.missing_keys) + list(bad.unexpected_keys) if not k.endswith("num_batches_tracked")]
    if wrong:
        raise RuntimeError(f"{checkpoint_path}: state_dict keys do not match {cls.__name__}: {wrong[:8]}")
    model = model.to(device).eval()
    return model, SimpleNamespace(base_channels=int(base), in_channels=int(cin), out_channels=int(cout))


def _device_volume(hu, name):
    if not isinstance(hu, torch.Tensor) or not hu.is_cuda:
        raise RuntimeError(f"{name}: device tensor required (no CPU fallback)")
    if hu.dtype != torch.float32 or hu.dim() != 3 or hu.numel() == 0:
        raise ValueError(f"{name}: a non-empty float32 [D,H,W] HU volume required")
    return hu.contiguous()


@torch.no_grad()
def _run(model, hu, merged, threshold, want_diff, chunk):
    from ..hip import unet as U
    with torch.cuda.device(hu.device):
        plan = U.plan_for(model, hu.device)
        D, H, W = hu.shape
        step = U.default_chunk(plan, D, H, W) if chunk is None else int(chunk)
        if step < 1:
            raise ValueError("chunk must be positive")
        diff = torch.empty_like(hu) if want_diff else None
        for z in range(0, D, step):
            with U.timed(f"normalize_hu @{H}x{W}"):
                x4 = U.normalize_hu(hu[z:z + step], pad4=True)
            y, last = U.forward(plan, x4)
            with U.timed(f"output {y.shape[3]}->1 @{H}x{W}"):
                d = U.out_diffmap(y, last.scale, last.shift, plan.out_weight, plan.out_bias, threshold,
                                  volume=None if merged is None else merged[z:z + step], want_diff=want_diff)
            if want_diff:
                diff[z:z + step] = d
    return diff


def predict_volume_device(model, hu: torch.Tensor, chunk: Optional[int] = None) -> torch.Tensor:
    """[D,H,W] float32 HU on the device -> [D,H,W] float32 difference map on the device, no host
    round trip.  ``chunk``: slices per call (default: by activation size)."""
    return _run(model, _device_volume(hu, "predict_volume_device"), None, 8, True, chunk)


def apply_predicted_diffmap_device(model, hu: torch.Tensor, merged: torch.Tensor, threshold=8,
                                   want_diff: bool = False, chunk: Optional[int] = None):
    """predict_volume_device + apply_diffmap fused: the thresholded uint8 difference map of ``hu`` is
    added INTO ``merged`` (float32 [D,H,W] device tensor) by the output kernel; the float map is
    written and returned only with ``want_diff``."""
    hu = _device_volume(hu, "apply_predicted_diffmap_device")
    if not isinstance(merged, torch.Tensor) or not merged.is_cuda or merged.dtype != torch.float32 or \
            merged.shape != hu.shape or not merged.is_contiguous():
        raise ValueError("apply_predicted_diffmap_device: merged must be a contiguous float32 device tensor of hu's shape")
    return _run(model, hu, merged, threshold, want_diff, chunk)


def predict_volume(model, hu_volume, device="cuda", use_amp=True) -> np.ndarray:
    """Drop-in for the reference's predict_volume: [D,H,W] HU on the host -> [D,H,W] float32 in
    difference-map units on the host: predict_volume_device plus one upload and one download.
    ``use_amp`` is accepted for compatibility; the precision is the operand mode of
    modules/hip/ops.py."""
    del use_amp
    hu = torch.from_numpy(np.ascontiguousarray(hu_volume, dtype=np.float32)).to(torch.device(device))
    return predict_volume_device(model, hu).cpu().numpy()
