"""Device wrappers of csrc/organ_masks.hip: the heart-mask clean-up, the organ mask and the apply
pass of modules/organ_masks.py on resident volumes, plus the 3-D labelling they are built on.

Conventions of modules/hip/slices.py: device tensors only (no CPU fallback), a bad argument raises
before anything is launched, the kernels go to the current stream, ``with torch.cuda.device(...)``
is left to the caller.  Volumes are uint8 [z, y, x] (``modules.nifti``'s ``labels_zyx`` view).
"""
from __future__ import annotations

import ctypes

import torch

from . import lib
from .lib import ptr as _p, stream as _stream
from .. import organ_masks as host

# bytes of (slice, label) images a chunk of the organ mask may hold (5 bytes per pixel)
CHUNK_BYTES = 256 << 20


def _labels(t, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name}: device tensor required (no CPU fallback)")
    if t.dtype != torch.uint8:
        raise RuntimeError(f"{name}: uint8 labels required (labels must be < 256), got {t.dtype}")
    if t.dim() != 3 or t.numel() == 0:
        raise ValueError(f"{name}: non-empty [z, y, x] volume required")
    if t.numel() >= 1 << 31:
        raise ValueError(f"{name}: volume too large ({t.numel()} voxels; z*y*x < 2^31)")
    return t.contiguous()


def _label_value(v, name: str) -> int:
    v = int(v)
    if not 0 <= v < 256:
        raise ValueError(f"{name}: label {v}: labels must be < 256")
    return v


def label3d(volume: torch.Tensor, match: int = 1):
    """6-connected components of ``volume == match`` (uint8 [z, y, x] on the device).  Returns
    (labels int32 [z, y, x]: the smallest voxel index of the component, -1 for background; count
    int32, sums int64 [3, z*y*x] (x, y, z coordinate sums), keys int64: the last three are valid at
    the roots, the voxels i with labels.view(-1)[i] == i)."""
    volume = _labels(volume, "label3d")
    match = _label_value(match, "label3d")
    D, H, W = volume.shape
    n = volume.numel()
    dev = volume.device
    labels = torch.empty((D, H, W), dtype=torch.int32, device=dev)
    count = torch.empty(n, dtype=torch.int32, device=dev)
    sums = torch.empty((3, n), dtype=torch.int64, device=dev)
    keys = torch.empty(n, dtype=torch.int32, device=dev)
    lib.call("dcs_cc3_label", _p(volume), match, D, H, W, _p(labels), _p(count), _p(sums), _p(keys), _stream())
    return labels, count, sums, keys.to(torch.int64) & 0xFFFFFFFF


def heart_workspace_size(shape) -> int:
    D, H, W = (int(s) for s in shape)
    return lib.query("dcs_heart_workspace_size", D, H, W)


def modify_heart_label(labels_zyx: torch.Tensor, *, heart_label: int = host.HEART_LABEL, gap_threshold: int = 2,
                       offset: float = 1.15, offset_y_base: float = 1.4, offset_z: float = 2.65,
                       min_region: int = 1024, workspace: torch.Tensor = None) -> torch.Tensor:
    """``modules.organ_masks.modify_heart_label`` on a resident uint8 [z, y, x] volume (the host
    function's [x, y, z] argument transposed); returns the modified volume in the same layout,
    equal to the host's bit for bit.  Nothing is read back: the choice of the lowest component is
    made on the device."""
    vol = _labels(labels_zyx, "modify_heart_label")
    heart_label = _label_value(heart_label, "modify_heart_label")
    if gap_threshold < 1:
        raise ValueError("modify_heart_label: gap_threshold must be >= 1")
    D, H, W = vol.shape
    nbytes = heart_workspace_size(vol.shape)
    if nbytes == 0:
        raise ValueError(f"modify_heart_label: unsupported volume shape {(D, H, W)}")
    ws = _workspace(workspace, nbytes, vol.device, "modify_heart_label")
    out = torch.empty_like(vol)
    lib.call("dcs_heart_modify", _p(vol), D, H, W, heart_label, int(gap_threshold), float(offset),
             float(offset_y_base - 1), float(offset_z), int(min_region), _p(out), _p(ws), ws.numel() * ws.element_size(),
             _stream())
    return out


def _workspace(ws, nbytes: int, device, name: str) -> torch.Tensor:
    if ws is None:
        return torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=device)
    if not isinstance(ws, torch.Tensor) or not ws.is_cuda or not ws.is_contiguous():
        raise RuntimeError(f"{name}: workspace: contiguous device tensor required")
    if ws.numel() * ws.element_size() < nbytes:
        raise ValueError(f"{name}: workspace too small ({ws.numel() * ws.element_size()} < {nbytes} bytes)")
    return ws


def _brush(table):
    offs = host.brush_offsets(table)
    if not 1 <= len(offs) <= 25 or any(max(abs(dy), abs(dx)) > 2 for dy, dx in offs):
        raise ValueError("organ_mask: brush: 1..25 offsets within radius 2")
    flat = [v for pair in offs for v in pair]
    return (ctypes.c_int8 * len(flat))(*flat), len(offs)


def default_chunk(shape, nlabels: int) -> int:
    """Slices per chunk so that the (slice, label) images stay within CHUNK_BYTES."""
    N, H, W = (int(s) for s in shape)
    per_slice = 5 * nlabels * (H * W + 4096)
    return max(1, min(N, CHUNK_BYTES // per_slice, 65535 // nlabels))


def organ_mask_workspace_size(shape, nlabels: int, chunk: int) -> int:
    N, H, W = (int(s) for s in shape)
    return lib.query("dcs_organ_mask_workspace_size", N, H, W, int(nlabels), int(chunk))


def organ_mask(labels_zyx: torch.Tensor, target_labels=host.MASK_TARGET_LABELS, *, chunk: int = None,
               workspace: torch.Tensor = None) -> torch.Tensor:
    """``modules.organ_masks.organ_mask`` on a resident uint8 [z, y, x] volume; returns the uint8
    0/1 mask, equal to the host's bit for bit.  ``chunk`` slices are in flight at a time (default:
    what keeps the workspace near CHUNK_BYTES)."""
    vol = _labels(labels_zyx, "organ_mask")
    targets = [_label_value(v, "organ_mask") for v in target_labels]
    if not 1 <= len(targets) <= 255:
        raise ValueError("organ_mask: 1..255 target labels required")
    N, H, W = vol.shape
    chunk = default_chunk(vol.shape, len(targets)) if chunk is None else int(chunk)
    nbytes = organ_mask_workspace_size(vol.shape, len(targets), chunk) if chunk >= 1 else 0
    if nbytes == 0:
        raise ValueError(f"organ_mask: unsupported shape {(N, H, W)} with {len(targets)} labels in chunks of {chunk}")
    ws = _workspace(workspace, nbytes, vol.device, "organ_mask")
    b1, n1 = _brush(host.BRUSH_2)
    b2, n2 = _brush(host.BRUSH_4)
    out = torch.empty_like(vol)
    tl = (ctypes.c_int32 * len(targets))(*targets)
    lib.call("dcs_organ_mask", _p(vol), N, H, W, tl, len(targets), b1, n1, b2, n2, chunk, _p(out), _p(ws),
             ws.numel() * ws.element_size(), _stream())
    return out


def apply_organ_mask(ncct: torch.Tensor, cect: torch.Tensor, scect: torch.Tensor, mask: torch.Tensor,
                     fill: int = host.MASK_FILL):
    """``modules.organ_masks.apply_organ_mask`` of three int16 series in one pass; returns the
    three masked copies."""
    series = []
    for name, t in (("ncct", ncct), ("cect", cect), ("scect", scect)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"apply_organ_mask: {name}: device tensor required (no CPU fallback)")
        if t.dtype != torch.int16:
            raise RuntimeError(f"apply_organ_mask: {name}: int16 required, got {t.dtype}")
        series.append(t.contiguous())
    if not isinstance(mask, torch.Tensor) or not mask.is_cuda:
        raise RuntimeError("apply_organ_mask: mask: device tensor required (no CPU fallback)")
    if mask.dtype != torch.uint8:
        raise RuntimeError(f"apply_organ_mask: mask: uint8 required, got {mask.dtype}")
    if any(t.shape != mask.shape for t in series) or mask.numel() == 0:
        raise ValueError("apply_organ_mask: the series and the mask must share one non-empty shape")
    if any(t.device != mask.device for t in series):
        raise ValueError("apply_organ_mask: operands on different devices")
    if not -32768 <= int(fill) <= 32767:
        raise ValueError("apply_organ_mask: fill must fit int16")
    mask = mask.contiguous()
    outs = [torch.empty_like(t) for t in series]
    lib.call("dcs_organ_apply", _p(series[0]), _p(series[1]), _p(series[2]), _p(mask), mask.numel(), int(fill),
             _p(outs[0]), _p(outs[1]), _p(outs[2]), _stream())
    return tuple(outs)
