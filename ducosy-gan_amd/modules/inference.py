"""Inference-side math of the reference's generate.py on the MI355X path.

Mirrors the array arithmetic of modules/preprocess.py:68-113 (HU transform, clipping,
[-1, 1] normalisation, inverse mapping to stored pixel values) and generate.py:144-236 (the
complementary HU-range synthesis) and generate.py:302-477 (the enhancement-difference synthesis),
and batches the Generator forward over slices (the
reference runs one slice per call, generate.py:108-111).  DICOM parsing stays on the host
(pydicom, imported lazily by generate.py); nothing here needs it, so the math is testable
without it.
"""
from __future__ import annotations

from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F


def hu_from_stored(pixels: np.ndarray, slope: float, intercept: float) -> np.ndarray:
    """preprocess.py:76-82: stored pixel values -> HU (float32)."""
    return pixels.astype(np.float32) * float(slope) + float(intercept)


def normalise_hu(hu: np.ndarray, hu_min: float, hu_max: float) -> np.ndarray:
    """preprocess.py:84-90: clip to [hu_min, hu_max] and map linearly to [-1, 1]."""
    x = np.clip(hu, hu_min, hu_max)
    return (2 * (x - hu_min) / (hu_max - hu_min) - 1).astype(np.float32)


def stored_from_output(out: np.ndarray, hu_min: float, hu_max: float, slope: float, intercept: float,
                       dtype) -> np.ndarray:
    """preprocess.py:99-113: model output in [-1, 1] -> HU -> stored values of the original
    DICOM dtype (numpy astype truncation toward zero, as the reference)."""
    hu = (out + 1.0) / 2.0 * (hu_max - hu_min) + hu_min
    return ((hu - float(intercept)) / float(slope)).astype(dtype)


def resize(x: torch.Tensor, size: Tuple[int, int]) -> torch.Tensor:
    """torchvision.transforms.Resize(size, antialias=True) on a [N,C,H,W] float tensor
    (generate.py:52, 107-115): bilinear with antialiasing."""
    if tuple(x.shape[-2:]) == tuple(size):
        return x
    return F.interpolate(x, size=size, mode="bilinear", align_corners=False, antialias=True)


@torch.no_grad()
def translate_slices(model, slices: Sequence[np.ndarray], img_size: int, batch: int = 16,
                     device="cuda", cond: Optional[Sequence[np.ndarray]] = None) -> List[np.ndarray]:
    """Run the Generator over normalised slices ([H,W] float32 each, any size) in batches of
    `batch` at img_size x img_size, and resize each output back to its slice's size
    (generate.py:104-116).  ``cond``: per-slice mask channels [m,H,W] for a mask-conditioned
    Generator (resized nearest, concatenated after the image as in trainer.py:451-453).
    Returns [H,W] float32 arrays in [-1, 1]."""
    out: List[np.ndarray] = []
    for i in range(0, len(slices), batch):
        chunk = slices[i:i + batch]
        x = torch.stack([resize(torch.from_numpy(np.ascontiguousarray(s))[None, None], (img_size, img_size))[0]
                         for s in chunk]).to(device)
        if cond is not None:
            m = torch.stack([F.interpolate(torch.as_tensor(np.ascontiguousarray(c))[None].float(),
                                           size=(img_size, img_size), mode="nearest")[0]
                             for c in cond[i:i + batch]]).to(device)
        y = model(x) if cond is None else model(x, m)  # concat fused into the stem gather
        for s, yi in zip(chunk, y):
            out.append(resize(yi[None], tuple(s.shape))[0, 0].float().cpu().numpy())
    return out


MASK_TYPES = {"soft_tissue": ["bone", "mediastinum"], "lung": ["lung"]}  # argmanager.py:132, 149


def conditioning_types(g, kind: str, mask_types=MASK_TYPES) -> Tuple[int, Optional[List[str]]]:
    """The conditioning rule of a Generator at inference: (mask channel count, mask types).
    0 channels for an image-only Generator; the training mask types of ``kind`` when their count
    matches the checkpoint's extra input channels, else None: zero planes."""
    extra = g.input_channels - 1
    if extra <= 0:
        return 0, None
    types = list(mask_types[kind])
    return extra, (types if len(types) == extra else None)


def _conditioning(g, kind, hu_slices, device, mask_types=MASK_TYPES):
    """Per-slice mask channels for a mask-conditioned Generator (None for an image-only one):
    the training mask types when their count matches the checkpoint, else zero planes."""
    extra, types = conditioning_types(g, kind, mask_types)
    if extra <= 0:
        return None
    if types is None:
        return [np.zeros((extra,) + h.shape, np.float32) for h in hu_slices]
    from .hip import ops
    out = []
    for h in hu_slices:
        m = ops.anatomical_masks(torch.from_numpy(np.ascontiguousarray(h, np.float32)).to(device), types)
        out.append(m[0].cpu().numpy())
    return out


@torch.no_grad()
def translate_volume_device(soft_model, lung_model, raw_stored, slopes, intercepts,
                            soft_range: Tuple[float, float], lung_range: Tuple[float, float], img_size: int,
                            batch: int = 16, device="cuda", mask_types=MASK_TYPES, want_stored: bool = False,
                            nmodel=None, diffmap_threshold=8, want_diff: bool = False, synthesis: str = "range",
                            enhancement_threshold: float = 5.0, enhancement_min_hu: float = -400.0):
    """The translation of one NCCT series with both Generators and the HU-range merge, resident on
    the device: what ``_conditioning`` + ``translate_slices`` + ``stored_from_output`` per model and
    ``synthesize`` per slice compute, without a host round trip in between.

    raw_stored: [D,H,W] int16 / uint16 host array (one upload); slopes / intercepts: one rescale
    pair per slice.  HU and both [-1, 1] images come from the HU kernel, the masks from the mask
    kernel on whole chunks, the resizes to and from img_size (when the slice size differs) from
    modules/hip/slices.py, and the Generators run over chunks of exactly ``batch`` slices in series
    order (the last one short), as translate_slices does: the f16x3 operand exponent is taken over
    a whole call, so the result depends on the chunking.

    Returns the merged values as a float32 [D,H,W] device tensor, the input of
    ``smooth_volume_device``; with want_stored=True the tuple (merged, soft stored, lung stored),
    the two stored-value series as int16 device tensors (the bits of a uint16 series).

    nmodel: a modules/nmodel U-Net; the difference-map stage then runs between the merge and the
    return: the U-Net over the ``hu`` tensor that is already here, ending in the kernel that adds the
    thresholded uint8 map into ``merged`` (modules/nmodel/inference.py::apply_predicted_diffmap_device),
    no transfer.  want_diff=True appends the float difference map (device) to the result.

    synthesis="enhancement": the merged tensor is ``synthesize_enhancement`` of the two stored-value
    series (enhancement_threshold, enhancement_min_hu) instead of the HU-range merge, from one
    kernel as well; everything else is as above."""
    from .hip import ops
    from .hip import slices as S
    if synthesis not in ("range", "enhancement"):
        raise ValueError(f"translate_volume_device: synthesis {synthesis!r} (range or enhancement expected)")
    raw = np.asarray(raw_stored)
    if raw.dtype not in (np.int16, np.uint16):
        raise TypeError(f"translate_volume_device: stored dtype {raw.dtype} (int16 or uint16 expected)")
    if raw.ndim != 3 or raw.size == 0:
        raise ValueError("translate_volume_device: [D,H,W] series required")
    D, H, W = raw.shape
    if len(slopes) != D or len(intercepts) != D:
        raise ValueError("translate_volume_device: one slope/intercept per slice")
    batch, size = int(batch), (int(img_size), int(img_size))
    if batch < 1:
        raise ValueError("translate_volume_device: batch must be positive")
    unsigned = raw.dtype == np.uint16
    if unsigned and not hasattr(torch, "uint16"):
        raise RuntimeError("translate_volume_device: this torch has no uint16 tensors")
    dev = torch.device(device)
    with torch.cuda.device(dev):
        bits = torch.from_numpy(np.ascontiguousarray(raw).view(np.int16)).to(dev)
        px = bits.view(torch.uint16) if unsigned else bits
        f32 = lambda v: torch.tensor([float(x) for x in v], dtype=torch.float32).to(dev)
        slope, inter = f32(slopes), f32(intercepts)
        hu, img_soft = ops.hu_transform(px, slope, inter, soft_range[0], soft_range[1], soft=False)
        _, img_lung = ops.hu_transform(px, slope, inter, lung_range[0], lung_range[1], soft=False, want_hu=False)
        ys = []
        for kind, model, img in (("soft_tissue", soft_model, img_soft), ("lung", lung_model, img_lung)):
            extra, types = conditioning_types(model, kind, mask_types)
            chunks = []
            for i in range(0, D, batch):
                x = S.resize_aa(img[i:i + batch, None], size)
                if extra <= 0:
                    out = model(x)
                else:
                    if types is None:
                        m = torch.zeros((x.shape[0], extra) + size, dtype=torch.float32, device=dev)
                    else:
                        m = S.resize_nearest(ops.anatomical_masks(hu[i:i + batch], types), size)
                    out = model(x, m)  # concat fused into the stem gather
                chunks.append(S.resize_aa(out.float(), (H, W)))
            ys.append(torch.cat(chunks).view(D, H, W))
        if synthesis == "enhancement":
            so, lo, merged = S.translate_enhance(bits, slope, inter, ys[0], ys[1], soft_range, lung_range,
                                                 enhancement_threshold, enhancement_min_hu, unsigned=unsigned,
                                                 want_stored=want_stored)
        else:
            so, lo, _, merged = S.translate_merge(bits, slope, inter, ys[0], ys[1], soft_range, lung_range,
                                                  unsigned=unsigned, want_soft=want_stored, want_lung=want_stored,
                                                  want_merged=False, want_f32=True)
        if nmodel is None:
            return (merged, so, lo) if want_stored else merged
        from .nmodel.inference import apply_predicted_diffmap_device
        diff = apply_predicted_diffmap_device(nmodel, hu, merged, diffmap_threshold, want_diff=want_diff)
    res = (merged, so, lo) if want_stored else (merged,)
    if want_diff:
        res += (diff,)
    return res if len(res) > 1 else merged


def synthesize(raw_stored: np.ndarray, raw_hu: np.ndarray, soft_stored: np.ndarray, lung_stored: np.ndarray,
               soft_range: Tuple[float, float], lung_range: Tuple[float, float]) -> np.ndarray:
    """generate.py:212-236: start from the NCCT stored values and overwrite the pixels whose
    NCCT HU lies in each model's HU range with that model's output (soft tissue first, lung
    second, so lung wins where the ranges touch)."""
    merged = raw_stored.copy()
    soft = (raw_hu >= soft_range[0]) & (raw_hu <= soft_range[1])
    lung = (raw_hu >= lung_range[0]) & (raw_hu <= lung_range[1])
    merged[soft] = soft_stored[soft]
    merged[lung] = lung_stored[lung]
    return merged


def synthesize_enhancement(raw_stored: np.ndarray, soft_stored: np.ndarray, lung_stored: np.ndarray, slope: float,
                           intercept: float, threshold: float = 5.0, min_hu: float = -400.0,
                           soft_rescale: Optional[Tuple[float, float]] = None,
                           lung_rescale: Optional[Tuple[float, float]] = None) -> np.ndarray:
    """generate.py:302-477 (synthesis_test, "sCECT v3") for one slice: keep the NCCT stored values
    and add each model's HU gain over the NCCT, as stored-value units, where that gain exceeds
    ``threshold`` and the NCCT HU exceeds ``min_hu`` (both strict; soft tissue first, then lung, a
    voxel can take both).  float32 throughout, one operation per step; the result is float32 and
    generally not integral.  soft_rescale / lung_rescale: (slope, intercept) of the two translated
    series when they differ from the NCCT's (the reference reads each file's own pair)."""
    f = np.float32
    a, b = f(slope), f(intercept)
    (sa, sb), (la, lb) = ((a, b) if p is None else (f(p[0]), f(p[1])) for p in (soft_rescale, lung_rescale))
    m = np.asarray(raw_stored).astype(f)      # astype copies: the input stays untouched
    hr = m * a + b
    es = (np.asarray(soft_stored).astype(f) * sa + sb) - hr
    el = (np.asarray(lung_stored).astype(f) * la + lb) - hr
    valid = hr > f(min_hu)
    for e in (es, el):
        k = (e > f(threshold)) & valid
        m[k] = m[k] + e[k] / a
    return m


def synthesize_volume(raw_stored, slopes, intercepts, soft_stored, lung_stored, soft_range: Tuple[float, float],
                      lung_range: Tuple[float, float], device=None, keep_on_device: bool = False,
                      mode: str = "range", threshold: float = 5.0, min_hu: float = -400.0):
    """``synthesize`` over a whole series: [D,H,W] stored values (int16 or uint16) of the NCCT
    and the two translations, one rescale slope / intercept per slice -> merged stored values.
    device=None: the per-slice host code.  With a device the merge runs in one kernel there
    (modules/hip/volume.py); keep_on_device=True then returns the merged values as a float32
    device tensor, the input of ``smooth_volume(..., device=...)``, instead of downloading.

    mode="enhancement": ``synthesize_enhancement`` (threshold, min_hu) in place of ``synthesize``;
    the result is float32 (a numpy array, or the device tensor with keep_on_device=True) and the
    two HU ranges are not used."""
    if mode not in ("range", "enhancement"):
        raise ValueError(f"synthesize_volume: mode {mode!r} (range or enhancement expected)")
    raw = np.asarray(raw_stored)
    if device is None:
        if mode == "enhancement":
            return np.stack([synthesize_enhancement(r, s, g, a, b, threshold, min_hu)
                             for r, a, b, s, g in zip(raw, slopes, intercepts, np.asarray(soft_stored),
                                                      np.asarray(lung_stored))])
        return np.stack([synthesize(r, hu_from_stored(r, a, b), s, g, soft_range, lung_range)
                         for r, a, b, s, g in zip(raw, slopes, intercepts, np.asarray(soft_stored),
                                                  np.asarray(lung_stored))])
    from .hip import volume as V
    if raw.dtype not in (np.int16, np.uint16):
        raise TypeError(f"synthesize_volume: stored dtype {raw.dtype} (int16 or uint16 expected)")
    dev = torch.device(device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=raw.dtype).view(np.int16)).to(dev)
    f32 = lambda v: torch.tensor([float(x) for x in v], dtype=torch.float32)
    with torch.cuda.device(dev):
        if mode == "enhancement":
            f = V.merge_enhancement(up(raw), up(soft_stored), up(lung_stored), f32(slopes), f32(intercepts),
                                    threshold, min_hu, unsigned=raw.dtype == np.uint16)
            return f if keep_on_device else f.cpu().numpy()
        out, f = V.merge_hu_ranges(up(raw), up(soft_stored), up(lung_stored), f32(slopes), f32(intercepts),
                                   soft_range, lung_range, unsigned=raw.dtype == np.uint16,
                                   want_stored=not keep_on_device, want_f32=keep_on_device)
        return f if keep_on_device else out.cpu().numpy().view(raw.dtype)


SMOOTH_KW = dict(method="gaussian3d", sigma_z=0.7, sigma_xy=0.05, enhance_sharpness=True, sharpen_amount=1.7,
                 sharpen_radius=1.2)  # generate.py:251-253


def smooth_volume_device(vol: torch.Tensor) -> torch.Tensor:
    """``smooth_volume`` of a float32 [D,H,W] device tensor, result left on the device (int16)."""
    from .hip import volume as V
    from .postprocess_gpu import postprocess_ct_volume_device
    with torch.cuda.device(vol.device):
        return postprocess_ct_volume_device(V.gaussian_filter1d(vol, 0.8, 0), **SMOOTH_KW)


def smooth_volume(volume: Iterable[np.ndarray], device=None) -> np.ndarray:
    """generate.py:246-254: z Gaussian (sigma 0.8) of the merged stored-value volume, then
    modules/postprocess.py's 'gaussian3d' (sigma_z 0.7, sigma_xy 0.05) with sharpening (1.7 /
    1.2); voxels >= 750 keep their value; int16 out.  device=None runs on the host (scipy); with
    a device the same arithmetic runs on the volume kernels there, bit-identical
    (modules/postprocess_gpu.py); ``volume`` may then be a float32 device tensor."""
    if device is not None:
        dev = torch.device(device)
        if isinstance(volume, torch.Tensor):
            vol = volume.to(device=dev, dtype=torch.float32)
        else:
            vol = torch.from_numpy(np.asarray(volume, dtype=np.float32)).to(dev)
        return smooth_volume_device(vol).cpu().numpy()
    from scipy.ndimage import gaussian_filter1d
    from .postprocess import postprocess_ct_volume
    vol = gaussian_filter1d(np.asarray(volume, dtype=np.float32), sigma=0.8, axis=0)
    return postprocess_ct_volume(vol, **SMOOTH_KW)
