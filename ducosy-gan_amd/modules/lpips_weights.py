"""Weights of LPIPS (lpips 0.1.4, net='alex', version='0.1') from files the user names.

Nothing here is downloaded: ``--lpips_weights PATH[,PATH]`` names one or two ``torch.save``d state
dicts, which are merged.  Two namings are accepted:

  * ``lpips.LPIPS(net='alex').state_dict()``: ``net.slice1.0``, ``net.slice2.3``, ``net.slice3.6``,
    ``net.slice4.8``, ``net.slice5.10`` (``.weight`` / ``.bias``) and ``lin0.model.1.weight`` ...
    ``lin4.model.1.weight`` ([1,C,1,1]); the ``lins.*`` duplicates and ``scaling_layer.*`` are ignored;
  * torchvision's ``alexnet`` state dict (``features.0`` / ``.3`` / ``.6`` / ``.8`` / ``.10``;
    ``classifier.*`` is ignored) plus the package's ``alex.pth``, which holds only the ``linK`` keys.

The scaling layer's shift and scale are constants of the package and are built in.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Tuple

import numpy as np
import torch

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
CHANNELS = (64, 192, 384, 256, 256)
# (Cout, Cin, k, stride, pad, 3x3 stride-2 max pool in front) of the five convolutions
CONVS = ((64, 3, 11, 4, 2, False), (192, 64, 5, 1, 2, True), (384, 192, 3, 1, 1, True),
         (256, 384, 3, 1, 1, False), (256, 256, 3, 1, 1, False))
MIN_SIDE = 31   # 31 -> 7 -> 3 -> 3 -> 1; at 30 the second pool has no output
_LPIPS_CONV = ("net.slice1.0", "net.slice2.3", "net.slice3.6", "net.slice4.8", "net.slice5.10")
_TV_CONV = ("features.0", "features.3", "features.6", "features.8", "features.10")


@dataclass
class LpipsWeights:
    """float32 host tensors: ``convs[k]`` = (weight [Cout,Cin,k,k], bias [Cout]), ``lins[k]`` = [C]."""
    convs: List[Tuple[torch.Tensor, torch.Tensor]]
    lins: List[torch.Tensor]

    def tensors(self) -> List[torch.Tensor]:
        return [t for wb in self.convs for t in wb] + list(self.lins)


def out_sizes(H: int, W: int) -> List[Tuple[int, int]]:
    """The map sizes of the five taps for an H x W slice with both sides >= MIN_SIDE (floor sizes)."""
    sizes, h, w = [], H, W
    for _, _, k, s, p, pool in CONVS:
        if pool:
            h, w = (h - 3) // 2 + 1, (w - 3) // 2 + 1
        h, w = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        sizes.append((h, w))
    return sizes


def from_state_dicts(*state_dicts: Dict[str, torch.Tensor]) -> LpipsWeights:
    """Merge the given state dicts and pick the trunk and ``lin`` tensors out of them.  Raises a
    ValueError that names every missing key and every tensor of the wrong shape."""
    sd: Dict[str, torch.Tensor] = {}
    for d in state_dicts:
        if not isinstance(d, dict):
            raise ValueError("lpips weights: a state dict (a mapping of names to tensors) is required")
        sd.update(d)
    problems, convs, lins = [], [], []
    for k, (co, ci, ks, _, _, _) in enumerate(CONVS):
        base = _LPIPS_CONV[k] if _LPIPS_CONV[k] + ".weight" in sd else _TV_CONV[k]
        got = []
        for suffix, shape in ((".weight", (co, ci, ks, ks)), (".bias", (co,))):
            t = sd.get(base + suffix)
            if t is None:
                problems.append(f"missing {_TV_CONV[k]}{suffix} (or {_LPIPS_CONV[k]}{suffix})")
            elif tuple(t.shape) != shape:
                problems.append(f"{base}{suffix} has shape {tuple(t.shape)}, expected {shape}")
            else:
                got.append(t.detach().to(torch.float32).contiguous().clone())
        convs.append(tuple(got))
        name = f"lin{k}.model.1.weight"
        t = sd.get(name)
        if t is None:
            problems.append(f"missing {name}")
        elif tuple(t.shape) != (1, co, 1, 1):
            problems.append(f"{name} has shape {tuple(t.shape)}, expected {(1, co, 1, 1)}")
        else:
            lins.append(t.detach().to(torch.float32).reshape(co).contiguous().clone())
    if problems:
        raise ValueError("lpips weights: " + "; ".join(problems))
    return LpipsWeights(convs, lins)


def load(spec: str) -> LpipsWeights:
    """``PATH[,PATH]``: one or two torch.save'd state dicts, read on the host and merged."""
    paths = [p for p in str(spec).split(",") if p]
    if not 1 <= len(paths) <= 2:
        raise ValueError("--lpips_weights takes one file or two files separated by a comma")
    return from_state_dicts(*[torch.load(p, map_location="cpu") for p in paths])


def random_state_dict(seed: int = 0, layout: str = "lpips") -> Dict[str, torch.Tensor]:
    """Stand-in weights from a seeded PRNG (tests and scripts/bench_metrics.py ``random``): He-scaled
    conv weights, small biases, non-negative ``lin`` vectors.  ``layout``: 'lpips' names the trunk as
    the package does, 'torchvision' as torchvision's alexnet; the ``lin`` keys are the same."""
    rng = np.random.RandomState(seed)
    names = {"lpips": _LPIPS_CONV, "torchvision": _TV_CONV}[layout]
    sd = {}
    for k, (co, ci, ks, _, _, _) in enumerate(CONVS):
        w = rng.standard_normal((co, ci, ks, ks)) * np.sqrt(2.0 / (ci * ks * ks))
        sd[names[k] + ".weight"] = torch.from_numpy(w.astype(np.float32))
        sd[names[k] + ".bias"] = torch.from_numpy((0.05 * rng.standard_normal(co)).astype(np.float32))
        sd[f"lin{k}.model.1.weight"] = torch.from_numpy(rng.uniform(0.0, 2.0 / co, (1, co, 1, 1)).astype(np.float32))
    return sd


def stem_fold(weights: LpipsWeights, dtype=torch.float64) -> Tuple[torch.Tensor, torch.Tensor]:
    """The first convolution over the scaling layer of three equal channels as a 2-channel
    convolution over (x, 1): ``(wx, wc)`` [64,11,11] each with wx = sum_c w[o,c] / scale_c and
    wc = -sum_c w[o,c] shift_c / scale_c.  The constant channel is zero in the padding (the
    reference pads after the scaling layer), so wc is not a bias."""
    w = weights.convs[0][0].to(dtype)
    scale = torch.tensor(SCALE, dtype=dtype).view(1, 3, 1, 1)
    shift = torch.tensor(SHIFT, dtype=dtype).view(1, 3, 1, 1)
    return (w / scale).sum(1), -(w * shift / scale).sum(1)
