"""Evaluation metrics of calculate.py on the device (csrc/metrics.hip through modules/hip/metrics.py).

The same functions as modules/metrics.py, on float32 [D,H,W] device tensors: every metric
returns ``(aggregate, per_slice_list)`` and follows the arithmetic fixed in that module's
docstring, so the two paths agree to the rounding of float64 sums taken in different orders
(tests/test_gpu_metrics.py).  A volume is read by a handful of bandwidth-bound passes:

  * one pass over the pair gives the per-slice sums behind MAE, PSNR and cosine similarity and
    the min/max of both volumes (``PairStats``);
  * the ``*_norm`` variants read the raw volumes again and normalise on the fly, bit for bit as
    ``normalize`` does, so no normalised copy is written;
  * SSIM, the Sobel texture similarity and the Euclidean distance take one pass each; EMD sorts
    the raw rows with torch.sort (plumbing) and takes one more pass.  The float32 normalisation
    ``(x - min) / div`` with div > 0 is monotone, so sorting before it gives the same sorted
    normalised samples as sorting after it;
  * MS-SSIM, computed only when asked for, re-normalises both volumes, pools them four times
    (one launch per level for the pair) and takes one pass per level; the level means come to
    the host and the powers and the product run there, shared with the host path.  Parity with
    torchmetrics is unpinned (modules/metrics.py);
  * LPIPS, computed only with weights, runs the AlexNet trunk on both volumes in chunks of slices
    (modules/hip/lpips.py): the first layer reads the normalised volumes and re-normalises on the
    fly, and only the five per-slice tap sums come to the host;
  * the region-wise evaluation (``region_metrics``, calculate.py --regions) takes one pass over the
    three series for the 21 sums of every slice and one SSIM pass that sums the map per region.

Only per-slice float64 vectors come back to the host.  No CPU fallback: host tensors raise.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import metrics as M
from .hip import lpips as L
from .hip import metrics as K

Result = M.Result


def _rng32(mn, mx) -> np.float32:
    return np.float32(mx) - np.float32(mn)


class PairStats:
    """The per-slice sums and extrema of a (target, prediction) pair, on the host."""

    def __init__(self, a: torch.Tensor, b: torch.Tensor, affine=None):
        self.dev = K.pair_stats(a, b, affine)
        self.h = self.dev.cpu().numpy()
        self.D, self.n = a.shape[0], a.shape[1] * a.shape[2]
        h = self.h
        self.amin, self.amax = np.float32(h[:, K.MIN_A].min()), np.float32(h[:, K.MAX_A].max())
        self.bmin, self.bmax = np.float32(h[:, K.MIN_B].min()), np.float32(h[:, K.MAX_B].max())

    def mae(self) -> Result:
        s = self.h[:, K.SUM_ABS]
        return float(s.sum() / (self.D * self.n)), (s / self.n).tolist()

    def psnr(self) -> Result:
        s = self.h[:, K.SUM_SQ]
        return M.psnr_from_mse(float(s.sum() / (self.D * self.n)), s / self.n, M.max_pixel_of(self.amin, self.amax))

    def cs(self) -> Result:
        vals = [M.cs_from_sums(r[K.SUM_AB], r[K.SUM_AA], r[K.SUM_BB]) for r in self.h]
        return float(np.mean(vals)), vals

    def normalize_affine(self):
        """(a_off, a_div, b_off, b_div) of normalize() on each volume; div 0 stands for zeros."""
        return (float(self.amin), float(_rng32(self.amin, self.amax)),
                float(self.bmin), float(_rng32(self.bmin, self.bmax)))


def _check_window(a) -> None:
    """SSIM's shape error, raised before anything is launched."""
    if isinstance(a, torch.Tensor) and a.dim() == 3 and min(a.shape[1:]) < M.SSIM_WIN:
        raise ValueError("ssim: win_size exceeds image extent: both sides of a slice must be at least 7")


def _ssim(a, b, data_range: float, affine=None) -> Result:
    sums = K.ssim_sums(a, b, data_range, affine).cpu().numpy()
    vals = (sums / ((a.shape[1] - 6) * (a.shape[2] - 6))).tolist()
    return float(np.mean(vals)), vals


def _emd(a, b, st: PairStats) -> Result:
    gmin = min(st.amin, st.bmin)
    div = np.float32(max(st.amax, st.bmax) - gmin) + M.EPS32
    D = a.shape[0]
    # sorting the raw rows: the normalisation is monotone, see the module docstring
    sa = torch.sort(a.reshape(D, -1), dim=1).values.reshape(a.shape)
    sb = torch.sort(b.reshape(D, -1), dim=1).values.reshape(b.shape)
    sums = K.sorted_l1(sa, sb, (float(gmin), float(div), float(gmin), float(div))).cpu().numpy()
    vals = (sums / st.n / st.n).tolist()
    return float(np.mean(vals)), vals


def _ts(a, b) -> Result:
    r = K.sobel_ts(a, b).cpu().numpy()
    n = a.shape[1] * a.shape[2]
    vals = [M.ts_from_sums(float(s), float(m1), float(m2), n) for s, m1, m2 in r]
    return float(np.mean(vals)), vals


def _ed(a, b, st: PairStats) -> Result:
    sums = K.ed_sums(a, b, st.dev).cpu().numpy()
    vals = (np.sqrt(sums) / st.n).tolist()
    return float(np.mean(vals)), vals


def minmax(x: torch.Tensor):
    """(min, max) of a device volume as numpy float32, exact."""
    st = PairStats(x, x)
    return st.amin, st.amax


def normalize(x: torch.Tensor) -> torch.Tensor:
    mn, mx = minmax(x)
    return K.normalize(x, float(mn), float(_rng32(mn, mx)))


def mae(img1, img2) -> Result:
    return PairStats(img1, img2).mae()


def psnr(img1, img2) -> Result:
    return PairStats(img1, img2).psnr()


def cs(img1, img2) -> Result:
    return PairStats(img1, img2).cs()


def ssim(img1, img2) -> Result:
    _check_window(img1)
    st = PairStats(img1, img2)
    return _ssim(img1, img2, float(_rng32(st.bmin, st.bmax)))


def emd(img1, img2) -> Result:
    return _emd(img1, img2, PairStats(img1, img2))


def ts(img1, img2) -> Result:
    return _ts(img1, img2)


def ed(img1, img2) -> Result:
    return _ed(img1, img2, PairStats(img1, img2))


def ms_ssim_pyramid(img1, img2):
    """modules/metrics.py::ms_ssim_pyramid on the device: the five float32 levels of both
    re-normalised volumes, bit for bit the host's."""
    a, b = K._pair(img1, img2, "ms_ssim")
    if not M.ms_ssim_defined(a.shape):
        raise ValueError(f"ms_ssim: both sides of a slice must be at least {M.MS_SSIM_MIN_SIDE}")
    st = PairStats(a, b)
    # div = range + 1e-8f is never 0, so the kernel's zero branch is not taken
    levels = [(K.normalize(a, float(st.amin), float(_rng32(st.amin, st.amax) + M.EPS32)),
               K.normalize(b, float(st.bmin), float(_rng32(st.bmin, st.bmax) + M.EPS32)))]
    for _ in range(len(M.MS_SSIM_BETAS) - 1):
        levels.append(K.pool2(*levels[-1]))
    return levels


def ms_ssim_levels(img1, img2) -> np.ndarray:
    """modules/metrics.py::ms_ssim_levels: float64 [5][D][2], the only values that come to the
    host besides the extrema of the re-normalisation."""
    sums, counts = [], []
    for x, y in ms_ssim_pyramid(img1, img2):
        counts.append((x.shape[1] - 10) * (x.shape[2] - 10))
        sums.append(K.msssim_level_sums(x, y, M.MS_SSIM_WINDOW, M.MS_SSIM_C1, M.MS_SSIM_C2))
    return torch.stack(sums).cpu().numpy() / np.array(counts, np.float64)[:, None, None]


def ms_ssim_slices(img1, img2) -> list:
    a, b = K._pair(img1, img2, "ms_ssim")
    if not M.ms_ssim_defined(a.shape):
        return []
    return M.ms_ssim_from_levels(ms_ssim_levels(a, b))


def ms_ssim(img1, img2) -> Result:
    """modules/metrics.py::ms_ssim; ``(nan, [])`` below 176 pixels on a side, without a launch."""
    vals = ms_ssim_slices(img1, img2)
    return M.ms_ssim_result(vals) if vals else (float("nan"), [])


def lpips_taps(img1, img2, weights, chunk: Optional[int] = None) -> np.ndarray:
    """modules/metrics.py::lpips_taps on the device: float64 [5][D], the only values that come to
    the host besides the extrema of the re-normalisation.  ``chunk``: slices per pass (default: as
    many as keep the feature maps within modules/hip/lpips.py::CHUNK_BYTES); no value depends on it."""
    a, b = K._pair(img1, img2, "lpips")
    if not M.lpips_defined(a.shape):
        raise ValueError(f"lpips: both sides of a slice must be at least {M.LPIPS_MIN_SIDE}")
    st = PairStats(a, b)
    # div = range + 1e-8f is never 0; the first layer's kernel re-normalises while it reads
    aff = (float(st.amin), float(_rng32(st.amin, st.amax) + M.EPS32), float(st.bmin), float(_rng32(st.bmin, st.bmax) + M.EPS32))
    sums = L.tap_sums(a, b, aff, weights, chunk).cpu().numpy()
    counts = np.array([h * w for h, w in L.LW.out_sizes(a.shape[1], a.shape[2])], np.float64)
    return sums / counts[:, None]


def lpips(img1=None, img2=None, weights=None, chunk: Optional[int] = None) -> Result:
    """modules/metrics.py::lpips on device tensors; ``(nan, [])`` without weights and below 31
    pixels on a side, without a launch."""
    if weights is None:
        return float("nan"), []
    if isinstance(img1, torch.Tensor) and img1.dim() == 3 and not M.lpips_defined(img1.shape):
        return float("nan"), []
    return M.lpips_from_taps(lpips_taps(img1, img2, weights, chunk))


_ms_ssim = ms_ssim


def to_device(x, device) -> torch.Tensor:
    """A float32 device tensor of a numpy array or tensor (one upload)."""
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return x.to(device=device, dtype=torch.float32)


def evaluate_pair(target, pred, device, advanced: bool = True, ms_ssim: bool = False,
                  lpips_weights=None) -> Dict[str, Result]:
    """modules/metrics.py::evaluate_pair on ``device``."""
    t, p = to_device(target, device), to_device(pred, device)
    _check_window(t)
    st = PairStats(t, p)
    aff = st.normalize_affine()
    stn = PairStats(t, p, aff)
    out = {"mae": st.mae(), "psnr": st.psnr(), "ssim": _ssim(t, p, float(_rng32(st.bmin, st.bmax))),
           "mae_norm": stn.mae(), "psnr_norm": stn.psnr(),
           "ssim_norm": _ssim(t, p, float(_rng32(stn.bmin, stn.bmax)), aff)}
    if advanced:
        ms = lp = lpips()   # not asked for: empty
        want_lp = lpips_weights is not None and M.lpips_defined(t.shape)
        if ms_ssim or want_lp:   # on materialised normalize() volumes, as the host path does
            tn, pn = K.normalize(t, aff[0], aff[1]), K.normalize(p, aff[2], aff[3])
            ms = _ms_ssim(tn, pn) if ms_ssim else ms
            lp = lpips(tn, pn, lpips_weights) if want_lp else lp
        out.update({"ms_ssim": ms, "lpips": lp, "emd": _emd(t, p, st),
                    "ts": _ts(t, p), "cs": st.cs(), "ed": _ed(t, p, st)})
    return out


def region_arrays(vue: torch.Tensor, std: torch.Tensor, gen: torch.Tensor, spec: M.RegionSpec = M.RegionSpec()):
    """(region_sums [D,21], region_ssim_sums [D,8], max_pixel) of modules/metrics.py on device
    volumes, as host arrays: one pass for the extrema of std and gen, one over the three series
    (it writes a byte per voxel: the region map), one for the SSIM map read against that map."""
    st = PairStats(std, gen)
    sums, rmap = K.region_sums(vue, std, gen, spec.ranges(), with_map=min(std.shape[1:]) >= M.SSIM_WIN)
    if rmap is None:   # a side below 7: no SSIM cell
        ssim_sums = np.zeros((std.shape[0], M.REGION_NSSIM), dtype=np.float64)
    else:
        ssim_sums = K.region_ssim_sums(std, gen, rmap, float(_rng32(st.bmin, st.bmax))).cpu().numpy()
    return sums.cpu().numpy(), ssim_sums, M.max_pixel_of(st.amin, st.amax)


def region_metrics(std, gen, vue, device: Optional[object] = "cuda", spec: M.RegionSpec = M.RegionSpec()):
    """modules/metrics.py::region_metrics; ``device=None`` runs the host module.  Series that are
    device tensors already (the ones evaluate_patient was given in the same call) are used as
    they are: nothing is uploaded twice."""
    if device is None:
        return M.region_metrics(std, gen, vue, spec)
    n = min(len(x) for x in (std, gen, vue))
    v, s, g = (to_device(x, device)[:n].contiguous() for x in (vue, std, gen))
    return M.region_from_sums(*region_arrays(v, s, g, spec))


def evaluate_patient(std, gen, vue=None, device: Optional[object] = "cuda", ms_ssim: bool = False, lpips_weights=None):
    """modules/metrics.py::evaluate_patient; ``device=None`` runs the host module, anything else
    uploads every series once and keeps the work on that device."""
    if device is None:
        return M.evaluate_patient(std, gen, vue, ms_ssim, lpips_weights)
    up = lambda v: None if v is None else to_device(v, device)
    return M.collect_patient(lambda t, p, adv, **kw: evaluate_pair(t, p, device, adv, **kw), up(std), up(gen), up(vue),
                             ms_ssim, lpips_weights)
