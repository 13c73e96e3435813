"""Evaluation metrics of calculate.py on the host: MAE, PSNR, SSIM, EMD, texture similarity,
cosine similarity and Euclidean distance of two float32 [D,H,W] volumes, ``img1`` the target
and ``img2`` the prediction.  Every metric returns ``(aggregate, per_slice_list)``.

The formulas and branches are the reference's.  Its numerics depend on the skimage version and
on numpy's float32 pairwise sums, so the arithmetic is fixed here, and modules/metrics_gpu.py
(csrc/metrics.hip) follows the same rules:

  * the elementwise steps of the reference's numpy expressions stay in float32: ``img1 - img2``,
    its square, ``normalize``, the ``(s - min) / (max - min + 1e-8)`` of EMD and ED (1e-8 as a
    float32 constant), the difference of the normalised slices;
  * every reduction (sum, mean, norm, dot) accumulates in float64; a norm or dot squares and
    multiplies in float64 too, as a float64 norm or dot does;
  * skimage's structural_similarity and sobel are restated in float64 on the float32 samples;
  * min and max are exact.

ms_ssim restates torchmetrics' MultiScaleStructuralSimilarityIndexMeasure(data_range=1.0) with
its defaults (rules at ``ms_ssim_levels``).  torchmetrics is not installed, so parity with the
reference's own output is unpinned; the two paths here agree with each other and with a direct
float64 formula (tests/test_cpu_msssim.py, tests/test_gpu_msssim.py).  lpips restates
lpips.LPIPS(net='alex') with ATen on weights the user names (modules/lpips_weights.py; rules at
``lpips_taps``) and returns ``(nan, [])`` without them, as the reference does without the library.

region_metrics (calculate.py --regions) is this package's own: the same error measures per HU-range
owner of synthesis() and over the enhancing voxels, from three series (rules at ``REGIONS``).
"""
from __future__ import annotations

import csv
from typing import Dict, List, NamedTuple, Sequence, Tuple

import numpy as np
from scipy.ndimage import correlate1d, uniform_filter

Result = Tuple[float, List[float]]
BASIC = ("mae", "psnr", "ssim", "mae_norm", "psnr_norm", "ssim_norm")
ADVANCED = ("ms_ssim", "lpips", "emd", "ts", "cs", "ed")
METRICS = BASIC + ADVANCED
EPS32 = np.float32(1e-8)
SSIM_WIN = 7
# MS-SSIM: torchmetrics' defaults.  The 11-tap gaussian (sigma 1.5) normalised to sum 1 in float64;
# the device path passes these eleven doubles to its kernel, so both filter with the same bits.
MS_SSIM_BETAS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MS_SSIM_TAPS = 11
MS_SSIM_MIN_SIDE = 176   # the fifth level must hold one window: 176 -> 88 -> 44 -> 22 -> 11
MS_SSIM_C1, MS_SSIM_C2 = 0.01 ** 2, 0.03 ** 2
LPIPS_MIN_SIDE = 31      # AlexNet's maps: 31 -> 7 -> 3 -> 3 -> 1; at 30 the second pool has no output
_g = np.exp(-((np.arange(MS_SSIM_TAPS, dtype=np.float64) - 5) / 1.5) ** 2 / 2)
MS_SSIM_WINDOW = _g / _g.sum()
MS_SSIM_WINDOW.setflags(write=False)


def _f32(img) -> np.ndarray:
    a = np.ascontiguousarray(img, dtype=np.float32)
    if a.ndim != 3:
        raise ValueError("a [D,H,W] volume is required")
    return a


def _pair(img1, img2):
    a, b = _f32(img1), _f32(img2)
    if a.shape != b.shape:
        raise ValueError(f"volumes differ in shape: {a.shape} and {b.shape}")
    return a, b


def _slice_mean(x: np.ndarray) -> np.ndarray:
    return np.mean(x.reshape(x.shape[0], -1), axis=1, dtype=np.float64)


def normalize(data) -> np.ndarray:
    """Volume-global min/max to [0,1] in float32; zeros when the range is 0."""
    data = np.asarray(data, dtype=np.float32)
    mn, mx = data.min(), data.max()
    if mx - mn == 0:
        return np.zeros_like(data)
    return (data - mn) / (mx - mn)


def mae(img1, img2) -> Result:
    a, b = _pair(img1, img2)
    diff = np.abs(a - b)
    return float(np.mean(diff, dtype=np.float64)), _slice_mean(diff).tolist()


def psnr_from_mse(mse: float, slice_mse: Sequence[float], max_pixel: float) -> Result:
    """PSNR's branches given the float64 mean squared errors (shared with the device path)."""
    if mse == 0:
        return float("inf"), [float("inf")] * len(slice_mse)
    with np.errstate(divide="ignore"):
        val = lambda m: float("inf") if m == 0 else float(20 * np.log10(np.float64(max_pixel) / np.sqrt(np.float64(m))))
        return val(mse), [val(m) for m in slice_mse]


def max_pixel_of(mn: np.float32, mx: np.float32) -> float:
    rng = np.float32(mx) - np.float32(mn)
    return 1.0 if rng == 0 else float(rng)


def psnr(img1, img2) -> Result:
    a, b = _pair(img1, img2)
    sq = (a - b) ** 2
    return psnr_from_mse(float(np.mean(sq, dtype=np.float64)), _slice_mean(sq), max_pixel_of(a.min(), a.max()))


def ssim_map(s1: np.ndarray, s2: np.ndarray, data_range: float) -> np.ndarray:
    """The full SSIM map of skimage.metrics.structural_similarity with its defaults, in float64
    (ssim_slice averages its interior; region_ssim_sums sums it per region)."""
    if min(s1.shape) < SSIM_WIN:
        raise ValueError("win_size exceeds image extent: both sides of a slice must be at least 7")
    x, y = s1.astype(np.float64), s2.astype(np.float64)
    n = SSIM_WIN * SSIM_WIN
    cov_norm = n / (n - 1.0)
    filt = lambda v: uniform_filter(v, size=SSIM_WIN, mode="reflect")
    ux, uy = filt(x), filt(y)
    uxx, uyy, uxy = filt(x * x), filt(y * y), filt(x * y)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    with np.errstate(invalid="ignore", divide="ignore"):
        return ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))


def ssim_slice(s1: np.ndarray, s2: np.ndarray, data_range: float) -> float:
    """skimage.metrics.structural_similarity with its defaults, in float64."""
    s = ssim_map(s1, s2, data_range)
    p = (SSIM_WIN - 1) // 2
    return float(np.mean(s[p:s.shape[0] - p, p:s.shape[1] - p], dtype=np.float64))


def ssim(img1, img2) -> Result:
    a, b = _pair(img1, img2)
    if a.shape[1] < SSIM_WIN or a.shape[2] < SSIM_WIN:
        raise ValueError("win_size exceeds image extent: both sides of a slice must be at least 7")
    data_range = float(b.max() - b.min())
    vals = [ssim_slice(s1, s2, data_range) for s1, s2 in zip(a, b)]
    return float(np.mean(vals)), vals


def ms_ssim_defined(shape) -> bool:
    return len(shape) == 3 and min(shape[1:]) >= MS_SSIM_MIN_SIDE


def ms_ssim_renormalize(x) -> np.ndarray:
    """``(x - min) / (max - min + 1e-8)`` over the volume in float32 (the reference's step before
    the metric); the identity on the output of normalize(), where 1 + 1e-8 rounds to 1."""
    x = _f32(x)
    mn, mx = x.min(), x.max()
    return (x - mn) / ((mx - mn) + EPS32)


def ms_ssim_pool(x: np.ndarray) -> np.ndarray:
    """2x2 average with floor sizes: float32(((a + b) + c) + d) * 0.25), the sum in float64."""
    h, w = x.shape[1] // 2 * 2, x.shape[2] // 2 * 2
    v = x[:, :h, :w].astype(np.float64)
    s = ((v[:, 0::2, 0::2] + v[:, 0::2, 1::2]) + v[:, 1::2, 0::2]) + v[:, 1::2, 1::2]
    return (s * 0.25).astype(np.float32)


def ms_ssim_pyramid(img1, img2) -> List[Tuple[np.ndarray, np.ndarray]]:
    """The five float32 levels of both re-normalised volumes."""
    a, b = _pair(img1, img2)
    if not ms_ssim_defined(a.shape):
        raise ValueError(f"ms_ssim: both sides of a slice must be at least {MS_SSIM_MIN_SIDE}")
    levels = [(ms_ssim_renormalize(a), ms_ssim_renormalize(b))]
    for _ in range(len(MS_SSIM_BETAS) - 1):
        levels.append((ms_ssim_pool(levels[-1][0]), ms_ssim_pool(levels[-1][1])))
    return levels


def _ms_ssim_filter(v: np.ndarray) -> np.ndarray:
    """The separable window along W, then along H; only the windows inside the image are kept
    (torchmetrics pads by 5 with reflection and crops 5 again, which leaves exactly these)."""
    r = MS_SSIM_TAPS // 2
    f = correlate1d(correlate1d(v, MS_SSIM_WINDOW, axis=1, mode="reflect"), MS_SSIM_WINDOW, axis=0, mode="reflect")
    return f[r:v.shape[0] - r, r:v.shape[1] - r]


def ms_ssim_level_slice(s1: np.ndarray, s2: np.ndarray) -> Tuple[float, float]:
    """The float64 means of the SSIM map and of its contrast-structure factor over the interior
    (h-10) x (w-10) of one slice of one level; no N/(N-1) factor."""
    x, y = s1.astype(np.float64), s2.astype(np.float64)
    ux, uy = _ms_ssim_filter(x), _ms_ssim_filter(y)
    vx = _ms_ssim_filter(x * x) - ux * ux
    vy = _ms_ssim_filter(y * y) - uy * uy
    vxy = _ms_ssim_filter(x * y) - ux * uy
    upper, lower = 2 * vxy + MS_SSIM_C2, vx + vy + MS_SSIM_C2
    cs_map = upper / lower
    sim = ((2 * (ux * uy) + MS_SSIM_C1) * upper) / ((ux * ux + uy * uy + MS_SSIM_C1) * lower)
    return float(np.mean(sim, dtype=np.float64)), float(np.mean(cs_map, dtype=np.float64))


def ms_ssim_levels(img1, img2) -> np.ndarray:
    """float64 [5][D][2]: per level and slice the mean of the SSIM map and of its contrast-structure
    factor, before the clamp.  The rules, torchmetrics' defaults restated:

      * both volumes are re-normalised (ms_ssim_renormalize);
      * five levels; the next is the 2x2 average of the last with floor sizes (ms_ssim_pool),
        stored as float32;
      * at every level the 11-tap gaussian (MS_SSIM_WINDOW) filters x, y, x^2, y^2 and xy in
        float64 on the float32 samples, over the windows that lie inside the image;
      * cs = (2 sxy + C2) / (sx2 + sy2 + C2), sim = ((2 ux uy + C1)(2 sxy + C2)) /
        ((ux^2 + uy^2 + C1)(sx2 + sy2 + C2)), C1 = 0.01^2, C2 = 0.03^2.
    Raises ValueError below 176 pixels on a side, where the fifth level cannot hold a window."""
    out = [[ms_ssim_level_slice(s1, s2) for s1, s2 in zip(x, y)] for x, y in ms_ssim_pyramid(img1, img2)]
    return np.array(out, dtype=np.float64)


def ms_ssim_from_levels(levels) -> List[float]:
    """Per slice ``prod_{i<4} cs_i^beta_i * sim_4^beta_4`` of the level means clamped below at 0
    (normalize='relu'), in float64 (shared with the device path)."""
    lv = np.maximum(np.asarray(levels, dtype=np.float64), 0.0)
    last = len(MS_SSIM_BETAS) - 1
    val = lv[last, :, 0] ** MS_SSIM_BETAS[last]
    for i in range(last - 1, -1, -1):
        val = lv[i, :, 1] ** MS_SSIM_BETAS[i] * val
    return val.tolist()


def ms_ssim_result(vals: Sequence[float]) -> Result:
    """The reference returns the batch value repeated for every slice."""
    agg = float(np.mean(vals))
    return agg, [agg] * len(vals)


def ms_ssim_slices(img1, img2) -> List[float]:
    """MS-SSIM of every slice; [] where it is not defined (a side below 176)."""
    a, b = _pair(img1, img2)
    if not ms_ssim_defined(a.shape):
        return []
    return ms_ssim_from_levels(ms_ssim_levels(a, b))


def ms_ssim(img1, img2) -> Result:
    """torchmetrics' MultiScaleStructuralSimilarityIndexMeasure(data_range=1.0) of the re-normalised
    volumes: the mean over the slices, repeated for every slice.  ``(nan, [])`` below 176 pixels on
    a side, as the reference gives where torchmetrics refuses the image."""
    vals = ms_ssim_slices(img1, img2)
    return ms_ssim_result(vals) if vals else (float("nan"), [])


def lpips_defined(shape) -> bool:
    return len(shape) == 3 and min(shape[1:]) >= LPIPS_MIN_SIDE


def lpips_input(x) -> np.ndarray:
    """The reference's input chain in float32: the re-normalised volume mapped to [-1, 1]."""
    return ms_ssim_renormalize(x) * np.float32(2) - np.float32(1)


def lpips_features(x, weights, dtype=None, stem=None):
    """The five ReLU outputs of the AlexNet trunk for slices x [N,H,W] (values of lpips_input; an
    array, or a tensor with the weights on its device), as torch tensors [N,C,h,w] of ``dtype``
    (default float32).  ``stem``: a function (x [N,1,H,W],
    weights) -> the first convolution's output before the ReLU, in place of the scaling layer on
    three equal channels and the 3-channel convolution (tests/test_cpu_lpips.py: the folds)."""
    import torch
    import torch.nn.functional as F
    from . import lpips_weights as LW
    dtype = dtype or torch.float32
    if not isinstance(x, torch.Tensor):
        x = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32))
    x = x.to(dtype).unsqueeze(1)
    feats = []
    for k, (_, _, _, stride, pad, pool) in enumerate(LW.CONVS):
        w, b = (t.to(dtype) for t in weights.convs[k])
        if k == 0 and stem is not None:
            x = stem(x, weights)
        elif k == 0:
            shift = torch.tensor(LW.SHIFT, dtype=dtype, device=x.device).view(1, 3, 1, 1)
            scale = torch.tensor(LW.SCALE, dtype=dtype, device=x.device).view(1, 3, 1, 1)
            x = F.conv2d((x.repeat(1, 3, 1, 1) - shift) / scale, w, b, stride=stride, padding=pad)
        else:
            x = F.conv2d(F.max_pool2d(x, 3, 2) if pool else x, w, b, stride=stride, padding=pad)
        x = F.relu(x)
        feats.append(x)
    return feats


def lpips_tap(f1, f2, lin):
    """One tap's distance of two feature tensors [N,C,h,w] -> [N]: channel-wise unit normalisation
    (eps 1e-10 on the norm), squared difference, the 1x1 projection ``lin`` [C], the spatial mean."""
    n1 = f1 / (f1.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    n2 = f2 / (f2.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    return ((n1 - n2).pow(2) * lin.to(f1.dtype).view(1, -1, 1, 1)).sum(1).mean((1, 2))


def lpips_taps(img1, img2, weights, dtype=None) -> np.ndarray:
    """float64 [5][D]: per tap and slice the spatial mean of the ``lin``-weighted squared difference
    of the unit-normalised features, computed with ATen on the host in ``dtype`` (default float32,
    as the reference does on the CPU; float64 is the oracle of the tests).  The rules, lpips 0.1.4
    with net='alex', version='0.1', lpips=True, spatial=False in eval mode restated:

      * both volumes go through lpips_input in float32, then the scaling layer (x - shift) / scale
        on three equal channels;
      * torchvision's AlexNet ``features`` with zero padding, biases and floor-sized 3x3 stride-2
        max pools; the five ReLU outputs are the taps (modules/lpips_weights.py::CONVS);
      * per tap lpips_tap; a slice's value is the sum over the taps.
    Slices are independent, so they run in chunks.  Raises ValueError below 31 pixels on a side."""
    import torch
    a, b = _pair(img1, img2)
    if not lpips_defined(a.shape):
        raise ValueError(f"lpips: both sides of a slice must be at least {LPIPS_MIN_SIDE}")
    xa, xb = lpips_input(a), lpips_input(b)
    step = max(1, (1 << 22) // (a.shape[1] * a.shape[2]))
    out = np.empty((len(weights.lins), a.shape[0]), dtype=np.float64)
    with torch.no_grad():
        for i in range(0, a.shape[0], step):
            fa = lpips_features(xa[i:i + step], weights, dtype)
            fb = lpips_features(xb[i:i + step], weights, dtype)
            for k, lin in enumerate(weights.lins):
                out[k, i:i + step] = lpips_tap(fa[k], fb[k], lin).to(torch.float64).numpy()
    return out


def lpips_from_taps(taps) -> Result:
    """The sum over the taps per slice, and the mean over the slices (shared with the device path)."""
    vals = np.asarray(taps, dtype=np.float64).sum(axis=0)
    return float(np.mean(vals)), vals.tolist()


def lpips(img1, img2, weights=None, dtype=None) -> Result:
    """lpips.LPIPS(net='alex') of the re-normalised volumes with the given weights
    (modules/lpips_weights.py): the mean over the slices and the per-slice values.  ``(nan, [])``
    without weights, as the reference gives without the library, and below 31 pixels on a side,
    where the package refuses the image.  The rules are at lpips_taps; the weights come from
    files, so parity with the reference's own output is unpinned."""
    if weights is None:
        return float("nan"), []
    a, b = _pair(img1, img2)
    if not lpips_defined(a.shape):
        return float("nan"), []
    return lpips_from_taps(lpips_taps(a, b, weights, dtype))


_ms_ssim = ms_ssim   # evaluate_pair's switch carries the function's name


def emd(img1, img2) -> Result:
    """Wasserstein-1 distance of the two globally normalised slices over H*W: for samples of
    equal size it is the mean absolute difference of the sorted samples."""
    a, b = _pair(img1, img2)
    gmin = min(a.min(), b.min())
    div = np.float32(max(a.max(), b.max()) - gmin) + EPS32
    vals = []
    for s1, s2 in zip(a, b):
        u = np.sort(((s1 - gmin) / div).ravel())
        v = np.sort(((s2 - gmin) / div).ravel())
        vals.append(float(np.mean(np.abs(u - v), dtype=np.float64) / s1.size))
    return float(np.mean(vals)), vals


def sobel(s: np.ndarray) -> np.ndarray:
    """skimage.filters.sobel of a 2-D image in float64."""
    x = s.astype(np.float64)
    smooth, edge = np.array([0.25, 0.5, 0.25]), np.array([1.0, 0.0, -1.0])
    h = correlate1d(correlate1d(x, edge, axis=0, mode="reflect"), smooth, axis=1, mode="reflect")
    v = correlate1d(correlate1d(x, edge, axis=1, mode="reflect"), smooth, axis=0, mode="reflect")
    return np.sqrt((h * h + v * v) / 2)


def ts_from_sums(sum_abs: float, max1: float, max2: float, n: int) -> float:
    m = max(max1, max2)
    return float(1.0 - (sum_abs / n) / m) if m > 0 else 1.0


def ts(img1, img2) -> Result:
    a, b = _pair(img1, img2)
    vals = []
    for s1, s2 in zip(a, b):
        g1, g2 = sobel(s1), sobel(s2)
        vals.append(ts_from_sums(float(np.sum(np.abs(g1 - g2), dtype=np.float64)), float(g1.max()), float(g2.max()),
                                 s1.size))
    return float(np.mean(vals)), vals


def cs_from_sums(sab, saa, sbb) -> float:
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.float64(sab) / (np.sqrt(np.float64(saa)) * np.sqrt(np.float64(sbb))))


def cs(img1, img2) -> Result:
    a, b = _pair(img1, img2)
    vals = []
    for s1, s2 in zip(a, b):
        x, y = s1.ravel().astype(np.float64), s2.ravel().astype(np.float64)
        vals.append(cs_from_sums(np.dot(x, y), np.dot(x, x), np.dot(y, y)))
    return float(np.mean(vals)), vals


def ed(img1, img2) -> Result:
    a, b = _pair(img1, img2)
    vals = []
    for s1, s2 in zip(a, b):
        n1 = (s1 - s1.min()) / (s1.max() - s1.min() + EPS32)
        n2 = (s2 - s2.min()) / (s2.max() - s2.min() + EPS32)
        d = (n1 - n2).astype(np.float64)
        vals.append(float(np.sqrt(np.sum(d * d, dtype=np.float64)) / s1.size))
    return float(np.mean(vals)), vals


def evaluate_pair(target, pred, advanced: bool = True, ms_ssim: bool = False, lpips_weights=None) -> Dict[str, Result]:
    """The basic metrics on the raw and the normalised volumes, and the advanced ones if asked;
    MS-SSIM is computed only with ``ms_ssim=True`` and LPIPS only with ``lpips_weights`` (loaded by
    modules/lpips_weights.py); each is ``(nan, [])`` otherwise."""
    ms = _ms_ssim if ms_ssim else lpips   # not asked for: empty, as lpips is
    t, p = _pair(target, pred)
    tn, pn = normalize(t), normalize(p)
    out = {"mae": mae(t, p), "psnr": psnr(t, p), "ssim": ssim(t, p),
           "mae_norm": mae(tn, pn), "psnr_norm": psnr(tn, pn), "ssim_norm": ssim(tn, pn)}
    if advanced:
        out.update({"ms_ssim": ms(tn, pn), "lpips": lpips(tn, pn, lpips_weights), "emd": emd(t, p), "ts": ts(t, p),
                    "cs": cs(t, p), "ed": ed(t, p)})
    return out


def pair_names(has_vue: bool) -> List[str]:
    return ["STD_vs_Generated"] + (["VUE_vs_STD", "VUE_vs_Generated"] if has_vue else [])


def collect_patient(pair_fn, std, gen, vue=None, ms_ssim: bool = False, lpips_weights=None):
    """The per-patient driver both paths share: the basic metrics for every pair, the advanced
    ones for STD against Generated; series are cut to the shortest.  ``pair_fn(target, pred,
    advanced)`` is evaluate_pair of the host or of the device module; with ``ms_ssim`` it is
    called with ``ms_ssim=True`` as well, with ``lpips_weights`` with those.  Returns (patient_metrics,
    csv_data): per metric the list of aggregates and the list of per-slice lists, one per pair."""
    n = min(len(v) for v in (std, gen, vue) if v is not None)
    std, gen = std[:n], gen[:n]
    pairs = [(std, gen, True)]
    if vue is not None:
        vue = vue[:n]
        pairs += [(vue, std, False), (vue, gen, False)]
    patient = {k: [] for k in METRICS}
    per_slice = {k: [] for k in METRICS}
    kw = {"ms_ssim": True} if ms_ssim else {}
    if lpips_weights is not None:
        kw["lpips_weights"] = lpips_weights
    for targ, pred, adv in pairs:
        for k, (agg, lst) in pair_fn(targ, pred, adv, **kw).items():
            patient[k].append(agg)
            per_slice[k].append(lst)
    return patient, per_slice


def evaluate_patient(std, gen, vue=None, ms_ssim: bool = False, lpips_weights=None):
    return collect_patient(evaluate_pair, std, gen, vue, ms_ssim, lpips_weights)


def detail_header(has_vue: bool) -> List[str]:
    names = pair_names(has_vue)
    return (["Slice_Idx"] + [f"{m}_{p}" for m in BASIC for p in names]
            + [f"{m}_STD_vs_Generated" for m in ADVANCED])


def detail_rows(csv_data: Dict[str, list], has_vue: bool) -> List[list]:
    npairs = len(pair_names(has_vue))
    rows = []
    for i in range(min(len(l) for l in csv_data["mae"])):
        row = [i]
        for m in BASIC:
            row += [csv_data[m][j][i] if j < len(csv_data[m]) else "" for j in range(npairs)]
        for m in ADVANCED:
            vals = csv_data[m]
            row.append(vals[0][i] if vals and i < len(vals[0]) else "")
        rows.append(row)
    return rows


def write_detail_csv(path: str, csv_data: Dict[str, list], has_vue: bool) -> None:
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(detail_header(has_vue))
        w.writerows(detail_rows(csv_data, has_vue))


# Region-wise evaluation (calculate.py --regions).  synthesis() hands every voxel to one owner by
# its NCCT value: the lung model where lung_min <= vue <= lung_max, the soft-tissue model where
# soft_min <= vue <= soft_max (lung wins where the ranges touch, as in synthesize), the NCCT
# itself elsewhere ("rest").  Over these lies the true enhancement, (std - vue) > thr and
# vue > min_hu with the float32 difference first and both comparisons strict, as
# synthesize_enhancement takes them; the predicted enhancement is the same with gen for std.
# Both paths produce the two float64 arrays below and region_from_sums derives every reported
# number from them.  The reference has no such metric.
REGIONS = ("lung", "soft", "rest", "enh")
REGION_VALUES = ("n", "mae", "bias", "psnr", "ssim")
ENH_VALUES = ("dice", "precision", "recall", "enh_true_mean", "enh_pred_mean")
REGION_COLUMNS = tuple(f"{v}_{r}" for r in REGIONS for v in REGION_VALUES) + tuple(f"{v}_enh" for v in ENH_VALUES)
REGION_NSUMS, REGION_NSSIM = 21, 8
# region_sums: columns 4 r + {RS_N, RS_ABS, RS_SQ, RS_BIAS} of region r, then the five below
RS_N, RS_ABS, RS_SQ, RS_BIAS = range(4)
RS_TP, RS_FP, RS_FN, RS_ENH_TRUE, RS_ENH_PRED = range(16, 21)


class RegionSpec(NamedTuple):
    """The HU ranges of the two models and the enhancement rule, generate.py's defaults."""
    lung_min: float = -1000.0
    lung_max: float = -150.0
    soft_min: float = -150.0
    soft_max: float = 250.0
    thr: float = 5.0
    min_hu: float = -400.0

    def ranges(self) -> Tuple[float, ...]:
        """(lung_min, lung_max, soft_min, soft_max, thr, min_hu) as the float32 values both paths compare with."""
        return tuple(float(np.float32(v)) for v in self)


def _triple(vue, std, gen):
    v, s = _pair(vue, std)
    s, g = _pair(std, gen)
    return v, s, g


def region_masks(vue, std, gen, spec: RegionSpec = RegionSpec()):
    """((lung, soft, rest, enh), pred): the membership of every voxel in float32; lung, soft and
    rest partition the volume, pred is the predicted enhancement mask."""
    v, s, g = _triple(vue, std, gen)
    lmin, lmax, smin, smax, thr, mh = (np.float32(x) for x in spec)
    lung = (v >= lmin) & (v <= lmax)
    soft = (v >= smin) & (v <= smax) & ~lung
    rest = ~(lung | soft)
    valid = v > mh
    return (lung, soft, rest, ((s - v) > thr) & valid), ((g - v) > thr) & valid


def region_sums(vue, std, gen, spec: RegionSpec = RegionSpec()) -> np.ndarray:
    """float64 [D,21]: per slice, for lung, soft, rest and enh in turn n, sum|std-gen|,
    sum (std-gen)^2, sum (gen-std); then TP, FP, FN of the predicted against the true enhancement
    mask; then sum (std-vue) and sum (gen-vue) over the true enhancement.  The differences and
    their squares are float32, every sum is float64, counts are exact."""
    v, s, g = _triple(vue, std, gen)
    masks, pred = region_masks(v, s, g, spec)
    d = s - g
    terms = (np.abs(d), d * d, g - s)
    et, ep = s - v, g - v
    f64 = lambda x: float(np.sum(x, dtype=np.float64))
    out = np.zeros((v.shape[0], REGION_NSUMS), dtype=np.float64)
    for z in range(v.shape[0]):
        for r, m in enumerate(masks):
            out[z, 4 * r: 4 * r + 4] = [np.count_nonzero(m[z])] + [f64(t[z][m[z]]) for t in terms]
        te, pe = masks[3][z], pred[z]
        out[z, RS_TP:] = [np.count_nonzero(te & pe), np.count_nonzero(~te & pe), np.count_nonzero(te & ~pe),
                          f64(et[z][te]), f64(ep[z][te])]
    return out


def region_ssim_sums(vue, std, gen, spec: RegionSpec = RegionSpec()) -> np.ndarray:
    """float64 [D,8]: per slice and region the number of its voxels inside the crop [3:H-3, 3:W-3]
    and the float64 sum over them of the map ssim_slice forms of (std, gen), data_range taken over
    the whole generated volume as ssim() takes it.  Zeros where a side is below 7."""
    v, s, g = _triple(vue, std, gen)
    out = np.zeros((v.shape[0], REGION_NSSIM), dtype=np.float64)
    if min(v.shape[1:]) < SSIM_WIN:
        return out
    masks, _ = region_masks(v, s, g, spec)
    data_range = float(g.max() - g.min())
    p = (SSIM_WIN - 1) // 2
    crop = lambda x: x[p:x.shape[0] - p, p:x.shape[1] - p]
    for z in range(v.shape[0]):
        smap = crop(ssim_map(s[z], g[z], data_range))
        for r, m in enumerate(masks):
            mz = crop(m[z])
            out[z, 2 * r: 2 * r + 2] = [np.count_nonzero(mz), float(np.sum(smap[mz], dtype=np.float64))]
    return out


def region_values(sums, ssim_sums, max_pixel: float) -> Dict[str, float]:
    """The reported values of one row of region_sums and of region_ssim_sums (a slice's, or the
    pooled sums of a volume), keyed by REGION_COLUMNS: per region n, mae, bias (mean of gen - std),
    psnr (psnr_from_mse with the whole-volume peak) and ssim; for enh also dice, precision, recall
    and the mean true and predicted enhancement.  nan where the denominator is 0."""
    nan = float("nan")
    div = lambda a, b: float(a / b) if b else nan
    out = {}
    for r, name in enumerate(REGIONS):
        n, sab, ssq, sbi = (float(x) for x in sums[4 * r: 4 * r + 4])
        out[f"n_{name}"] = int(n)
        out[f"mae_{name}"] = div(sab, n)
        out[f"bias_{name}"] = div(sbi, n)
        out[f"psnr_{name}"] = psnr_from_mse(ssq / n, (), max_pixel)[0] if n else nan
        out[f"ssim_{name}"] = div(float(ssim_sums[2 * r + 1]), float(ssim_sums[2 * r]))
    tp, fp, fn, st, sp = (float(x) for x in sums[RS_TP:])
    n_enh = float(sums[4 * REGIONS.index("enh") + RS_N])
    out["dice_enh"] = div(2 * tp, 2 * tp + fp + fn)
    out["precision_enh"] = div(tp, tp + fp)
    out["recall_enh"] = div(tp, tp + fn)
    out["enh_true_mean_enh"] = div(st, n_enh)
    out["enh_pred_mean_enh"] = div(sp, n_enh)
    return out


def region_from_sums(sums, ssim_sums, max_pixel: float):
    """(aggregate, per_slice) of both paths' raw arrays: per_slice maps every REGION_COLUMNS name
    to the list of slice values; the aggregate pools over the volume, the slice sums added in
    slice order in float64 before any division."""
    sums, ssim_sums = np.asarray(sums, dtype=np.float64), np.asarray(ssim_sums, dtype=np.float64)
    if sums.ndim != 2 or sums.shape[1] != REGION_NSUMS or ssim_sums.shape != (sums.shape[0], REGION_NSSIM):
        raise ValueError("region_from_sums: [D,21] and [D,8] arrays are required")
    rows = [region_values(a, b, max_pixel) for a, b in zip(sums, ssim_sums)]
    tot, stot = np.zeros(REGION_NSUMS), np.zeros(REGION_NSSIM)
    for a, b in zip(sums, ssim_sums):
        tot, stot = tot + a, stot + b
    return region_values(tot, stot, max_pixel), {k: [row[k] for row in rows] for k in REGION_COLUMNS}


def region_metrics(std, gen, vue, spec: RegionSpec = RegionSpec()):
    """The region-wise evaluation of one patient on the host: (aggregate, per_slice) of
    region_from_sums; the series are cut to the shortest, as evaluate_patient cuts them."""
    n = min(len(x) for x in (std, gen, vue))
    v, s, g = _triple(vue[:n], std[:n], gen[:n])
    return region_from_sums(region_sums(v, s, g, spec), region_ssim_sums(v, s, g, spec), max_pixel_of(s.min(), s.max()))


def region_header() -> List[str]:
    return ["Slice_Idx"] + list(REGION_COLUMNS)


def write_region_csv(path: str, per_slice: Dict[str, list]) -> None:
    """One row per slice; a value that is not defined (nan: an empty region) is an empty cell."""
    cell = lambda x: "" if isinstance(x, float) and np.isnan(x) else x
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(region_header())
        for i in range(len(per_slice[REGION_COLUMNS[0]])):
            w.writerow([i] + [cell(per_slice[k][i]) for k in REGION_COLUMNS])
