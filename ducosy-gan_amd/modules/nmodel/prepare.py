"""Training targets of the normal-map U-Net from a voxel-aligned NCCT / CECT pair.

The definition of the target is this project's own, not the reference's.  The reference ships the
U-Net, its trainer and the stage that applies its output, but neither a recipe for nor a program
that writes ``vue_files/`` and ``diff_map/``; its README says only that the stage "analyses the
difference between the original and the generated image to emphasise the contrast effect".  What
its code fixes: ``synthesis()`` adds the predicted map to the merged volume before the smoothing,
``apply_diffmap`` drops values below 8, and ``CTDiffDataset.normalize_diff`` clips the target to
[0, 4000].  So the target is defined here as

    real CECT - merged sCECT before the smoothing,

in the units ``apply_diffmap`` adds (stored values of the NCCT series, HU when the slope is 1).
Parity with the reference is not applicable.  ``POST VUE`` and ``POST STD`` are reconstructions of
one acquisition, so the pair is taken as voxel-aligned; nothing here registers.

``residual_targets`` is the host statement of csrc/nmodel_data.hip (modules/hip/nmodel_data.py):
float32, one rounding per step, so both give the same bits.
"""
from __future__ import annotations

import numpy as np

from .dataset import DIFF_RANGE

NSTATS = 11
N, N_APPLY, N_NEG, N_OVER, SUM_CLIP, SUM_ABS, SUM_X, SUM_Y, SUM_XX, SUM_YY, SUM_XY = range(NSTATS)
STAT_NAMES = ("n", "n_apply", "n_neg", "n_over", "sum_clip", "sum_abs", "sum_x", "sum_y", "sum_xx", "sum_yy", "sum_xy")
COUNT_COLS = (N, N_APPLY, N_NEG, N_OVER)
# a variance below this share of n * sum v^2 is rounding of the float64 sums, not spread: float32
# data cannot vary by less than 6e-8 of its magnitude
ZERO_VARIANCE = 1e-12


def _series(stored, slopes, intercepts, name):
    a = np.asarray(stored)
    if a.dtype not in (np.int16, np.uint16):
        raise TypeError(f"residual_targets: {name}: stored dtype {a.dtype} (int16 or uint16 expected)")
    if a.ndim != 3 or a.size == 0:
        raise ValueError(f"residual_targets: {name}: non-empty [D,H,W] series required")
    s = np.asarray(slopes, dtype=np.float64).astype(np.float32).reshape(-1)
    i = np.asarray(intercepts, dtype=np.float64).astype(np.float32).reshape(-1)
    if s.size != a.shape[0] or i.size != a.shape[0]:
        raise ValueError(f"residual_targets: {name}: one slope / intercept per slice")
    return a, s[:, None, None], i[:, None, None]


def residual_targets(ncct_stored, ncct_slopes, ncct_intercepts, cect_stored, cect_slopes, cect_intercepts,
                     merged=None, threshold=8.0):
    """(vue, diff, stats) of one patient.

    ncct_stored, cect_stored: [D,H,W] stored values, int16 or uint16 independently; one rescale pair
    per slice and series, cast to float32 first (as ``hu_from_stored`` and ``synthesize_enhancement``
    do).  merged: the merged sCECT before the smoothing as float32 [D,H,W] in stored-value units of
    the NCCT series (``translate_volume_device`` returns it), or None.  Per voxel in float32, one
    rounding per step:

        x = f32(ncct) * sn + in     vue: the NCCT in HU, what CTDiffDataset.normalize_hu expects
        y = f32(cect) * sc + ic     the CECT in HU, with its own rescale pair
        g = merged * sn + in        g = x with merged=None: the plain enhancement CECT - NCCT
        diff = (y - g) / sn         stored-value units of the NCCT series: what apply_diffmap adds

    stats: float64 [D, 11] per slice: n, n_apply (diff >= threshold), n_neg (diff < 0), n_over
    (diff > 4000), sum clip(diff, 0, 4000), sum |diff|, sum x, sum y, sum x^2, sum y^2, sum xy, the
    last five with x and y widened to float64 before multiplying (``pearson_from_sums`` reads them).
    A shape mismatch raises ValueError."""
    f = np.float32
    n, sn, in_ = _series(ncct_stored, ncct_slopes, ncct_intercepts, "ncct")
    c, sc, ic = _series(cect_stored, cect_slopes, cect_intercepts, "cect")
    if n.shape != c.shape:
        raise ValueError(f"residual_targets: the series differ in shape: ncct {n.shape}, cect {c.shape}")
    if not np.all(np.isfinite(sn)) or np.any(sn == 0):
        raise ValueError("residual_targets: the NCCT slopes must be finite and not zero")
    x = n.astype(f) * sn + in_
    y = c.astype(f) * sc + ic
    if merged is None:
        g = x
    else:
        m = np.asarray(merged)
        if m.shape != n.shape:
            raise ValueError(f"residual_targets: merged {m.shape} differs in shape from the series {n.shape}")
        g = m.astype(f, copy=False) * sn + in_
    diff = (y - g) / sn
    assert x.dtype == f and diff.dtype == f
    D = n.shape[0]
    lo, hi = f(DIFF_RANGE[0]), f(DIFF_RANGE[1])
    stats = np.zeros((D, NSTATS), np.float64)
    sums = lambda a: a.reshape(D, -1).astype(np.float64).sum(axis=1)
    stats[:, N] = n.shape[1] * n.shape[2]
    stats[:, N_APPLY] = (diff >= f(threshold)).reshape(D, -1).sum(axis=1)
    stats[:, N_NEG] = (diff < 0).reshape(D, -1).sum(axis=1)
    stats[:, N_OVER] = (diff > hi).reshape(D, -1).sum(axis=1)
    stats[:, SUM_CLIP] = sums(np.clip(diff, lo, hi))
    stats[:, SUM_ABS] = sums(np.abs(diff))
    x64, y64 = x.reshape(D, -1).astype(np.float64), y.reshape(D, -1).astype(np.float64)
    stats[:, SUM_X], stats[:, SUM_Y] = x64.sum(axis=1), y64.sum(axis=1)
    stats[:, SUM_XX], stats[:, SUM_YY], stats[:, SUM_XY] = (x64 * x64).sum(axis=1), (y64 * y64).sum(axis=1), (x64 * y64).sum(axis=1)
    return x, diff, stats


def pearson_from_sums(stats_rows):
    """Pearson correlation of NCCT against CECT from rows of ``stats`` ([..., 11] -> [...]):
    (n Sxy - Sx Sy) / sqrt((n Sxx - Sx^2) (n Syy - Sy^2)) in float64.  A row without variance in
    either series (a constant slice) has no correlation: NaN, which the builder writes as an empty
    cell.  The correlation of a whole volume is that of its summed rows."""
    r = np.asarray(stats_rows, dtype=np.float64)
    n, sx, sy, sxx, syy, sxy = (r[..., k] for k in (N, SUM_X, SUM_Y, SUM_XX, SUM_YY, SUM_XY))
    vx, vy = n * sxx - sx * sx, n * syy - sy * sy
    ok = (vx > ZERO_VARIANCE * n * sxx) & (vy > ZERO_VARIANCE * n * syy)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = (n * sxy - sx * sy) / np.sqrt(np.where(ok, vx * vy, np.nan))
    return np.where(ok, out, np.nan)


def volume_summary(stats):
    """The volume totals a manifest row holds, from the per-slice ``stats``: the four counts, the
    mean of the clipped target, the share of voxels at or above the threshold, the correlation."""
    tot = np.asarray(stats, dtype=np.float64).sum(axis=0)
    out = {STAT_NAMES[k]: int(tot[k]) for k in COUNT_COLS}
    out["mean_clipped"] = float(tot[SUM_CLIP] / tot[N])
    out["share_apply"] = float(tot[N_APPLY] / tot[N])
    out["corr"] = float(pearson_from_sums(tot))
    return out
