"""Region-wise evaluation on the host (modules/metrics.py::region_metrics, calculate.py --regions)
without a GPU: the two raw arrays against a voxel-by-voxel restatement written here, a slice whose
sums are worked out by hand, the partition property, a phantom series with empty regions, and the
command line (the files of a run without the flag do not change with it)."""
import csv
import functools
import math
import pickle

import numpy as np
import pytest

from modules import metrics as M
from modules import phantom

SPEC = M.RegionSpec()
NAN = float("nan")


def threshold_values(spec=SPEC):
    """HU values on and next to every threshold of the region rules."""
    on = [spec.lung_min, spec.lung_max, spec.soft_min, spec.soft_max, spec.min_hu]
    return sorted({v + d for v in on for d in (-1.0, 0.0, 1.0)})


@functools.lru_cache(maxsize=None)
def hu_triple(shape, seed=0, slope=1.0, round_noise=True):
    """Seeded (vue, std, gen): the NCCT is the recipe of tests/test_gpu_metrics.py::volumes (an air
    band at -1000, which the lung model owns, a body from N(40, 60), a +1500 block) plus voxels on
    and next to every threshold; std = vue + a rounded gain (N(60, 25) on a third of the voxels,
    N(0, 4) elsewhere, and exactly thr on some); gen = std + rounded N(0, 20), and vue itself on
    some voxels.  round_noise=False leaves the noise of gen unrounded, so that the sums round."""
    rng = np.random.default_rng([31, seed, *shape])
    d, h, w = shape
    v = np.round(rng.normal(40, 60, shape))
    v[:, : max(1, h // 4), :] = -1000
    v[:, h // 2: h // 2 + max(1, h // 5), w // 3: w // 3 + max(1, w // 4)] = 1500
    edge = threshold_values()
    flat = v.reshape(d, -1)
    for z in range(d):                                     # every threshold value in every slice
        pos = rng.choice(flat.shape[1], size=len(edge), replace=False)
        flat[z, pos] = edge
    gain = np.where(rng.uniform(size=shape) < 1 / 3, np.round(rng.normal(60, 25, shape)), np.round(rng.normal(0, 4, shape)))
    gain[rng.uniform(size=shape) < 0.05] = SPEC.thr        # a difference of exactly thr: excluded
    s = v + gain
    noise = rng.normal(0, 20, shape)
    g = s + (np.round(noise) if round_noise else noise)
    miss = rng.uniform(size=shape) < 0.08                  # no predicted gain at all: false negatives
    g[miss] = v[miss]
    out = tuple((x * slope).astype(np.float32) for x in (v, s, g))
    for x in out:
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def phantom_triple():
    """(vue, std, gen) [10,64,64]: the rounded phantom slices of seed 7 as the NCCT (chest, one lung,
    air, tiny lungs, threshold values; twice), a seeded gain of about +60 HU on soft tissue for
    the CECT, seeded noise on top for the generated series."""
    v = np.stack([np.round(phantom.slice_hu(7, i, 64)) for i in range(10)])
    rng = np.random.default_rng(77)
    soft = (v >= 0) & (v <= 250)
    s = v + np.where(soft, np.round(rng.normal(60, 10, v.shape)), 0.0)
    g = s + np.round(rng.normal(0, 15, v.shape))
    out = tuple(x.astype(np.float32) for x in (v, s, g))
    for x in out:
        x.setflags(write=False)
    return out


CHEST, AIR = (0, 4, 5, 9), (2, 7)


def restate_sums(vue, std, gen, spec=SPEC):
    """region_sums voxel by voxel: np.float32 scalars for the elementwise steps, Python ints and
    floats for the counts and sums."""
    f = np.float32
    lmin, lmax, smin, smax, thr, mh = (f(x) for x in spec)
    out = []
    for z in range(vue.shape[0]):
        n, sab, ssq, sbi = [0] * 4, [0.0] * 4, [0.0] * 4, [0.0] * 4
        tp = fp = fn = 0
        st = sp = 0.0
        for y in range(vue.shape[1]):
            for x in range(vue.shape[2]):
                v, s, g = f(vue[z, y, x]), f(std[z, y, x]), f(gen[z, y, x])
                if lmin <= v <= lmax:
                    owner = 0
                elif smin <= v <= smax:
                    owner = 1
                else:
                    owner = 2
                te = bool(f(s - v) > thr and v > mh)
                pe = bool(f(g - v) > thr and v > mh)
                d = f(s - g)
                for r in [owner] + ([3] if te else []):
                    n[r] += 1
                    sab[r] += float(abs(d))
                    ssq[r] += float(f(d * d))
                    sbi[r] += float(f(g - s))
                tp += te and pe
                fp += (not te) and pe
                fn += te and not pe
                if te:
                    st += float(f(s - v))
                    sp += float(f(g - v))
        row = []
        for r in range(4):
            row += [n[r], sab[r], ssq[r], sbi[r]]
        out.append(row + [tp, fp, fn, st, sp])
    return np.array(out, dtype=np.float64)


def ssim_pixel_direct(xp, yp, y, x, c1, c2):
    """The SSIM map at (y, x) from the symmetric-padded float64 slices: a direct 49-tap sum."""
    sx = sy = sxx = syy = sxy = 0.0
    for dy in range(7):
        for dx in range(7):
            a, b = float(xp[y + dy, x + dx]), float(yp[y + dy, x + dx])
            sx, sy, sxx, syy, sxy = sx + a, sy + b, sxx + a * a, syy + b * b, sxy + a * b
    ux, uy, uxx, uyy, uxy = sx / 49, sy / 49, sxx / 49, syy / 49, sxy / 49
    cn = 49 / 48
    vx, vy, vxy = cn * (uxx - ux * ux), cn * (uyy - uy * uy), cn * (uxy - ux * uy)
    return ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))


def restate_ssim_sums(vue, std, gen, spec=SPEC):
    """region_ssim_sums pixel by pixel, without ssim_slice: (count, sum of the direct map) per region
    over the crop [3:H-3, 3:W-3]."""
    f = np.float32
    lmin, lmax, smin, smax, thr, mh = (f(x) for x in spec)
    dr = float(gen.max() - gen.min())
    c1, c2 = (0.01 * dr) ** 2, (0.03 * dr) ** 2
    d, h, w = vue.shape
    out = np.zeros((d, 8))
    for z in range(d):
        xp = np.pad(std[z].astype(np.float64), 3, mode="symmetric")
        yp = np.pad(gen[z].astype(np.float64), 3, mode="symmetric")
        for y in range(3, h - 3):
            for x in range(3, w - 3):
                v, s = f(vue[z, y, x]), f(std[z, y, x])
                owner = 0 if lmin <= v <= lmax else (1 if smin <= v <= smax else 2)
                val = ssim_pixel_direct(xp, yp, y, x, c1, c2)
                for r in [owner] + ([3] if (f(s - v) > thr and v > mh) else []):
                    out[z, 2 * r] += 1
                    out[z, 2 * r + 1] += val
    return out


COUNT_COLS = [0, 4, 8, 12, 16, 17, 18]


@pytest.mark.parametrize("shape", [(3, 9, 11), (2, 7, 7)])
@pytest.mark.parametrize("slope", [1.0, 0.5])
def test_raw_arrays_against_a_voxel_loop(shape, slope):
    """Counts exact, sums relative 1e-12 (the data are multiples of 0.5, so every sum is exact in
    either order), SSIM absolute 1e-10 (two float64 orders of a 49-term mean)."""
    v, s, g = hu_triple(shape, 1, slope)
    spec = M.RegionSpec(*(x * slope for x in SPEC)) if slope != 1.0 else SPEC
    got, want = M.region_sums(v, s, g, spec), restate_sums(v, s, g, spec)
    assert got.shape == want.shape == (shape[0], M.REGION_NSUMS) and got.dtype == np.float64
    assert np.array_equal(got[:, COUNT_COLS], want[:, COUNT_COLS])
    assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want))
    if shape == (3, 9, 11):                                  # every region in every slice; TP, FP and FN occur
        assert want[:, [0, 4, 8, 12]].min() > 0 and want[:, 16:19].sum(axis=0).min() > 0
    gs, ws = M.region_ssim_sums(v, s, g, spec), restate_ssim_sums(v, s, g, spec)
    assert gs.shape == (shape[0], M.REGION_NSSIM)
    assert np.array_equal(gs[:, 0::2], ws[:, 0::2])
    assert gs[:, 0:6:2].sum(axis=1).tolist() == [(shape[1] - 6) * (shape[2] - 6)] * shape[0]
    cnt = np.maximum(ws[:, 0::2], 1)
    assert np.all(np.abs(gs[:, 1::2] - ws[:, 1::2]) / cnt <= 1e-10)


def test_hand_computed_voxels():
    """Eight voxels (vue, std, gen) on and around the thresholds; every sum is written out."""
    vox = [(-1000, -990, -992),     # lung (on lung_min); vue <= -400: no enhancement.  d = 2
           (-150, -100, -120),      # on lung_max and soft_min: lung wins; enh 50, pred 30: TP.  d = 20
           (250, 300, 252),         # soft (on soft_max); enh 50, pred 2: FN.  d = 48
           (251, 251, 260),         # rest; true 0, pred 9: FP.  d = -9
           (-400, -300, -300),      # lung; vue == min_hu is not above it: neither mask.  d = 0
           (0, 5, 5),               # soft; a gain of exactly thr is excluded from both masks.  d = 0
           (-1001, -1001, -1000),   # rest (below lung_min).  d = -1
           (40, 100.5, 90.25)]      # soft; enh 60.5, pred 50.25: TP.  d = 10.25
    v, s, g = (np.array([x[i] for x in vox], np.float32).reshape(1, 2, 4) for i in range(3))
    want = [3, 22.0, 404.0, -22.0,                       # lung: voxels 0, 1, 4
            3, 58.25, 2409.0625, -58.25,                 # soft: 2, 5, 7
            2, 10.0, 82.0, 10.0,                         # rest: 3, 6
            3, 78.25, 2809.0625, -78.25,                 # enh: 1, 2, 7
            2, 1, 1, 160.5, 82.25]                       # TP, FP, FN, sum (std-vue), sum (gen-vue) over enh
    assert M.region_sums(v, s, g).tolist() == [want]
    masks, pred = M.region_masks(v, s, g)
    assert [m.ravel().tolist() for m in masks] == [[True, True, False, False, True, False, False, False],
                                                   [False, False, True, False, False, True, False, True],
                                                   [False, False, False, True, False, False, True, False],
                                                   [False, True, True, False, False, False, False, True]]
    assert pred.ravel().tolist() == [False, True, False, True, False, False, False, True]
    assert np.array_equal(M.region_ssim_sums(v, s, g), np.zeros((1, 8)))          # a side below 7
    agg, per = M.region_metrics(s, g, v)
    assert list(per) == list(M.REGION_COLUMNS) and list(agg) == list(M.REGION_COLUMNS)
    peak = 300.0 - (-1001.0)
    for vals in (agg, {k: x[0] for k, x in per.items()}):
        assert (vals["n_lung"], vals["n_soft"], vals["n_rest"], vals["n_enh"]) == (3, 3, 2, 3)
        assert vals["mae_lung"] == 22 / 3 and vals["bias_lung"] == -22 / 3 and vals["mae_rest"] == 5.0
        assert vals["bias_rest"] == 5.0 and vals["mae_enh"] == 78.25 / 3
        assert vals["psnr_soft"] == pytest.approx(20 * math.log10(peak / math.sqrt(2409.0625 / 3)), rel=1e-15)
        assert vals["dice_enh"] == 4 / 6 and vals["precision_enh"] == 2 / 3 and vals["recall_enh"] == 2 / 3
        assert vals["enh_true_mean_enh"] == 53.5 and vals["enh_pred_mean_enh"] == 82.25 / 3
        assert all(math.isnan(vals[f"ssim_{r}"]) for r in M.REGIONS)


def test_empty_regions_and_zero_error():
    """No enhancement anywhere: nan for every enh value, Dice included; a region without error has
    an infinite PSNR, as psnr() gives."""
    v = np.full((2, 3, 3), 40.0, np.float32)
    agg, per = M.region_metrics(v, v, v)
    assert agg["n_soft"] == 18 and agg["mae_soft"] == 0.0 and agg["psnr_soft"] == math.inf
    for k in ("mae_enh", "bias_enh", "psnr_enh", "dice_enh", "precision_enh", "recall_enh", "enh_true_mean_enh",
              "mae_lung", "psnr_rest"):
        assert math.isnan(agg[k]) and all(math.isnan(x) for x in per[k])
    assert agg["n_enh"] == 0 and per["n_lung"] == [0, 0]


@pytest.mark.parametrize("shape", [(3, 9, 11), (2, 33, 65)])
def test_partition(shape):
    v, s, g = hu_triple(shape, 2)
    sums = M.region_sums(v, s, g)
    assert np.all(sums[:, 0] + sums[:, 4] + sums[:, 8] == shape[1] * shape[2])
    pooled = sums.sum(axis=0)
    mae, _ = M.mae(s, g)
    want = mae * v.size
    assert abs((pooled[1] + pooled[5] + pooled[9]) - want) <= 1e-12 * want
    ss = M.region_ssim_sums(v, s, g)
    assert np.all(ss[:, 0] + ss[:, 2] + ss[:, 4] == (shape[1] - 6) * (shape[2] - 6))
    _, slices = M.ssim(s, g)                               # the three owners' map sums add up to the slice's
    assert np.all(np.abs((ss[:, 1] + ss[:, 3] + ss[:, 5]) / ((shape[1] - 6) * (shape[2] - 6)) - slices) <= 1e-12)
    # the series are cut to the shortest, as evaluate_patient cuts them
    agg, per = M.region_metrics(s, g[:2], v)
    assert len(per["mae_lung"]) == 2 and agg == M.region_metrics(s[:2], g[:2], v[:2])[0]


def test_phantom_series(tmp_path):
    v, s, g = phantom_triple()
    sums = M.region_sums(v, s, g)
    assert sums[0, [0, 4, 8]].tolist() == [614, 1712, 1770]
    for z in CHEST:
        assert all(sums[z, 4 * r] > 0 for r in range(4)), z
    for z in AIR:
        assert sums[z, [0, 4, 8, 12]].tolist() == [0, 0, 4096, 0]
    agg, per = M.region_metrics(s, g, v)
    for z in AIR:
        for r in ("lung", "soft", "enh"):
            assert per[f"n_{r}"][z] == 0
            assert all(math.isnan(per[f"{k}_{r}"][z]) for k in ("mae", "bias", "psnr", "ssim"))
        assert all(math.isnan(per[f"{k}_enh"][z]) for k in M.ENH_VALUES)
        assert per["mae_rest"][z] > 0 and math.isfinite(per["ssim_rest"][z])
    for z in CHEST:
        assert all(math.isfinite(per[k][z]) for k in M.REGION_COLUMNS), z
    assert all(math.isfinite(agg[k]) for k in M.REGION_COLUMNS)
    # pooled over the volume: the sums of the slice sums over the sum of the counts
    assert agg["mae_soft"] == pytest.approx(sums[:, 5].sum() / sums[:, 4].sum(), rel=1e-15)
    assert 50 < agg["enh_true_mean_enh"] < 70 and agg["recall_enh"] > 0.9
    path = tmp_path / "p_regions.csv"
    M.write_region_csv(str(path), per)
    rows = list(csv.reader(open(path)))
    assert rows[0] == ["Slice_Idx"] + list(M.REGION_COLUMNS) and len(rows) == 11
    col = {name: i for i, name in enumerate(rows[0])}
    for z in AIR:
        r = rows[1 + z]
        assert r[col["mae_lung"]] == "" and r[col["ssim_soft"]] == "" and r[col["dice_enh"]] == ""
        assert r[col["n_lung"]] == "0" and r[col["n_rest"]] == "4096" and float(r[col["mae_rest"]]) == per["mae_rest"][z]
    assert float(rows[1][col["psnr_enh"]]) == per["psnr_enh"][0]


EXPECTED_HEADER = ["Slice_Idx"] + [f"{v}_{r}" for r in ("lung", "soft", "rest", "enh")
                                   for v in ("n", "mae", "bias", "psnr", "ssim")] + [
    "dice_enh", "precision_enh", "recall_enh", "enh_true_mean_enh", "enh_pred_mean_enh"]


def write_cli_tree(tmp_path, out_names=("out",)):
    """Two patients of three 16x16 slices under tmp_path/in/DS: P1 with VUE, STD and generated
    series, P2 without a VUE series; the generated series go under every tmp_path/<out>/DS."""
    from modules import dicom
    rng = np.random.default_rng(5)
    base = rng.integers(-1100, 400, (3, 16, 16))
    base[2] = rng.integers(-1030, -1010, (16, 16))          # an air slice: lung, soft and enh are empty
    std = base + np.where(rng.uniform(size=base.shape) < 0.4, rng.integers(20, 90, base.shape), 0)
    gen = std + rng.integers(-15, 15, base.shape)
    series = {"vue": base, "std": std, "generated": gen}
    for patient in ("P1", "P2"):
        dirs = {"vue": [tmp_path / "in" / "DS" / patient / "POST VUE"],
                "std": [tmp_path / "in" / "DS" / patient / "POST STD"],
                "generated": [tmp_path / o / "DS" / patient for o in out_names]}
        for cat, vol in series.items():
            if patient == "P2" and cat == "vue":
                continue
            for d in dirs[cat]:
                d.mkdir(parents=True)
                for i in range(3):
                    ds = dicom.new_ct_slice((vol[i] + 1024).astype(np.int16), instance=i + 1, uid_suffix=f"{i}")
                    ds.ImagePositionPatient = [0.0, 0.0, 2.5 * i]
                    ds.save_as(str(d / f"{i:03d}.dcm"))
    return {k: x.astype(np.float32) for k, x in series.items()}


def test_command_line(tmp_path):
    import calculate
    series = write_cli_tree(tmp_path, ("out_plain", "out_regions"))
    common = ["--input_dir_root", str(tmp_path / "in"), "--dataset_names", "DS"]
    calculate.main(common + ["--output_dir_root", str(tmp_path / "out_plain")])
    calculate.main(common + ["--output_dir_root", str(tmp_path / "out_regions"), "--regions"])
    plain, reg = tmp_path / "out_plain" / "calculated", tmp_path / "out_regions" / "calculated"
    assert np.array_equal(np.load(reg / "data" / "DS_P1_vue.npy"), series["vue"])
    old = ["detail/DS_P1_metrics.csv", "detail/DS_P2_metrics.csv", "result_all_metrics.pkl", "summary_statistics.csv"]
    for name in old:
        assert (plain / name).read_bytes() == (reg / name).read_bytes(), name
    names = lambda root: sorted(str(p.relative_to(root)) for p in root.rglob("*") if p.is_file())
    assert not (plain / "regions").exists()
    new = ["regions/DS_P1_regions.csv", "result_region_metrics.pkl", "summary_statistics_regions.csv"]
    assert sorted(set(names(reg)) - set(names(plain))) == sorted(new)       # P2 has no VUE: no region CSV
    assert set(names(plain)) <= set(names(reg))
    rows = list(csv.reader(open(reg / "regions" / "DS_P1_regions.csv")))
    assert rows[0] == EXPECTED_HEADER and [r[0] for r in rows[1:]] == ["0", "1", "2"]
    agg, per = M.region_metrics(series["std"], series["generated"], series["vue"])
    for i, r in enumerate(rows[1:]):
        for name, cell in zip(rows[0][1:], r[1:]):
            want = per[name][i]
            assert cell == ("" if isinstance(want, float) and math.isnan(want) else str(want)), (name, i)
    summary = pickle.load(open(reg / "result_region_metrics.pkl", "rb"))
    assert summary["patient"] == ["DS_P1"] and set(summary) == {"patient", *M.REGION_COLUMNS}
    assert all(summary[k] == [agg[k]] or (math.isnan(agg[k]) and math.isnan(summary[k][0])) for k in M.REGION_COLUMNS)
    stats = list(csv.DictReader(open(reg / "summary_statistics_regions.csv")))
    finite = [k for k in M.REGION_COLUMNS if any(math.isfinite(x) for x in per[k])]
    assert [s["Metric"] for s in stats] == finite and "ssim_lung" in finite
    assert set(stats[0]) == {"Metric", "Mean", "Std", "Min", "Max", "Median", "Count"}


def test_command_line_flags_and_other_ranges(tmp_path):
    """The flags carry generate.py's names and defaults; other ranges move the voxels."""
    import calculate
    a = calculate.get_args([])
    assert not a.regions
    assert (a.lung_hu_min, a.lung_hu_max, a.soft_hu_min, a.soft_hu_max) == (-1000, -150, -150, 250)
    assert (a.enhancement_threshold, a.enhancement_min_hu) == (5.0, -400.0)
    series = write_cli_tree(tmp_path)
    calculate.main(["--input_dir_root", str(tmp_path / "in"), "--dataset_names", "DS", "--output_dir_root",
                    str(tmp_path / "out"), "--regions", "--lung_hu_min", "-2000", "--lung_hu_max", "3000",
                    "--enhancement_threshold", "50"])
    rows = list(csv.DictReader(open(tmp_path / "out" / "calculated" / "regions" / "DS_P1_regions.csv")))
    spec = M.RegionSpec(lung_min=-2000, lung_max=3000, thr=50.0)
    _, per = M.region_metrics(series["std"], series["generated"], series["vue"], spec)
    for i, r in enumerate(rows):
        assert r["n_lung"] == "256" and r["n_soft"] == r["n_rest"] == "0" and r["mae_soft"] == ""
        assert int(r["n_enh"]) == per["n_enh"][i] and float(r["ssim_lung"]) == per["ssim_lung"][i]
    assert per["n_enh"][0] > 0 and per["n_enh"][1] > 0 and per["n_enh"][2] == 0
