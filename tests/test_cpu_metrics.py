"""Host path of the evaluation metrics (modules/metrics.py, calculate.py) without a GPU: every
metric against a literal numpy / scipy restatement of the reference formula written here, the
branches (inf, constant inputs, the SSIM window error), and the detail CSV layout."""
import csv
import math

import numpy as np
import pytest
import scipy.ndimage as ndi
from scipy.stats import wasserstein_distance

from modules import metrics as M

SHAPES = [(1, 7, 7), (2, 8, 70), (3, 33, 65), (2, 70, 300)]


def hu_pair(shape, seed=0, slope=1.0):
    """Seeded HU-like integer volumes: an air band at -1000, a body from N(40, 60), a +1500 block;
    the prediction is the target plus rounded N(0, 20)."""
    rng = np.random.default_rng([seed, *shape])
    d, h, w = shape
    t = np.round(rng.normal(40, 60, shape))
    t[:, : max(1, h // 4), :] = -1000
    t[:, h // 2: h // 2 + max(1, h // 5), w // 3: w // 3 + max(1, w // 4)] = 1500
    p = t + np.round(rng.normal(0, 20, shape))
    return (t * slope).astype(np.float32), (p * slope).astype(np.float32)


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


# Literal float32 restatements of the reference formulas.  Bar: relative 1e-5; float32 pairwise
# summation of <= 1e5 non-negative terms errs by at most about log2(N) * 2^-24 ~ 1e-6.
RTOL = 1e-5


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("slope", [1.0, 0.5])
def test_against_float32_restatements(shape, slope):
    a, b = hu_pair(shape, 1, slope)
    # mae
    diff = np.abs(a - b)
    agg, lst = M.mae(a, b)
    assert rel(agg, np.mean(diff)) <= RTOL
    assert all(rel(x, np.mean(s)) <= RTOL for x, s in zip(lst, diff))
    # psnr
    mse = np.mean((a - b) ** 2)
    mp = a.max() - a.min()
    agg, lst = M.psnr(a, b)
    assert rel(agg, 20 * np.log10(mp / np.sqrt(mse))) <= RTOL
    for x, s1, s2 in zip(lst, a, b):
        assert rel(x, 20 * np.log10(mp / np.sqrt(np.mean((s1 - s2) ** 2)))) <= RTOL
    # emd
    gmin, gmax = min(a.min(), b.min()), max(a.max(), b.max())
    agg, lst = M.emd(a, b)
    want = []
    for s1, s2 in zip(a, b):
        n1 = (s1 - gmin) / (gmax - gmin + 1e-8)
        n2 = (s2 - gmin) / (gmax - gmin + 1e-8)
        want.append(wasserstein_distance(n1.flatten(), n2.flatten()) / np.prod(s1.shape))
    assert all(rel(x, w) <= RTOL for x, w in zip(lst, want))
    assert rel(agg, np.mean(want)) <= RTOL
    # cs
    agg, lst = M.cs(a, b)
    for x, s1, s2 in zip(lst, a, b):
        v1, v2 = s1.flatten(), s2.flatten()
        assert rel(x, np.dot(v1, v2) / (np.linalg.norm(v1) * np.linalg.norm(v2))) <= RTOL
    # ed
    agg, lst = M.ed(a, b)
    for x, s1, s2 in zip(lst, a, b):
        n1 = (s1 - s1.min()) / (s1.max() - s1.min() + 1e-8)
        n2 = (s2 - s2.min()) / (s2.max() - s2.min() + 1e-8)
        assert rel(x, np.linalg.norm(n1 - n2) / np.prod(n1.shape)) <= RTOL
    # normalize
    n = M.normalize(a)
    assert n.dtype == np.float32 and np.array_equal(n, (a - a.min()) / (a.max() - a.min()))


def ssim_direct(s1, s2, data_range):
    """structural_similarity restated independently: symmetric padding and a direct 49-term sum."""
    x, y = np.pad(s1.astype(np.float64), 3, mode="symmetric"), np.pad(s2.astype(np.float64), 3, mode="symmetric")
    h, w = s1.shape

    def mean49(v):
        acc = np.zeros((h, w))
        for dy in range(7):
            for dx in range(7):
                acc += v[dy:dy + h, dx:dx + w]
        return acc / 49

    ux, uy, uxx, uyy, uxy = mean49(x), mean49(y), mean49(x * x), mean49(y * y), mean49(x * y)
    cn = 49 / 48
    vx, vy, vxy = cn * (uxx - ux * ux), cn * (uyy - uy * uy), cn * (uxy - ux * uy)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux ** 2 + uy ** 2 + c1) * (vx + vy + c2))
    return s[3:h - 3, 3:w - 3].mean()


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("norm", [False, True])
def test_ssim_against_direct_sum(shape, norm):
    """Bar: absolute 1e-10 (the two host summation orders were measured to differ by <= 2.3e-14)."""
    a, b = hu_pair(shape, 2)
    if norm:
        a, b = M.normalize(a), M.normalize(b)
    agg, lst = M.ssim(a, b)
    dr = float(b.max() - b.min())
    want = [ssim_direct(s1, s2, dr) for s1, s2 in zip(a, b)]
    assert len(lst) == shape[0]
    assert max(abs(x - w) for x, w in zip(lst, want)) <= 1e-10
    assert abs(agg - np.mean(want)) <= 1e-10


@pytest.mark.parametrize("shape", SHAPES)
def test_sobel_against_scipy(shape):
    a, _ = hu_pair(shape, 3, 0.5)
    for s in a:
        x = s.astype(np.float64)
        h, v = ndi.sobel(x, axis=0, mode="reflect") / 4, ndi.sobel(x, axis=1, mode="reflect") / 4
        want = np.sqrt((h ** 2 + v ** 2) / 2)
        got = M.sobel(s)
        assert np.max(np.abs(got - want)) <= 1e-12 * max(1.0, want.max())


def test_ts_formula():
    a, b = hu_pair((2, 20, 31), 4)
    agg, lst = M.ts(a, b)
    for x, s1, s2 in zip(lst, a, b):
        g1, g2 = M.sobel(s1), M.sobel(s2)
        assert rel(x, 1.0 - np.mean(np.abs(g1 - g2)) / max(g1.max(), g2.max())) <= 1e-12
    assert rel(agg, np.mean(lst)) <= 1e-15


def test_psnr_branches():
    a, b = hu_pair((3, 9, 11), 5)
    agg, lst = M.psnr(a, a)
    assert agg == math.inf and lst == [math.inf] * 3
    b2 = b.copy()
    b2[1] = a[1]
    agg, lst = M.psnr(a, b2)
    assert math.isfinite(agg) and lst[1] == math.inf and math.isfinite(lst[0]) and math.isfinite(lst[2])
    const = np.full((2, 8, 8), 7.0, np.float32)
    other = const + 2
    agg, lst = M.psnr(const, other)          # max_pixel 1.0: 20 log10(1 / 2)
    assert rel(agg, 20 * math.log10(0.5)) <= 1e-15 and all(rel(x, agg) <= 1e-15 for x in lst)


def test_constant_slices_and_normalize_of_a_constant():
    a, b = hu_pair((3, 9, 11), 6)
    a[1], b[1] = 5.0, -3.0
    _, e = M.ed(a, b)
    assert e[1] == 0.0 and e[0] > 0
    _, t = M.ts(a, b)
    assert t[1] == 1.0 and 0 < t[0] < 1
    assert np.array_equal(M.normalize(np.full((2, 3, 4), 9.0, np.float32)), np.zeros((2, 3, 4), np.float32))


def test_ssim_window_error_and_absent_metrics():
    a = np.zeros((2, 6, 20), np.float32)
    with pytest.raises(ValueError):
        M.ssim(a, a)
    with pytest.raises(ValueError):
        M.ssim(a.transpose(0, 2, 1), a.transpose(0, 2, 1))
    for fn in (M.ms_ssim, M.lpips):
        agg, lst = fn(a, a)
        assert math.isnan(agg) and lst == []


def reference_header(has_vue):
    """The header rule of the reference's process_single_patient."""
    pairs = ["STD_vs_Generated"] + (["VUE_vs_STD", "VUE_vs_Generated"] if has_vue else [])
    header = ["Slice_Idx"]
    for metric in ["mae", "psnr", "ssim", "mae_norm", "psnr_norm", "ssim_norm"]:
        for pname in pairs:
            header.append(f"{metric}_{pname}")
    for metric in ["ms_ssim", "lpips", "emd", "ts", "cs", "ed"]:
        header.append(f"{metric}_STD_vs_Generated")
    return header


@pytest.mark.parametrize("has_vue", [False, True])
def test_detail_csv_layout(tmp_path, has_vue):
    std, gen = hu_pair((2, 8, 9), 7)
    vue = hu_pair((3, 8, 9), 8)[0] if has_vue else None      # one slice more: cut to the shortest
    patient, per_slice = M.evaluate_patient(std, gen, vue)
    npairs = 3 if has_vue else 1
    assert set(patient) == set(M.METRICS)
    for k in M.BASIC:
        assert len(patient[k]) == npairs and [len(l) for l in per_slice[k]] == [2] * npairs
    for k in M.ADVANCED:
        assert len(patient[k]) == 1
    path = tmp_path / "p_metrics.csv"
    M.write_detail_csv(str(path), per_slice, has_vue)
    rows = list(csv.reader(open(path)))
    assert rows[0] == reference_header(has_vue)
    assert len(rows) == 3 and [r[0] for r in rows[1:]] == ["0", "1"]
    col = {name: i for i, name in enumerate(rows[0])}
    for i, r in enumerate(rows[1:]):
        assert len(r) == len(rows[0])
        assert r[col["ms_ssim_STD_vs_Generated"]] == "" and r[col["lpips_STD_vs_Generated"]] == ""
        assert float(r[col["mae_STD_vs_Generated"]]) == per_slice["mae"][0][i]
        assert float(r[col["ed_STD_vs_Generated"]]) == per_slice["ed"][0][i]
        if has_vue:
            assert float(r[col["ssim_norm_VUE_vs_Generated"]]) == per_slice["ssim_norm"][2][i]
            assert float(r[col["psnr_VUE_vs_STD"]]) == per_slice["psnr"][1][i]
    # the pair order of the reference: target / prediction of every pair
    want = M.evaluate_pair(std, gen)
    assert patient["mae"][0] == want["mae"][0] and patient["cs"][0] == want["cs"][0]
    if has_vue:
        assert patient["mae"][1] == M.mae(vue[:2], std)[0] and patient["mae"][2] == M.mae(vue[:2], gen)[0]


def test_calculate_arguments_have_no_side_effects(tmp_path, monkeypatch):
    """The reference's flags plus --device; parsing creates no directory and sets no variable."""
    import calculate
    monkeypatch.chdir(tmp_path)
    before = dict(__import__("os").environ)
    a = calculate.get_args([])
    assert a.device == "cpu" and a.ncct_folder == "POST VUE" and a.cect_folder == "POST STD" and a.num_workers == 1
    assert calculate.get_args(["--device", "cuda", "--mask", "--reset", "--skip_convert"]).device == "cuda"
    with pytest.raises(SystemExit):
        calculate.get_args(["--device", "tpu"])
    assert list(tmp_path.iterdir()) == [] and dict(__import__("os").environ) == before


def test_calculate_end_to_end_on_the_host(tmp_path):
    """A three-series patient with shuffled z positions through calculate.py on the host."""
    import calculate
    from modules import dicom
    rng = np.random.default_rng(11)
    base = rng.integers(900, 1200, (3, 16, 16)).astype(np.int16)
    series = {"vue": base, "std": (base + rng.integers(0, 60, base.shape)).astype(np.int16),
              "generated": (base + rng.integers(0, 60, base.shape)).astype(np.int16)}
    dirs = {"vue": tmp_path / "in" / "DS" / "P1" / "POST VUE", "std": tmp_path / "in" / "DS" / "P1" / "POST STD",
            "generated": tmp_path / "out" / "DS" / "P1"}
    order = [2, 0, 1]                                       # file order differs from z order
    for cat, vol in series.items():
        dirs[cat].mkdir(parents=True)
        for fi, zi in enumerate(order):
            ds = dicom.new_ct_slice(vol[zi], instance=fi + 1, uid_suffix=f"{fi}")
            ds.ImagePositionPatient = [0.0, 0.0, 2.5 * zi]
            ds.save_as(str(dirs[cat] / f"{fi:03d}.dcm"))
    calculate.main(["--input_dir_root", str(tmp_path / "in"), "--output_dir_root", str(tmp_path / "out"),
                    "--dataset_names", "DS"])
    calc = tmp_path / "out" / "calculated"
    for cat, vol in series.items():
        got = np.load(calc / "data" / f"DS_P1_{cat}.npy")
        assert got.dtype == np.float32 and np.array_equal(got, vol.astype(np.float32) - 1024)
    rows = list(csv.reader(open(calc / "detail" / "DS_P1_metrics.csv")))
    assert rows[0] == reference_header(True) and len(rows) == 4
    import pickle
    summary = pickle.load(open(calc / "result_all_metrics.pkl", "rb"))
    assert set(summary) == set(M.METRICS) and len(summary["mae"]) == 1 and len(summary["mae"][0]) == 3
    stats = list(csv.DictReader(open(calc / "summary_statistics.csv")))
    assert stats and set(stats[0]) == {"Metric", "Mean", "Std", "Min", "Max", "Median", "Count"}
    assert not any(s["Metric"].startswith(("ms_ssim", "lpips")) for s in stats)
