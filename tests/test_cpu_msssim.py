"""MS-SSIM on the host (modules/metrics.py::ms_ssim and calculate.py --ms_ssim), no GPU.

The level means are compared with an independent float64 formula written here: a direct 2-D
correlation with the 121-tap window np.outer(g, g) over sliding_window_view.  Both sum 121
products of magnitude <= 1 in float64 in different orders, so they agree to a few 1e-16 per
filtered value; 1e-12 on the means is the bar.
"""
import csv
import functools
import math
import pickle

import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

from modules import metrics as M

SHAPES = [(2, 176, 176), (2, 177, 243)]


@functools.lru_cache(maxsize=None)
def volumes(shape):
    """Seeded HU-like integer volumes (the generator of tests/test_gpu_metrics.py): an air band at
    -1000, a body from N(40, 60), a +1500 block; the prediction is the target plus rounded N(0, 20)."""
    rng = np.random.default_rng([17, *shape])
    d, h, w = shape
    t = np.round(rng.normal(40, 60, shape))
    t[:, : max(1, h // 4), :] = -1000
    t[:, h // 2: h // 2 + max(1, h // 5), w // 3: w // 3 + max(1, w // 4)] = 1500
    p = t + np.round(rng.normal(0, 20, shape))
    t, p = t.astype(np.float32), p.astype(np.float32)
    t.setflags(write=False)
    p.setflags(write=False)
    return t, p


def anti_pair(shape=(2, 176, 176)):
    t = np.random.default_rng(5).random(shape, dtype=np.float32)
    return t, (np.float32(1) - t)


def direct_levels(a, b):
    """[5][D][2] (sim, cs) means from the definition, in float64."""
    g = np.exp(-((np.arange(11) - 5) / 1.5) ** 2 / 2)
    g /= g.sum()
    win = np.outer(g, g)
    renorm = lambda v: (v - v.min()) / ((v.max() - v.min()) + np.float32(1e-8))
    x, y = renorm(a), renorm(b)
    assert x.dtype == y.dtype == np.float32
    filt = lambda v: np.einsum("dhwij,ij->dhw", sliding_window_view(v, (11, 11), axis=(1, 2)), win)
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    out, shapes = [], []
    for level in range(5):
        shapes.append(x.shape[1:])
        X, Y = x.astype(np.float64), y.astype(np.float64)
        ux, uy = filt(X), filt(Y)
        sxx, syy, sxy = filt(X * X) - ux * ux, filt(Y * Y) - uy * uy, filt(X * Y) - ux * uy
        cs = (2 * sxy + c2) / (sxx + syy + c2)
        sim = ((2 * ux * uy + c1) * (2 * sxy + c2)) / ((ux ** 2 + uy ** 2 + c1) * (sxx + syy + c2))
        assert sim.shape[1:] == (x.shape[1] - 10, x.shape[2] - 10)
        out.append(np.stack([sim.mean(axis=(1, 2)), cs.mean(axis=(1, 2))], axis=1))
        if level < 4:
            h, w = x.shape[1] // 2 * 2, x.shape[2] // 2 * 2
            # the pooling rule fixes the order of the four-term sum, so it is followed here
            q = lambda v: v[:, :h, :w].astype(np.float64).reshape(v.shape[0], h // 2, 2, w // 2, 2)
            pool = lambda v: ((((q(v)[:, :, 0, :, 0] + q(v)[:, :, 0, :, 1]) + q(v)[:, :, 1, :, 0]) + q(v)[:, :, 1, :, 1])
                              * 0.25).astype(np.float32)
            x, y = pool(x), pool(y)
    return np.array(out), shapes


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_levels_against_the_direct_formula(shape):
    t, p = volumes(shape)
    want, _ = direct_levels(t, p)
    got = M.ms_ssim_levels(t, p)
    assert got.shape == want.shape == (5, shape[0], 2) and got.dtype == np.float64
    err = np.abs(got - want).max()
    print("max abs error of the level means", err)
    assert err <= 1e-12
    # the final values follow from the level means
    lv = np.maximum(want, 0)
    final = np.prod(lv[:4, :, 1] ** np.array(M.MS_SSIM_BETAS[:4])[:, None], axis=0) * lv[4, :, 0] ** M.MS_SSIM_BETAS[4]
    vals = M.ms_ssim_slices(t, p)
    assert np.abs(np.array(vals) - final).max() <= 1e-12
    agg, lst = M.ms_ssim(t, p)
    assert agg == float(np.mean(vals)) and lst == [agg] * shape[0] and 0 < agg < 1


def test_window_and_constants():
    g = M.MS_SSIM_WINDOW
    assert g.dtype == np.float64 and g.shape == (11,) and abs(g.sum() - 1) <= 1e-15
    assert np.array_equal(g, g[::-1]) and g.argmax() == 5
    assert M.MS_SSIM_BETAS == (0.0448, 0.2856, 0.3001, 0.2363, 0.1333) and M.MS_SSIM_MIN_SIDE == 176


def test_pyramid_shapes_follow_the_floor_rule():
    t, p = volumes((2, 177, 243))
    levels = M.ms_ssim_pyramid(t, p)
    assert [x.shape[1:] for x, _ in levels] == [(177, 243), (88, 121), (44, 60), (22, 30), (11, 15)]
    assert all(x.dtype == y.dtype == np.float32 and x.shape == y.shape for x, y in levels)
    assert direct_levels(t, p)[1] == [x.shape[1:] for x, _ in levels]
    # one pooled sample by the rule: float32((((a + b) + c) + d) * 0.25), the sum in float64
    x0, x1 = levels[0][0], levels[1][0]
    q = x0[1, 174:176, 240:242].astype(np.float64)
    assert x1[1, 87, 120] == np.float32((((q[0, 0] + q[0, 1]) + q[1, 0]) + q[1, 1]) * 0.25)
    # the last level of a 176 x 176 slice is one window
    last = M.ms_ssim_pyramid(*volumes((2, 176, 176)))[-1][0]
    assert last.shape == (2, 11, 11)


def test_identical_volumes_give_exactly_one():
    t, _ = volumes((2, 176, 176))
    assert M.ms_ssim(t, t) == (1.0, [1.0, 1.0])
    assert M.ms_ssim_slices(t, t) == [1.0, 1.0]


def test_anticorrelated_pair_is_clamped_to_zero():
    t, p = anti_pair()
    levels = M.ms_ssim_levels(t, p)
    assert levels[:, :, 1].min() < -0.05          # the clamp really ran
    assert M.ms_ssim_slices(t, p) == [0.0, 0.0]
    assert M.ms_ssim(t, p) == (0.0, [0.0, 0.0])


@pytest.mark.parametrize("shape", [(2, 175, 300), (2, 300, 175)])
def test_too_small_gives_nan(shape):
    a = np.random.default_rng(1).random(shape, dtype=np.float32)
    agg, lst = M.ms_ssim(a, a)
    assert math.isnan(agg) and lst == []
    assert M.ms_ssim_slices(a, a) == []
    with pytest.raises(ValueError):
        M.ms_ssim_levels(a, a)


def test_renormalisation():
    t, _ = volumes((2, 176, 176))
    tn = M.normalize(t)
    assert np.array_equal(M.ms_ssim_renormalize(tn), tn)            # 1 + 1e-8 is 1.0f
    r = M.ms_ssim_renormalize(t)
    assert r.dtype == np.float32 and not np.array_equal(r, t) and r.min() == 0 and 0.99 < r.max() <= 1
    assert np.array_equal(r, (t - t.min()) / ((t.max() - t.min()) + np.float32(1e-8)))
    # ms_ssim is public: raw HU gives what the re-normalised volumes give
    _, p = volumes((2, 176, 176))
    assert M.ms_ssim(t, p) == M.ms_ssim(M.ms_ssim_renormalize(t), M.ms_ssim_renormalize(p))


def _same(a, b):
    return np.array_equal(np.array([a[0]] + list(a[1])), np.array([b[0]] + list(b[1])), equal_nan=True)


def test_evaluate_pair_switch():
    t, p = volumes((2, 176, 176))
    off, default, on = M.evaluate_pair(t, p, ms_ssim=False), M.evaluate_pair(t, p), M.evaluate_pair(t, p, ms_ssim=True)
    assert list(off) == list(default) == list(on) == list(M.METRICS)
    for k in M.METRICS:
        assert _same(off[k], default[k])
        if k != "ms_ssim":
            assert _same(off[k], on[k]), k
    assert math.isnan(off["ms_ssim"][0]) and off["ms_ssim"][1] == []
    assert on["ms_ssim"] == M.ms_ssim(M.normalize(t), M.normalize(p)) and 0 < on["ms_ssim"][0] < 1
    assert math.isnan(on["lpips"][0]) and on["lpips"][1] == []
    assert "ms_ssim" not in M.evaluate_pair(t, p, advanced=False, ms_ssim=True)
    m_off, l_off = M.evaluate_patient(t, p)
    m_on, l_on = M.evaluate_patient(t, p, t, ms_ssim=True)
    assert l_off["ms_ssim"] == [[]] and l_on["ms_ssim"] == [on["ms_ssim"][1]] and m_on["ms_ssim"] == [on["ms_ssim"][0]]


def test_calculate_with_the_switch(tmp_path):
    """A three-slice 176 x 176 patient through calculate.py --ms_ssim on the host."""
    import calculate
    from modules import dicom
    rng = np.random.default_rng(29)
    base = rng.integers(900, 1200, (3, 176, 176)).astype(np.int16)
    series = {"std": base, "generated": (base + rng.integers(0, 60, base.shape)).astype(np.int16)}
    dirs = {"std": tmp_path / "in" / "DS" / "P1" / "POST STD", "generated": tmp_path / "out" / "DS" / "P1"}
    for cat, vol in series.items():
        dirs[cat].mkdir(parents=True)
        for i in range(3):
            ds = dicom.new_ct_slice(vol[i], instance=i + 1, uid_suffix=f"{i}")
            ds.ImagePositionPatient = [0.0, 0.0, 2.5 * i]
            ds.save_as(str(dirs[cat] / f"{i:03d}.dcm"))
    assert calculate.get_args([]).ms_ssim is False
    calculate.main(["--input_dir_root", str(tmp_path / "in"), "--output_dir_root", str(tmp_path / "out"),
                    "--dataset_names", "DS", "--ms_ssim"])
    calc = tmp_path / "out" / "calculated"
    rows = list(csv.DictReader(open(calc / "detail" / "DS_P1_metrics.csv")))
    assert len(rows) == 3
    cells = [r["ms_ssim_STD_vs_Generated"] for r in rows]
    want = M.ms_ssim(M.normalize(series["std"].astype(np.float32) - 1024),
                     M.normalize(series["generated"].astype(np.float32) - 1024))[0]
    assert len(set(cells)) == 1 and float(cells[0]) == want and 0 < want < 1
    assert all(r["lpips_STD_vs_Generated"] == "" for r in rows)
    summary = pickle.load(open(calc / "result_all_metrics.pkl", "rb"))
    assert summary["ms_ssim"] == [[want]] and math.isnan(summary["lpips"][0][0])
    stats = {s["Metric"]: s for s in csv.DictReader(open(calc / "summary_statistics.csv"))}
    assert stats["ms_ssim_STD_vs_Generated"]["Count"] == "3"
    assert float(stats["ms_ssim_STD_vs_Generated"]["Mean"]) == float(f"{want:.4f}")
    assert not any(k.startswith("lpips") for k in stats)
