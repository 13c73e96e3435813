"""LPIPS on the host (modules/metrics.py::lpips, modules/lpips_weights.py, calculate.py
--lpips_weights), no GPU.

The weights are stand-ins from a seeded PRNG (lpips_weights.random_state_dict: He-scaled conv
weights, small biases, non-negative lin vectors); the real ones cannot be obtained here, so
parity with the lpips package is unpinned and the oracle is the same restatement in float64.

F32_BAR: the float32 path against the float64 oracle.  The longest dot product of the trunk has
K = 384 * 9 = 3456 terms; its worst-case rounding error is K * eps32 / 2 relative to the sum of
magnitudes (2.1e-4), and the observed error of blocked float32 sums is far below that.  The bar
is that worst case, as a relative error of a slice's value.
"""
import csv
import functools
import math
import pickle

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from modules import lpips_weights as LW
from modules import metrics as M

F32_BAR = 3456 * float(np.finfo(np.float32).eps) / 2


@functools.lru_cache(maxsize=None)
def weights(seed=3):
    return LW.from_state_dicts(LW.random_state_dict(seed))


@functools.lru_cache(maxsize=None)
def volumes(shape):
    """Seeded HU-like integer volumes (the generator of tests/test_cpu_msssim.py)."""
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


def test_without_weights_nothing_changes():
    t, p = volumes((3, 35, 47))
    agg, lst = M.lpips(t, p)
    assert math.isnan(agg) and lst == []
    out = M.evaluate_pair(t, p)
    assert math.isnan(out["lpips"][0]) and out["lpips"][1] == []


def test_float32_agrees_with_the_float64_oracle():
    t, p = volumes((3, 35, 47))
    tn, pn = M.normalize(t), M.normalize(p)
    agg, lst = M.lpips(tn, pn, weights())
    agg64, lst64 = M.lpips(tn, pn, weights(), dtype=torch.float64)
    assert len(lst) == len(lst64) == 3 and all(v > 0 for v in lst64)
    err = max(abs(a - b) / b for a, b in zip(lst, lst64))
    print(f"float32 against float64: {err:.3e} (bar {F32_BAR:.3e}); values {lst64}")
    assert err <= F32_BAR
    assert abs(agg - agg64) <= F32_BAR * agg64 and agg64 == float(np.mean(lst64))
    # the per-slice list holds the per-slice values, not the repeated mean
    assert len(set(lst64)) == 3
    # the taps sum to the value
    taps = M.lpips_taps(tn, pn, weights(), torch.float64)
    assert taps.shape == (5, 3) and np.array_equal(taps.sum(0), np.array(lst64))


def test_identical_volumes_give_zero_and_the_value_is_symmetric():
    t, p = volumes((3, 35, 47))
    for dtype in (None, torch.float64):
        agg, lst = M.lpips(t, t, weights(), dtype=dtype)
        assert agg == 0.0 and lst == [0.0, 0.0, 0.0]
        assert M.lpips(t, p, weights(), dtype=dtype) == M.lpips(p, t, weights(), dtype=dtype)


def test_smallest_image():
    rng = np.random.default_rng(2)
    for shape in ((2, 30, 40), (2, 40, 30)):
        a, b = rng.random(shape, dtype=np.float32), rng.random(shape, dtype=np.float32)
        agg, lst = M.lpips(a, b, weights())
        assert math.isnan(agg) and lst == []
        with pytest.raises(ValueError, match="at least 31"):
            M.lpips_taps(a, b, weights())
    a, b = rng.random((2, 31, 31), dtype=np.float32), rng.random((2, 31, 31), dtype=np.float32)
    agg, lst = M.lpips(a, b, weights())
    assert len(lst) == 2 and all(math.isfinite(v) and v > 0 for v in lst) and math.isfinite(agg)
    assert LW.out_sizes(31, 31) == [(7, 7), (3, 3), (1, 1), (1, 1), (1, 1)]
    assert LW.out_sizes(512, 512) == [(127, 127), (63, 63), (31, 31), (31, 31), (31, 31)]
    fa = M.lpips_features(M.lpips_input(a), weights())
    assert [tuple(f.shape[1:]) for f in fa] == [(c, h, w) for c, (h, w) in zip(LW.CHANNELS, LW.out_sizes(31, 31))]


def test_loader_accepts_both_layouts(tmp_path):
    sd_l, sd_t = LW.random_state_dict(5, "lpips"), LW.random_state_dict(5, "torchvision")
    trunk = {k: v for k, v in sd_t.items() if k.startswith("features.")}
    lins = {k: v for k, v in sd_t.items() if k.startswith("lin")}
    assert len(trunk) == 10 and len(lins) == 5
    # what the real files carry besides: ignored
    sd_l.update({"scaling_layer.shift": torch.zeros(1, 3, 1, 1), "lins.0.model.1.weight": torch.ones(1, 64, 1, 1)})
    trunk.update({"classifier.1.weight": torch.zeros(8, 8), "classifier.1.bias": torch.zeros(8)})
    torch.save(sd_l, tmp_path / "lpips.pth")
    torch.save(trunk, tmp_path / "alexnet.pth")
    torch.save(lins, tmp_path / "alex.pth")
    one = LW.load(str(tmp_path / "lpips.pth"))
    two = LW.load(f"{tmp_path / 'alexnet.pth'},{tmp_path / 'alex.pth'}")
    direct = LW.from_state_dicts(LW.random_state_dict(5))
    for a, b, c in zip(one.tensors(), two.tensors(), direct.tensors()):
        assert a.dtype == torch.float32 and torch.equal(a, b) and torch.equal(a, c)
    assert [tuple(w.shape) for w, _ in one.convs] == [(co, ci, k, k) for co, ci, k, _, _, _ in LW.CONVS]
    assert [tuple(l.shape) for l in one.lins] == [(c,) for c in LW.CHANNELS]


def test_loader_names_what_is_wrong(tmp_path):
    sd = LW.random_state_dict(5, "torchvision")
    missing = {k: v for k, v in sd.items() if k != "lin3.model.1.weight"}
    with pytest.raises(ValueError, match=r"lin3\.model\.1\.weight"):
        LW.from_state_dicts(missing)
    bad = dict(sd)
    bad["features.3.weight"] = torch.zeros(192, 64, 3, 3)
    with pytest.raises(ValueError, match=r"features\.3\.weight has shape \(192, 64, 3, 3\)"):
        LW.from_state_dicts(bad)
    torch.save({k: v for k, v in sd.items() if k.startswith("features.")}, tmp_path / "alexnet.pth")
    with pytest.raises(ValueError, match=r"lin0\.model\.1\.weight.*lin4\.model\.1\.weight"):
        LW.load(str(tmp_path / "alexnet.pth"))
    with pytest.raises(ValueError, match="one file or two"):
        LW.load("a,b,c")


def test_first_layer_fold_needs_the_constant_channel():
    """The scaling layer on three equal channels folds into a 2-channel convolution over (x, 1);
    the padding is zero after the scaling layer, so the constant channel is zero there too and a
    fold that adds its weights to the bias is wrong wherever the kernel overhangs the image."""
    w = weights()
    x = torch.from_numpy(np.random.default_rng(4).uniform(0.5, 1.0, (2, 37, 45)).astype(np.float32))  # non-zero border
    want = M.lpips_features(x, w, torch.float64, stem=None)[0]
    wx, wc = LW.stem_fold(w, torch.float64)
    bias = w.convs[0][1].double()

    def two_channel(x1, _):
        return F.conv2d(torch.cat((x1, torch.ones_like(x1)), 1), torch.stack((wx, wc), 1), bias, stride=4, padding=2)

    def plain_bias(x1, _):
        return F.conv2d(x1, wx.unsqueeze(1), bias + wc.sum((1, 2)), stride=4, padding=2)

    got = M.lpips_features(x, w, torch.float64, stem=two_channel)[0]
    wrong = M.lpips_features(x, w, torch.float64, stem=plain_bias)[0]
    scale = float(want.abs().max())
    assert float((got - want).abs().max()) <= 1e-12 * scale
    ring = torch.ones_like(want, dtype=torch.bool)
    ring[:, :, 1:-1, 1:-1] = False
    assert float((wrong - want).abs()[ring].max()) > 1e-3 * scale      # the ring that sees the padding
    assert float((wrong - want).abs()[~ring].max()) <= 1e-12 * scale   # and only that ring


def _write_patient(tmp_path, series):
    from modules import dicom
    dirs = {"std": tmp_path / "in" / "DS" / "P1" / "POST STD", "generated": tmp_path / "out" / "DS" / "P1"}
    for cat, vol in series.items():
        dirs[cat].mkdir(parents=True)
        for i in range(len(vol)):
            ds = dicom.new_ct_slice(vol[i], instance=i + 1, uid_suffix=f"{i}")
            ds.ImagePositionPatient = [0.0, 0.0, 2.5 * i]
            ds.save_as(str(dirs[cat] / f"{i:03d}.dcm"))


def test_calculate_with_the_flag(tmp_path):
    """A three-slice 32 x 32 patient through calculate.py on the host, with and without --lpips_weights."""
    import calculate
    rng = np.random.default_rng(29)
    base = rng.integers(900, 1200, (3, 32, 32)).astype(np.int16)
    series = {"std": base, "generated": (base + rng.integers(0, 60, base.shape)).astype(np.int16)}
    wpath = tmp_path / "w.pth"
    torch.save(LW.random_state_dict(3), wpath)
    assert calculate.get_args([]).lpips_weights is None
    runs = {}
    for name, extra in (("on", ["--lpips_weights", str(wpath)]), ("off", [])):
        root = tmp_path / name
        root.mkdir()
        _write_patient(root, series)
        calculate.main(["--input_dir_root", str(root / "in"), "--output_dir_root", str(root / "out"),
                        "--dataset_names", "DS"] + extra)
        calc = root / "out" / "calculated"
        runs[name] = (list(csv.DictReader(open(calc / "detail" / "DS_P1_metrics.csv"))),
                      pickle.load(open(calc / "result_all_metrics.pkl", "rb")),
                      {s["Metric"]: s for s in csv.DictReader(open(calc / "summary_statistics.csv"))})
    want = M.lpips(M.normalize(series["std"].astype(np.float32) - 1024),
                   M.normalize(series["generated"].astype(np.float32) - 1024), weights())
    rows, summary, stats = runs["on"]
    assert [float(r["lpips_STD_vs_Generated"]) for r in rows] == want[1] and len(rows) == 3
    assert summary["lpips"] == [[want[0]]] and want[0] > 0
    assert stats["lpips_STD_vs_Generated"]["Count"] == "3"
    assert float(stats["lpips_STD_vs_Generated"]["Mean"]) == float(f"{np.mean(want[1]):.4f}")
    # without the flag: the empty column, the nan entry and no summary row of earlier runs
    rows0, summary0, stats0 = runs["off"]
    assert all(r["lpips_STD_vs_Generated"] == "" for r in rows0)
    assert math.isnan(summary0["lpips"][0][0]) and not any(k.startswith("lpips") for k in stats0)
    # and the flag changes nothing else
    for r, r0 in zip(rows, rows0):
        assert {k: v for k, v in r.items() if not k.startswith("lpips")} == \
               {k: v for k, v in r0.items() if not k.startswith("lpips")}
    assert {k: v for k, v in stats.items() if not k.startswith("lpips")} == stats0
    for k in M.METRICS:
        if k != "lpips":
            assert np.array_equal(np.array(summary[k]), np.array(summary0[k]), equal_nan=True), k
