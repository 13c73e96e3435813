"""Evaluation metrics on the GPU (csrc/metrics.hip, modules/hip/metrics.py, modules/metrics_gpu.py,
calculate.py --device cuda) against the host path modules/metrics.py.

Bars.  mae, psnr, emd, ed, ts and the norms of cs: relative 1e-10 (sums of N <= 1e5 non-negative
float64 terms taken in two orders differ by at most N * 2^-53 ~ 1e-11).  cs: relative 1e-10; the
volumes here have sum|ab| / |sum ab| <= 100, asserted on the host.  ssim: absolute 1e-10 per
slice (tests/test_cpu_metrics.py).  min/max and normalize are exact; inf and nan positions agree.
"""
import csv
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG
from modules import dicom
from modules import metrics as M
from modules import metrics_gpu as G
from modules.hip import lib
from modules.hip import metrics as K

pytestmark = pytest.mark.gpu

RTOL = 1e-10
SSIM_ATOL = 1e-10
# The SSIM and Sobel kernels work on 64 x 32 output tiles (DCS_MET_TILE_X x DCS_MET_TILE_Y); SSIM's
# outputs are the interior (H-6) x (W-6).  (2,45,150) spans 2 x 3 tiles of both kernels and is a
# multiple of neither; (2,70,300) 2-3 x 5.  A slice above 8192 voxels (DCS_MET_PAIR_CHUNK)
# spans several blocks of the pair kernels; an odd slice size takes their scalar path.
assert (K.TILE_X, K.TILE_Y, lib.MET_PAIR_CHUNK) == (64, 32, 8192)
SHAPES = [(1, 7, 7), (2, 8, 70), (3, 33, 65), (2, 70, 300), (5, 9, 130), (2, 45, 150)]
KINDS = ["hu", "half", "same_slice", "const_slice"]
CASES = [(s, k) for s in SHAPES for k in KINDS]


@functools.lru_cache(maxsize=None)
def volumes(shape, kind):
    """Seeded HU-like integer volumes: an air band at -1000 (flat windows), a body from
    N(40, 60), a +1500 block; the prediction is the target plus rounded N(0, 20)."""
    rng = np.random.default_rng([17, *shape])
    d, h, w = shape
    t = np.round(rng.normal(40, 60, shape))
    t[:, : max(1, h // 4), :] = -1000
    t[:, h // 2: h // 2 + max(1, h // 5), w // 3: w // 3 + max(1, w // 4)] = 1500
    p = t + np.round(rng.normal(0, 20, shape))
    if kind == "half":                       # slope 0.5: the values are not integers
        t, p = t * 0.5, p * 0.5
    if kind == "same_slice":                 # one slice identical in both inputs
        p[d // 2] = t[d // 2]
    if kind == "const_slice":                # one constant slice
        t[d // 2], p[d // 2] = 5.0, -3.0
    t, p = t.astype(np.float32), p.astype(np.float32)
    t.setflags(write=False)
    p.setflags(write=False)
    return t, p


@functools.lru_cache(maxsize=None)
def host(shape, kind):
    """The host results of one case, computed once and shared."""
    t, p = volumes(shape, kind)
    return M.evaluate_pair(t, p)


def dev(x):
    return torch.from_numpy(np.array(x)).cuda()


def check(name, got, want):
    """got against want ((aggregate, list) of one metric) at the metric's bar."""
    (ga, gl), (wa, wl) = got, want
    g, w = np.array([ga] + list(gl), np.float64), np.array([wa] + list(wl), np.float64)
    assert g.shape == w.shape, name
    assert np.array_equal(np.isnan(g), np.isnan(w)), (name, g, w)
    assert np.array_equal(np.isinf(g), np.isinf(w)) and np.array_equal(g[np.isinf(g)], w[np.isinf(w)]), (name, g, w)
    f = np.isfinite(w)
    err = np.abs(g[f] - w[f])
    print(name, "max abs err", err.max() if err.size else 0.0,
          "max rel err", (err / np.maximum(np.abs(w[f]), 1e-300)).max() if err.size else 0.0)
    if name.startswith("ssim"):
        assert np.all(err <= SSIM_ATOL), (name, g, w)
    else:
        assert np.all(err <= RTOL * np.abs(w[f])), (name, g, w)


@pytest.mark.parametrize("shape,kind", CASES, ids=[f"{'x'.join(map(str, s))}-{k}" for s, k in CASES])
def test_device_against_host(shape, kind):
    t, p = volumes(shape, kind)
    want = host(shape, kind)
    # the bar of cs rests on little cancellation in sum ab
    for s1, s2 in zip(t.astype(np.float64), p.astype(np.float64)):
        assert np.abs(s1 * s2).sum() <= 100 * abs((s1 * s2).sum())
    dt, dp = dev(t), dev(p)
    got = G.evaluate_pair(dt, dp, "cuda")
    assert list(got) == list(want)
    for k in want:
        check(k, got[k], want[k])
    # the per-metric functions, on the raw and on materialised normalised volumes
    fns = {"mae": G.mae, "psnr": G.psnr, "ssim": G.ssim, "emd": G.emd, "ts": G.ts, "cs": G.cs, "ed": G.ed}
    for k, fn in fns.items():
        check(k, fn(dt, dp), want[k])
    tn, pn = G.normalize(dt), G.normalize(dp)
    assert np.array_equal(tn.cpu().numpy(), M.normalize(t)) and np.array_equal(pn.cpu().numpy(), M.normalize(p))
    for k in ("mae", "psnr", "ssim"):
        check(k + "_norm", fns[k](tn, pn), want[k + "_norm"])
    # exact extrema, per slice and global; the on-the-fly normalisation reads the same values
    st = K.pair_stats(dt, dp).cpu().numpy()
    flat = lambda v: v.reshape(v.shape[0], -1)
    for col, ref in ((K.MIN_A, flat(t).min(1)), (K.MAX_A, flat(t).max(1)), (K.MIN_B, flat(p).min(1)),
                     (K.MAX_B, flat(p).max(1))):
        assert np.array_equal(st[:, col], ref.astype(np.float64))
    assert G.minmax(dt) == (t.min(), t.max())
    ps = G.PairStats(dt, dp)
    stn = K.pair_stats(dt, dp, ps.normalize_affine()).cpu().numpy()
    hn, hp = flat(M.normalize(t)), flat(M.normalize(p))
    for col, ref in ((K.MIN_A, hn.min(1)), (K.MAX_A, hn.max(1)), (K.MIN_B, hp.min(1)), (K.MAX_B, hp.max(1))):
        assert np.array_equal(stn[:, col], ref.astype(np.float64))
    # the norms of cs
    for col, v in ((K.SUM_AA, t), (K.SUM_BB, p)):
        ref = (flat(v).astype(np.float64) ** 2).sum(1)
        assert np.all(np.abs(st[:, col] - ref) <= RTOL * ref)


def test_run_to_run_bit_identical():
    t, p = (dev(v) for v in volumes((2, 70, 300), "half"))
    a, b = G.evaluate_pair(t, p, "cuda"), G.evaluate_pair(t, p, "cuda")
    for k in a:
        assert np.array(a[k][1]).tobytes() == np.array(b[k][1]).tobytes(), k
        assert np.array(a[k][0]).tobytes() == np.array(b[k][0]).tobytes(), k
    for fn in (lambda: K.pair_stats(t, p), lambda: K.sobel_ts(t, p), lambda: K.ssim_sums(t, p, 1234.5)):
        assert torch.equal(fn(), fn())


@pytest.mark.parametrize("with_vue", [False, True])
def test_evaluate_patient_against_host(with_vue):
    std, gen = (np.array(v) for v in volumes((3, 33, 65), "hu"))
    gen = np.concatenate([gen, gen[:1]])                   # unequal lengths: cut to the shortest
    vue = volumes((3, 33, 65), "half")[0][:2] * 2 if with_vue else None
    want_m, want_l = G.evaluate_patient(std, gen, vue, device=None)
    got_m, got_l = G.evaluate_patient(std, gen, vue, device="cuda")
    n = 2 if with_vue else 3
    assert set(got_m) == set(want_m) == set(M.METRICS) and set(got_l) == set(want_l)
    for k in M.METRICS:
        assert len(got_m[k]) == len(want_m[k]) == ((3 if with_vue else 1) if k in M.BASIC else 1)
        assert [len(l) for l in got_l[k]] == [len(l) for l in want_l[k]]
        if k in M.BASIC or k in ("emd", "ts", "cs", "ed"):
            assert all(len(l) == n for l in got_l[k])
        for j in range(len(want_m[k])):
            check(k, (got_m[k][j], got_l[k][j]), (want_m[k][j], want_l[k][j]))


def test_bad_arguments_raise():
    t, p = volumes((2, 8, 70), "hu")
    dt, dp = dev(t), dev(p)
    for fn in (G.mae, G.psnr, G.ssim, G.emd, G.ts, G.cs, G.ed, K.pair_stats, K.sobel_ts):
        with pytest.raises(RuntimeError):
            fn(torch.from_numpy(np.array(t)), dp)            # host tensor
        with pytest.raises(RuntimeError):
            fn(dt.double(), dp.double())                     # float64
        with pytest.raises(ValueError):
            fn(dt, dp[:, :, :60])                            # mismatched shapes
    small = dt[:, :6, :].contiguous()
    with pytest.raises(ValueError):
        G.ssim(small, small)
    with pytest.raises(ValueError):
        G.evaluate_pair(small, small, "cuda")
    with pytest.raises(ValueError):
        K.ssim_sums(small, small, 1.0)
    with pytest.raises(ValueError):
        K.ed_sums(dt, dp, torch.zeros(2, 3, dtype=torch.float64, device="cuda"))
    # the C entry points refuse the same calls before any launch
    out = torch.zeros(2, dtype=torch.float64, device="cuda")
    ws = torch.zeros(64, dtype=torch.float64, device="cuda")
    ptr = lambda x: x.data_ptr()
    with pytest.raises(lib.HipLibraryError, match="1001"):
        lib.call("dcs_met_ssim", ptr(small), ptr(small), 2, 6, 70, None, 1.0, ptr(out), ptr(ws), 512, None)
    with pytest.raises(lib.HipLibraryError, match="1001"):
        lib.call("dcs_met_sobel_ts", ptr(dt), ptr(dp), 0, 8, 70, ptr(out), ptr(ws), 512, None)
    with pytest.raises(lib.HipLibraryError, match="1002"):
        lib.call("dcs_met_pair_stats", ptr(dt), ptr(dp), 2, 8, 70, None, ptr(out), ptr(ws), 8, None)
    assert lib.query("dcs_met_workspace_size", 0, 8, 70) == 0
    assert lib.query("dcs_met_workspace_size", 2, 8, 70) == 8 * 2 * 9
    torch.cuda.synchronize()


def _run_calculate(tmp_path, device):
    out = tmp_path / f"out_{device}"
    cmd = [sys.executable, os.path.join(PKG, "calculate.py"), "--input_dir_root", str(tmp_path / "in"),
           "--output_dir_root", str(out), "--dataset_names", "DS", "--device", device]
    subprocess.run(cmd, check=True, timeout=300, stdout=subprocess.DEVNULL)
    return out / "calculated"


def test_calculate_end_to_end(tmp_path):
    """A three-series patient (3 slices of 16x16, shuffled z positions) through calculate.py with
    --device cuda and --device cpu, a fresh child process each."""
    rng = np.random.default_rng(23)
    base = rng.integers(900, 1200, (3, 16, 16)).astype(np.int16)
    series = {"vue": base, "std": (base + rng.integers(0, 60, base.shape)).astype(np.int16),
              "generated": (base + rng.integers(0, 60, base.shape)).astype(np.int16)}
    series["generated"][1] = series["std"][1]               # an inf cell
    order = [2, 0, 1]
    for dev_name in ("cuda", "cpu"):
        dirs = {"vue": tmp_path / "in" / "DS" / "P1" / "POST VUE", "std": tmp_path / "in" / "DS" / "P1" / "POST STD",
                "generated": tmp_path / f"out_{dev_name}" / "DS" / "P1"}
        for cat, vol in series.items():
            if dirs[cat].exists():
                continue
            dirs[cat].mkdir(parents=True)
            for fi, zi in enumerate(order):
                ds = dicom.new_ct_slice(vol[zi], instance=fi + 1, uid_suffix=f"{fi}")
                ds.ImagePositionPatient = [0.0, 0.0, 2.5 * zi]
                ds.save_as(str(dirs[cat] / f"{fi:03d}.dcm"))
    calc = {d: _run_calculate(tmp_path, d) for d in ("cuda", "cpu")}
    for cat, vol in series.items():
        a = np.load(calc["cuda"] / "data" / f"DS_P1_{cat}.npy")
        b = np.load(calc["cpu"] / "data" / f"DS_P1_{cat}.npy")
        assert np.array_equal(a, b) and np.array_equal(a, vol.astype(np.float32) - 1024)     # z order
    rows = {d: list(csv.reader(open(calc[d] / "detail" / "DS_P1_metrics.csv"))) for d in calc}
    assert rows["cuda"][0] == rows["cpu"][0] and len(rows["cuda"]) == len(rows["cpu"]) == 4
    saw_inf = saw_empty = False
    for name, *cells in zip(rows["cpu"][0], *rows["cuda"][1:], *rows["cpu"][1:]):
        got, want = cells[:3], cells[3:]
        for g, w in zip(got, want):
            if w == "":
                assert g == ""
                saw_empty = True
                continue
            g, w = float(g), float(w)
            if np.isinf(w):
                assert g == w
                saw_inf = True
            elif name.startswith("ssim"):
                assert abs(g - w) <= SSIM_ATOL, name
            else:
                assert abs(g - w) <= RTOL * abs(w), name
    assert saw_inf and saw_empty
    for d in calc:
        assert (calc[d] / "result_all_metrics.pkl").exists() and (calc[d] / "summary_statistics.csv").exists()
