"""MS-SSIM on the GPU (csrc/metrics.hip: msssim_kernel, pool2_kernel; modules/metrics_gpu.py;
calculate.py --ms_ssim --device cuda) against the host path modules/metrics.py.

Bars.  The pyramids are bit-identical (the pooling rule fixes the order of the four-term sum).
Per level and slice the means of the SSIM map and of its contrast-structure factor: absolute
1e-10, the bar SSIM has; both paths divide by denominators of at least C2 in float64.  The final
values, per slice and aggregate: absolute 1e-9.  With d(x^b)/dx = b x^(b-1), every clamped level
mean >= 0.05 (asserted on the host values below) and b <= 0.3001, an error of 1e-10 in a level
moves its factor by under 2.5e-10; five factors of at most 1 give about 1.2e-9 in the worst case.
The per-level errors this test prints (1.3e-13 at most on an MI355X, on the constant slice, and
9e-15 elsewhere) leave room for 1e-9, which is the bar used.  The anti-correlated pair is exactly 0.0 on both paths.

Shapes: (2,176,176) reaches one output pixel at the fifth level; (2,177,243) has odd sizes at
every level; (3,200,355) spans several partial 64 x 32 tiles at level 0.
"""
import csv
import ctypes
import functools
import math
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

LEVEL_ATOL = 1e-10
FINAL_ATOL = 1e-9
RTOL, SSIM_ATOL = 1e-10, 1e-10           # the bars of tests/test_gpu_metrics.py for the other columns
assert (K.TILE_X, K.TILE_Y) == (64, 32)
SHAPES = [(2, 176, 176), (2, 177, 243), (3, 200, 355)]
KINDS = ["hu", "same_slice", "const_slice"]
CASES = [(s, k) for s in SHAPES for k in KINDS]
ANTI = ((2, 176, 176), "anti")


@functools.lru_cache(maxsize=None)
def volumes(shape, kind):
    """Seeded HU-like integer volumes (the generator of tests/test_gpu_metrics.py): an air band at
    -1000 (flat windows), a body from N(40, 60), a +1500 block; the prediction is the target plus
    rounded N(0, 20).  "anti": uniform noise t and p = 1 - t."""
    d, h, w = shape
    if kind == "anti":
        t = np.random.default_rng(5).random(shape, dtype=np.float32)
        p = np.float32(1) - t
    else:
        rng = np.random.default_rng([17, *shape])
        t = np.round(rng.normal(40, 60, shape))
        t[:, : max(1, h // 4), :] = -1000
        t[:, h // 2: h // 2 + max(1, h // 5), w // 3: w // 3 + max(1, w // 4)] = 1500
        p = t + np.round(rng.normal(0, 20, shape))
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
    """The host pyramid, level means and per-slice values of one case, computed once and shared."""
    t, p = volumes(shape, kind)
    levels = M.ms_ssim_levels(t, p)
    levels.setflags(write=False)
    return M.ms_ssim_pyramid(t, p), levels, tuple(M.ms_ssim_from_levels(levels))


def dev(x):
    return torch.from_numpy(np.array(x)).cuda()


@pytest.mark.parametrize("shape,kind", CASES + [ANTI], ids=[f"{'x'.join(map(str, s))}-{k}" for s, k in CASES + [ANTI]])
def test_device_against_host(shape, kind):
    t, p = volumes(shape, kind)
    pyr, want_levels, want_vals = host(shape, kind)
    dt, dp = dev(t), dev(p)
    got_pyr = G.ms_ssim_pyramid(dt, dp)
    assert len(got_pyr) == len(pyr) == 5
    for (gx, gy), (hx, hy) in zip(got_pyr, pyr):
        assert gx.dtype == gy.dtype == torch.float32
        assert np.array_equal(gx.cpu().numpy(), hx) and np.array_equal(gy.cpu().numpy(), hy)
    got_levels = G.ms_ssim_levels(dt, dp)
    assert got_levels.shape == want_levels.shape == (5, shape[0], 2) and got_levels.dtype == np.float64
    err = np.abs(got_levels - want_levels)
    print("level means: max abs err per level", err.max(axis=(1, 2)))
    assert np.all(err <= LEVEL_ATOL)
    got_vals = G.ms_ssim_slices(dt, dp)
    got, want = G.ms_ssim(dt, dp), M.ms_ssim(t, p)
    assert len(got_vals) == shape[0] and got[1] == [got[0]] * shape[0] and want[1] == [want[0]] * shape[0]
    if kind == "anti":
        assert want_levels[:, :, 1].min() < -0.05            # the clamp really ran
        assert got_vals == [0.0] * shape[0] == list(want_vals) and got[0] == 0.0 == want[0]
        return
    # the bar of the final values rests on clamped level means of at least 0.05
    used = np.concatenate([want_levels[:4, :, 1].ravel(), want_levels[4, :, 0].ravel()])
    print("smallest level mean used", used.min())
    assert used.min() >= 0.05
    ferr = np.abs(np.array(got_vals) - np.array(want_vals))
    print("final values: max abs err", ferr.max(), "aggregate", abs(got[0] - want[0]))
    assert np.all(ferr <= FINAL_ATOL) and abs(got[0] - want[0]) <= FINAL_ATOL


def test_identical_volumes_give_exactly_one():
    t = dev(volumes((2, 177, 243), "hu")[0])
    assert G.ms_ssim(t, t) == (1.0, [1.0, 1.0])


def test_run_to_run_bit_identical():
    t, p = (dev(v) for v in volumes((3, 200, 355), "hu"))
    a, b = G.ms_ssim_levels(t, p), G.ms_ssim_levels(t, p)
    assert a.tobytes() == b.tobytes()
    x, y = G.ms_ssim_pyramid(t, p)[1]
    fn = lambda: K.msssim_level_sums(x, y, M.MS_SSIM_WINDOW, M.MS_SSIM_C1, M.MS_SSIM_C2)
    assert torch.equal(fn(), fn())
    assert all(torch.equal(u, v) for u, v in zip(K.pool2(x, y), K.pool2(x, y)))


def test_evaluate_pair_switch():
    t, p = volumes((2, 176, 176), "hu")
    dt, dp = dev(t), dev(p)
    off, on = G.evaluate_pair(dt, dp, "cuda"), G.evaluate_pair(dt, dp, "cuda", ms_ssim=True)
    assert list(off) == list(on) == list(M.METRICS)
    for k in M.METRICS:
        if k != "ms_ssim":
            assert np.array_equal(np.array([off[k][0]] + list(off[k][1])), np.array([on[k][0]] + list(on[k][1])),
                                  equal_nan=True), k
    assert math.isnan(off["ms_ssim"][0]) and off["ms_ssim"][1] == []
    want = M.evaluate_pair(t, p, ms_ssim=True)["ms_ssim"]
    assert abs(on["ms_ssim"][0] - want[0]) <= FINAL_ATOL and on["ms_ssim"][1] == [on["ms_ssim"][0]] * 2
    got_m, got_l = G.evaluate_patient(np.array(t), np.array(p), np.array(t), device="cuda", ms_ssim=True)
    assert got_m["ms_ssim"] == [on["ms_ssim"][0]] and got_l["ms_ssim"] == [on["ms_ssim"][1]]
    assert G.evaluate_patient(np.array(t), np.array(p), device="cuda")[1]["ms_ssim"] == [[]]


def test_bad_arguments():
    t, p = volumes((2, 176, 176), "hu")
    dt, dp = dev(t), dev(p)
    win = lambda x, y: K.msssim_level_sums(x, y, M.MS_SSIM_WINDOW, M.MS_SSIM_C1, M.MS_SSIM_C2)
    for fn in (G.ms_ssim, G.ms_ssim_slices, G.ms_ssim_levels, G.ms_ssim_pyramid, K.pool2, win):
        with pytest.raises(RuntimeError):
            fn(torch.from_numpy(np.array(t)), dp)            # host tensor
        with pytest.raises(RuntimeError):
            fn(dt.double(), dp.double())                     # float64
        with pytest.raises(ValueError):
            fn(dt, dp[:, :, :100])                           # mismatched shapes
    # not defined below 176 on a side: (nan, []) without a launch, and no exception
    for small in (dt[:, :175, :].contiguous(), dt[:, :, :175].contiguous()):
        agg, lst = G.ms_ssim(small, small)
        assert math.isnan(agg) and lst == [] and G.ms_ssim_slices(small, small) == []
        with pytest.raises(ValueError):
            G.ms_ssim_levels(small, small)
    tiny = dt[:, :10, :].contiguous()
    with pytest.raises(ValueError):
        win(tiny, tiny)
    with pytest.raises(ValueError):
        K.msssim_level_sums(dt, dp, M.MS_SSIM_WINDOW[:7], M.MS_SSIM_C1, M.MS_SSIM_C2)
    with pytest.raises(ValueError):
        K.pool2(dt[:, :1, :].contiguous(), dp[:, :1, :].contiguous())
    # the C entry points refuse the same calls before any launch
    out = torch.zeros(4, dtype=torch.float64, device="cuda")
    nws = lib.query("dcs_met_workspace_size", 2, 176, 176)
    ws = torch.zeros(nws // 8, dtype=torch.float64, device="cuda")
    oa, ob = torch.zeros(2, 88, 88, device="cuda"), torch.zeros(2, 88, 88, device="cuda")
    ptr = lambda x: x.data_ptr()
    g = (ctypes.c_double * 11)(*M.MS_SSIM_WINDOW)
    bad = (ctypes.c_double * 11)(*([float("nan")] + [0.1] * 10))
    c1, c2 = M.MS_SSIM_C1, M.MS_SSIM_C2
    level = lambda *a: lib.call("dcs_met_msssim_level", *a)
    with pytest.raises(lib.HipLibraryError, match="1001"):
        level(ptr(dt), ptr(dp), 2, 10, 176, g, c1, c2, ptr(out), ptr(ws), nws, None)          # H = 10
    with pytest.raises(lib.HipLibraryError, match="1001"):
        level(ptr(dt), ptr(dp), 2, 176, 10, g, c1, c2, ptr(out), ptr(ws), nws, None)
    with pytest.raises(lib.HipLibraryError, match="1001"):
        level(None, ptr(dp), 2, 176, 176, g, c1, c2, ptr(out), ptr(ws), nws, None)            # null pointer
    with pytest.raises(lib.HipLibraryError, match="1001"):
        level(ptr(dt), ptr(dp), 2, 176, 176, None, c1, c2, ptr(out), ptr(ws), nws, None)      # null window
    with pytest.raises(lib.HipLibraryError, match="1001"):
        level(ptr(dt), ptr(dp), 2, 176, 176, bad, c1, c2, ptr(out), ptr(ws), nws, None)       # non-finite window
    with pytest.raises(lib.HipLibraryError, match="1002"):
        level(ptr(dt), ptr(dp), 2, 176, 176, g, c1, c2, ptr(out), ptr(ws), 2 * 18 * 2 * 8 - 1, None)   # short workspace
    with pytest.raises(lib.HipLibraryError, match="1001"):
        lib.call("dcs_met_pool2", ptr(dt), ptr(dp), ptr(oa), ptr(ob), 2, 1, 176, None)
    with pytest.raises(lib.HipLibraryError, match="1001"):
        lib.call("dcs_met_pool2", ptr(dt), ptr(dp), ptr(oa), ptr(ob), 2, 176, 1, None)
    with pytest.raises(lib.HipLibraryError, match="1001"):
        lib.call("dcs_met_pool2", ptr(dt), ptr(dp), None, ptr(ob), 2, 176, 176, None)
    assert not out.any() and not oa.any() and not ob.any()       # nothing was launched
    assert lib.query("dcs_met_workspace_size", 2, 8, 70) == 8 * 2 * 9            # unchanged
    assert nws >= 2 * 18 * 2 * 8                                 # covers two partials per tile
    torch.cuda.synchronize()


def _run_calculate(tmp_path, device):
    out = tmp_path / f"out_{device}"
    cmd = [sys.executable, os.path.join(PKG, "calculate.py"), "--input_dir_root", str(tmp_path / "in"),
           "--output_dir_root", str(out), "--dataset_names", "DS", "--device", device, "--ms_ssim"]
    subprocess.run(cmd, check=True, timeout=300, stdout=subprocess.DEVNULL)
    return out / "calculated"


def test_calculate_end_to_end(tmp_path):
    """A three-slice 176 x 176 patient through calculate.py --ms_ssim with --device cuda and
    --device cpu, a fresh child process each."""
    rng = np.random.default_rng(31)
    base = rng.integers(900, 1200, (3, 176, 176)).astype(np.int16)
    series = {"vue": base, "std": (base + rng.integers(0, 60, base.shape)).astype(np.int16),
              "generated": (base + rng.integers(0, 60, base.shape)).astype(np.int16)}
    for dev_name in ("cuda", "cpu"):
        dirs = {"vue": tmp_path / "in" / "DS" / "P1" / "POST VUE", "std": tmp_path / "in" / "DS" / "P1" / "POST STD",
                "generated": tmp_path / f"out_{dev_name}" / "DS" / "P1"}
        for cat, vol in series.items():
            if dirs[cat].exists():
                continue
            dirs[cat].mkdir(parents=True)
            for i in range(3):
                ds = dicom.new_ct_slice(vol[i], instance=i + 1, uid_suffix=f"{i}")
                ds.ImagePositionPatient = [0.0, 0.0, 2.5 * i]
                ds.save_as(str(dirs[cat] / f"{i:03d}.dcm"))
    calc = {d: _run_calculate(tmp_path, d) for d in ("cuda", "cpu")}
    rows = {d: list(csv.reader(open(calc[d] / "detail" / "DS_P1_metrics.csv"))) for d in calc}
    assert rows["cuda"][0] == rows["cpu"][0] and len(rows["cuda"]) == len(rows["cpu"]) == 4
    seen = set()
    for name, *cells in zip(rows["cpu"][0], *rows["cuda"][1:], *rows["cpu"][1:]):
        got, want = cells[:3], cells[3:]
        if name.startswith("lpips"):
            assert got == want == ["", "", ""]
            seen.add("lpips")
            continue
        got, want = [float(g) for g in got], [float(w) for w in want]
        for g, w in zip(got, want):
            if name.startswith("ms_ssim"):
                assert abs(g - w) <= FINAL_ATOL and 0 < w < 1, name
                seen.add("ms_ssim")
            elif name.startswith("ssim"):
                assert abs(g - w) <= SSIM_ATOL, name
            else:
                assert abs(g - w) <= RTOL * abs(w), name
        if name.startswith("ms_ssim"):
            assert len(set(got)) == 1 and len(set(want)) == 1    # the batch value, repeated
    assert seen == {"lpips", "ms_ssim"}
    for d in calc:
        stats = {s["Metric"] for s in csv.DictReader(open(calc[d] / "summary_statistics.csv"))}
        assert "ms_ssim_STD_vs_Generated" in stats and not any(s.startswith("lpips") for s in stats)
