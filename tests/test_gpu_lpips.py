"""LPIPS on the GPU (csrc/lpips.hip: lpips_stem_kernel, lpips_tap_kernel; layers 2-5 on the rows
pass; modules/hip/lpips.py; modules/metrics_gpu.py::lpips) against the float64 oracle
modules/metrics.py::lpips_taps(dtype=float64) on the same seeded stand-in weights.

Bar: the project's own (tests/test_gpu_nmodel.py), 4 x the error of the float32 ATen path on the
host against float64, taken as the maximum over the cases below so that one lucky small
denominator does not set it.  Errors are relative, per slice (and per tap and slice).

Shapes: 2x31x31, every map ends at 1x1; 3x35x47, non-square, odd maps, both pools drop a
remainder row and column; 2x96x80, maps of 23x19 -> 11x9 -> 5x4, several tiles and partials;
1x512x512, the workload's own map sizes 127 / 63 / 31.  The prediction is the target plus
N(0, 150) HU, which gives values of a few 1e-3 to 1e-2.
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
from modules import metrics_gpu as G
from modules.hip import lib
from modules.hip import lpips as L

pytestmark = pytest.mark.gpu

SHAPES = [(2, 31, 31), (3, 35, 47), (2, 96, 80), (1, 512, 512)]
RTOL, SSIM_ATOL = 1e-10, 1e-10   # the bars of tests/test_gpu_metrics.py for the other columns


@functools.lru_cache(maxsize=None)
def weights():
    return LW.from_state_dicts(LW.random_state_dict(3))


@functools.lru_cache(maxsize=None)
def volumes(shape):
    """Seeded HU-like volumes: an air band at -1000, a body from N(40, 60), a +1500 block; the
    prediction is the target plus rounded N(0, 150)."""
    rng = np.random.default_rng([23, *shape])
    d, h, w = shape
    t = np.round(rng.normal(40, 60, shape))
    t[:, : max(1, h // 4), :] = -1000
    t[:, h // 2: h // 2 + max(1, h // 5), w // 3: w // 3 + max(1, w // 4)] = 1500
    p = t + np.round(rng.normal(0, 150, shape))
    t, p = M.normalize(t.astype(np.float32)), M.normalize(p.astype(np.float32))
    t.setflags(write=False)
    p.setflags(write=False)
    return t, p


@functools.lru_cache(maxsize=None)
def oracle(shape):
    """(float64 taps [5][D], float32-ATen taps [5][D]) on the host, computed once per shape."""
    t, p = volumes(shape)
    t64, t32 = M.lpips_taps(t, p, weights(), torch.float64), M.lpips_taps(t, p, weights(), torch.float32)
    t64.setflags(write=False)
    t32.setflags(write=False)
    return t64, t32


def rel(got, want):
    return float(np.max(np.abs(np.asarray(got) - np.asarray(want)) / np.abs(np.asarray(want))))


@functools.lru_cache(maxsize=None)
def bars():
    """(bar of a slice's value, bar of one tap's value): 4 x the float32 ATen path's largest relative
    error over all cases."""
    pairs = [oracle(s) for s in SHAPES]
    return (4 * max(rel(t32.sum(0), t64.sum(0)) for t64, t32 in pairs),
            4 * max(rel(t32, t64) for t64, t32 in pairs))


def dev(x):
    return torch.from_numpy(np.array(x)).cuda()   # a copy: the cached arrays are read-only


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_the_float64_oracle(shape):
    t, p = volumes(shape)
    t64, _ = oracle(shape)
    bar, tap_bar = bars()
    taps = G.lpips_taps(dev(t), dev(p), weights())
    assert taps.shape == t64.shape == (5, shape[0]) and np.all(t64 > 0)
    tap_err, err = rel(taps, t64), rel(taps.sum(0), t64.sum(0))
    print(f"lpips {shape}: per-tap error {tap_err:.3e} (bar {tap_bar:.3e}), per-slice error {err:.3e} (bar {bar:.3e}); "
          f"values {t64.sum(0)[:3]}")
    assert tap_err <= tap_bar   # each of the five taps: a wrong pool or norm cannot hide behind the largest
    assert err <= bar
    agg, lst = G.lpips(dev(t), dev(p), weights())
    assert lst == taps.sum(0).tolist() and agg == float(np.mean(lst))


def _scaled3(x, dtype):
    """The scaling layer on three equal channels of lpips_input values x [N,H,W]."""
    shift = torch.tensor(LW.SHIFT, dtype=dtype).view(1, 3, 1, 1)
    scale = torch.tensor(LW.SCALE, dtype=dtype).view(1, 3, 1, 1)
    return (torch.from_numpy(x).to(dtype).unsqueeze(1).repeat(1, 3, 1, 1) - shift) / scale


@functools.lru_cache(maxsize=None)
def stem_oracle(shape):
    """(float64, float32) F.conv2d + ReLU of the first layer on the 3-channel scaled input, NHWC."""
    x = M.lpips_input(volumes(shape)[0])
    w, b = weights().convs[0]
    y64 = F.relu(F.conv2d(_scaled3(x, torch.float64), w.double(), b.double(), stride=4, padding=2))
    y32 = F.relu(F.conv2d(_scaled3(x, torch.float32), w, b, stride=4, padding=2))
    return y64.permute(0, 2, 3, 1).contiguous(), y32.permute(0, 2, 3, 1).double()


def _rings(y):
    m = torch.ones(y.shape[1:3], dtype=torch.bool)
    m[2:-2, 2:-2] = False
    return m


def test_first_layer_alone():
    """The whole map and, separately, its outer two rings, where the constant channel of the fold
    sees the padding: relative to the largest output, 4 x the float32 F.conv2d error over the cases."""
    errs32, errs, ring_errs = [], [], []
    plan = L.plan_for(weights(), "cuda")
    for shape in SHAPES:
        t = volumes(shape)[0]
        y64, y32 = stem_oracle(shape)
        mn, mx = t.min(), t.max()
        got = L.stem(dev(t), float(mn), float((mx - mn) + M.EPS32), plan).cpu().double()
        assert got.shape == y64.shape
        scale = float(y64.abs().max())
        errs32.append(float((y32 - y64).abs().max()) / scale)
        errs.append(float((got - y64).abs().max()) / scale)
        ring_errs.append(float((got - y64).abs()[:, _rings(y64)].max()) / scale)
    bar = 4 * max(errs32)
    print(f"first layer: errors {errs}, outer two rings {ring_errs}, bar {bar:.3e}")
    assert max(errs) <= bar
    assert max(ring_errs) <= bar


@pytest.mark.parametrize("C,h,w,pool", [(64, 23, 19, True), (192, 11, 9, True), (384, 5, 4, True), (256, 1, 1, False),
                                        (256, 3, 3, False)])
def test_fused_pass_alone(C, h, w, pool):
    """Given float32 feature maps: the sums against the formula in float64 (the kernel's own
    arithmetic: float64 on the float32 samples, so 1e-12 relative), the pooled maps exactly."""
    rng = np.random.default_rng([C, h, w])
    N = 3
    f = np.maximum(rng.normal(0.2, 1.0, (2 * N, h, w, C)), 0).astype(np.float32)
    f[0, 0, 0, :] = 0   # a pixel whose features are all zero in both images: 0 / 1e-10 -> 0, no NaN
    f[N, 0, 0, :] = 0
    f[1, h - 1, w - 1, :] = 0   # and in one image only
    lin = rng.uniform(0, 1, C).astype(np.float32)
    fd = dev(f)
    sums, pooled = L.tap(fd, dev(lin), pool)
    a, b = torch.from_numpy(f[:N]).double(), torch.from_numpy(f[N:]).double()
    na = a / (a.pow(2).sum(-1, keepdim=True).sqrt() + 1e-10)
    nb = b / (b.pow(2).sum(-1, keepdim=True).sqrt() + 1e-10)
    want = ((na - nb).pow(2) * torch.from_numpy(lin).double()).sum((1, 2, 3)).numpy()
    got = sums.cpu().numpy()
    assert np.all(np.isfinite(got)) and want.max() > 0
    assert float(np.max(np.abs(got - want))) <= 1e-12 * float(want.max())
    if pool:
        wantp = F.max_pool2d(torch.from_numpy(f).permute(0, 3, 1, 2), 3, 2).permute(0, 2, 3, 1)
        assert pooled.shape == wantp.shape and torch.equal(pooled.cpu(), wantp)
    else:
        assert pooled is None
    # an all-zero lin vector, and identical maps
    zero, _ = L.tap(fd, torch.zeros(C, device="cuda"), False)
    same, _ = L.tap(torch.cat((fd[:N], fd[:N])), dev(lin), False)
    assert not zero.any() and not same.any()


def test_chunk_invariance():
    """A slice's value depends neither on the chunk it was in nor on its neighbours, bit for bit."""
    t, p = volumes((5, 35, 47))
    dt, dp = dev(t), dev(p)
    runs = [G.lpips_taps(dt, dp, weights(), chunk=c) for c in (1, 2, 5, 5)]
    for r in runs[1:]:
        assert np.array_equal(r, runs[0])
    # slice 3 without its neighbours, re-normalised by the volume's extrema as it was among them
    st = G.PairStats(dt, dp)
    aff = (float(st.amin), float(G._rng32(st.amin, st.amax) + M.EPS32), float(st.bmin), float(G._rng32(st.bmin, st.bmax) + M.EPS32))
    one = L.tap_sums(dt[3:4].contiguous(), dp[3:4].contiguous(), aff, weights()).cpu().numpy()
    counts = np.array([h * w for h, w in LW.out_sizes(35, 47)], np.float64)
    assert np.array_equal(one[:, 0] / counts, runs[0][:, 3])


def test_agreement_with_the_host():
    t, p = volumes((3, 35, 47))
    raw_t, raw_p = (t * 2500 - 1000).astype(np.float32), (p * 2400 - 900).astype(np.float32)
    bar, _ = bars()
    host_m, host_l = M.evaluate_patient(raw_t, raw_p, lpips_weights=weights())
    dev_m, dev_l = G.evaluate_patient(raw_t, raw_p, device="cuda", lpips_weights=weights())
    off_m, off_l = G.evaluate_patient(raw_t, raw_p, device="cuda")
    assert list(dev_m) == list(host_m) == list(M.METRICS)
    for k in M.METRICS:
        assert len(dev_l[k]) == len(host_l[k]) and len(dev_m[k]) == len(host_m[k])
        for got, want in zip(dev_l[k], host_l[k]):
            assert len(got) == len(want)
            for g, w in zip(got, want):
                if k == "lpips":
                    assert abs(g - w) <= bar * w and w > 0
                elif k.startswith("ssim"):
                    assert abs(g - w) <= SSIM_ATOL, k
                elif math.isinf(w):
                    assert g == w, k
                else:
                    assert abs(g - w) <= RTOL * abs(w), k
        if k != "lpips":   # with lpips_weights=None the device result is what it is without the keyword
            assert np.array_equal(np.array(off_m[k]), np.array(dev_m[k]), equal_nan=True), k
            assert off_l[k] == dev_l[k], k
    assert len(dev_l["lpips"]) == 1 and len(dev_l["lpips"][0]) == 3
    assert abs(dev_m["lpips"][0] - host_m["lpips"][0]) <= bar * host_m["lpips"][0]
    assert math.isnan(off_m["lpips"][0]) and off_l["lpips"] == [[]]


def test_below_the_minimum_size_nothing_is_launched(monkeypatch):
    calls = []
    real = lib.call
    monkeypatch.setattr(lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    x = torch.rand(2, 30, 64, device="cuda")
    y = torch.rand(2, 30, 64, device="cuda")
    agg, lst = G.lpips(x, y, weights())
    assert math.isnan(agg) and lst == [] and calls == []
    out = G.evaluate_pair(x, y, "cuda", lpips_weights=weights())
    assert math.isnan(out["lpips"][0]) and out["lpips"][1] == []
    assert not any(n.startswith("dcs_lpips") or n in ("dcs_conv_rows", "dcs_met_normalize") for n in calls)
    with pytest.raises(ValueError):
        G.lpips_taps(x, y, weights())
    with pytest.raises(RuntimeError):
        G.lpips_taps(torch.rand(2, 40, 40), torch.rand(2, 40, 40), weights())    # host tensors
    # the C entry points refuse bad calls before any launch
    plan = L.plan_for(weights(), "cuda")
    out = torch.zeros(2, 6, 15, 64, device="cuda")
    ptr = lambda v: v.data_ptr()
    with pytest.raises(lib.HipLibraryError, match="1001"):
        real("dcs_lpips_stem", ptr(x), 2, 10, 64, 0.0, 1.0, ptr(plan.wx), ptr(plan.cb), ptr(out), None)    # H = 10
    with pytest.raises(lib.HipLibraryError, match="1001"):
        real("dcs_lpips_stem", ptr(x), 2, 30, 64, 0.0, 0.0, ptr(plan.wx), ptr(plan.cb), ptr(out), None)    # div = 0
    f = torch.zeros(2, 3, 3, 64, device="cuda")
    s = torch.zeros(1, dtype=torch.float64, device="cuda")
    ws = torch.zeros(4, dtype=torch.float64, device="cuda")
    with pytest.raises(lib.HipLibraryError, match="1001"):
        real("dcs_lpips_tap", ptr(f[:1]), ptr(f[1:]), 1, 3, 3, 60, ptr(plan.lins[0]), None, None, ptr(s), ptr(ws), 32, None)
    with pytest.raises(lib.HipLibraryError, match="1002"):
        real("dcs_lpips_tap", ptr(f[:1]), ptr(f[1:]), 1, 3, 3, 64, ptr(plan.lins[0]), None, None, ptr(s), ptr(ws), 4, None)
    assert not out.any() and not s.any()
    torch.cuda.synchronize()


def test_calculate_on_the_device(tmp_path):
    """A three-slice 32 x 32 patient through calculate.py --device cuda --lpips_weights, in this process:
    the column, the pickle entry and the summary row hold the device's values, within the bar of the host's."""
    import calculate
    from modules import dicom
    rng = np.random.default_rng(29)
    base = rng.integers(900, 1200, (3, 32, 32)).astype(np.int16)
    series = {"std": base, "generated": (base + rng.integers(0, 60, base.shape)).astype(np.int16)}
    dirs = {"std": tmp_path / "in" / "DS" / "P1" / "POST STD", "generated": tmp_path / "out" / "DS" / "P1"}
    for cat, vol in series.items():
        dirs[cat].mkdir(parents=True)
        for i in range(3):
            ds = dicom.new_ct_slice(vol[i], instance=i + 1, uid_suffix=f"{i}")
            ds.ImagePositionPatient = [0.0, 0.0, 2.5 * i]
            ds.save_as(str(dirs[cat] / f"{i:03d}.dcm"))
    wpath = tmp_path / "w.pth"
    torch.save(LW.random_state_dict(3), wpath)
    calculate.main(["--input_dir_root", str(tmp_path / "in"), "--output_dir_root", str(tmp_path / "out"),
                    "--dataset_names", "DS", "--device", "cuda", "--lpips_weights", str(wpath)])
    calc = tmp_path / "out" / "calculated"
    tn, pn = (M.normalize(series[k].astype(np.float32) - 1024) for k in ("std", "generated"))
    want = M.lpips(tn, pn, weights(), dtype=torch.float64)
    bar, _ = bars()
    cells = [float(r["lpips_STD_vs_Generated"]) for r in csv.DictReader(open(calc / "detail" / "DS_P1_metrics.csv"))]
    assert cells == G.lpips(dev(tn), dev(pn), weights())[1] and len(cells) == 3
    assert rel(cells, want[1]) <= bar
    summary = pickle.load(open(calc / "result_all_metrics.pkl", "rb"))
    assert summary["lpips"] == [[float(np.mean(cells))]]
    stats = {s["Metric"]: s for s in csv.DictReader(open(calc / "summary_statistics.csv"))}
    assert stats["lpips_STD_vs_Generated"]["Count"] == "3"
