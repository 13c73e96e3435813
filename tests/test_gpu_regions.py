"""Region-wise evaluation on the GPU (csrc/metrics.hip: region_kernel, region_ssim_kernel;
modules/hip/metrics.py; modules/metrics_gpu.py::region_metrics; calculate.py --regions --device cuda)
against the host path modules/metrics.py.

Bars.  Counts: equal.  Non-negative sums: relative 1e-10 (two orders of N <= 1e5 float64 terms
differ by at most N * 2^-53; every slice here has fewer than 1e5 voxels).  Signed sums:
|delta| <= 1e-10 * the float64 sum of the absolute values of the same terms, computed here on the
host.  SSIM sums over their counts: absolute 1e-10, the per-slice SSIM bar; a region averages
fewer pixels than a slice, so the bar rests on a per-pixel condition asserted here on the host: two
float64 evaluation orders of the map (scipy's running sums, a direct 49-tap sum) differ by at most
9e-13 per pixel on these volumes.
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
from modules import metrics as M
from modules import metrics_gpu as G
from modules.hip import lib
from modules.hip import metrics as K
from test_cpu_regions import AIR, CHEST, COUNT_COLS, EXPECTED_HEADER, SPEC, hu_triple, phantom_triple, write_cli_tree

pytestmark = pytest.mark.gpu

RTOL = 1e-10
SSIM_ATOL = 1e-10
PIXEL_ATOL = 9e-13
# (2,70,300): 2-3 x 5 SSIM tiles and more than 8192 voxels (DCS_MET_PAIR_CHUNK) per slice, so
# several blocks per slice of the one-pass kernel; (5,61,67): an odd slice size takes its scalar path
assert (K.TILE_X, K.TILE_Y, lib.MET_PAIR_CHUNK) == (64, 32, 8192)
SHAPES = [(2, 7, 7), (3, 33, 65), (2, 70, 300), (5, 61, 67)]
CASES = SHAPES + ["phantom"]
NONNEG = [1, 2, 5, 6, 9, 10, 13, 14, 19]          # sum|d| and sum d^2 per region; std - vue > thr > 0 over enh
SIGNED = [3, 7, 11, 15, 20]                      # sum (gen - std) per region, sum (gen - vue) over enh


@functools.lru_cache(maxsize=None)
def triple(case):
    return phantom_triple() if case == "phantom" else hu_triple(case, 3, round_noise=False)


@functools.lru_cache(maxsize=None)
def host(case):
    """The host arrays of one case, computed once and shared."""
    v, s, g = triple(case)
    sums, ss = M.region_sums(v, s, g), M.region_ssim_sums(v, s, g)
    sums.setflags(write=False)
    ss.setflags(write=False)
    return sums, ss


def dev(x):
    return torch.from_numpy(np.array(x)).cuda()


def abs_sums(v, s, g, spec=SPEC):
    """S_abs of the signed columns: the float64 sums of |gen - std| per region and of |gen - vue| over enh."""
    masks, _ = M.region_masks(v, s, g, spec)
    flat = lambda x, m, z: np.abs(x[z][m[z]]).astype(np.float64).sum()
    out = np.zeros((v.shape[0], 5))
    for z in range(v.shape[0]):
        out[z, :4] = [flat(g - s, m, z) for m in masks]
        out[z, 4] = flat(g - v, masks[3], z)
    return out


def ssim_map_direct(s1, s2, data_range):
    """The SSIM map in another float64 order: symmetric padding and a direct 49-term sum."""
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
    return ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux ** 2 + uy ** 2 + c1) * (vx + vy + c2))


def check_arrays(got, want, sabs, got_ss, want_ss):
    assert got.shape == want.shape and got_ss.shape == want_ss.shape
    assert np.array_equal(got[:, COUNT_COLS], want[:, COUNT_COLS])
    err = np.abs(got - want)
    print("max rel err, non-negative sums", (err[:, NONNEG] / np.maximum(want[:, NONNEG], 1e-300)).max())
    print("max err / S_abs, signed sums", (err[:, SIGNED] / np.maximum(sabs, 1e-300)).max())
    assert np.all(want[:, NONNEG] >= 0)
    assert np.all(err[:, NONNEG] <= RTOL * want[:, NONNEG])
    assert np.all(err[:, SIGNED] <= RTOL * sabs)
    assert np.array_equal(got_ss[:, 0::2], want_ss[:, 0::2])
    cnt = np.maximum(want_ss[:, 0::2], 1)
    serr = np.abs(got_ss[:, 1::2] - want_ss[:, 1::2]) / cnt
    print("max abs err, region SSIM means", serr.max())
    assert np.all(serr <= SSIM_ATOL)


@pytest.mark.parametrize("case", CASES, ids=[c if isinstance(c, str) else "x".join(map(str, c)) for c in CASES])
def test_device_arrays_against_host(case):
    v, s, g = triple(case)
    want, want_ss = host(case)
    if case == "phantom":
        assert all(want[z, 4 * r] > 0 for z in CHEST for r in range(4))
        assert all(want[z, [0, 4, 8, 12]].tolist() == [0, 0, 4096, 0] for z in AIR)
    elif case != (2, 7, 7):                               # every region and every overlap count occurs
        assert want[:, COUNT_COLS].sum(axis=0).min() > 0
    # the per-pixel condition the SSIM bar rests on, on the host
    dr = float(g.max() - g.min())
    pix = max(np.abs(M.ssim_map(a, b, dr) - ssim_map_direct(a, b, dr))[3:-3, 3:-3].max() for a, b in zip(s, g))
    print("two host orders of the map, max per pixel", pix)
    assert pix <= PIXEL_ATOL
    dv, ds, dg = dev(v), dev(s), dev(g)
    got, rmap = K.region_sums(dv, ds, dg, SPEC.ranges())
    masks, _ = M.region_masks(v, s, g)
    owner = np.where(masks[0], 0, np.where(masks[1], 1, 2)) | (masks[3] * 4)
    assert rmap.dtype == torch.uint8 and np.array_equal(rmap.cpu().numpy(), owner.astype(np.uint8))
    st = G.PairStats(ds, dg)
    assert float(G._rng32(st.bmin, st.bmax)) == dr
    got_ss = K.region_ssim_sums(ds, dg, rmap, dr)
    check_arrays(got.cpu().numpy(), want, abs_sums(v, s, g), got_ss.cpu().numpy(), want_ss)
    # without the map the sums are the same bits
    again, none = K.region_sums(dv, ds, dg, SPEC.ranges(), with_map=False)
    assert none is None and torch.equal(again, got)
    # the driver: the same arrays, and the shared derivation
    a, b, peak = G.region_arrays(dv, ds, dg)
    assert np.array_equal(a, got.cpu().numpy()) and np.array_equal(b, got_ss.cpu().numpy())
    assert peak == M.max_pixel_of(s.min(), s.max())
    agg, per = G.region_metrics(s, g, v, device="cuda")
    wagg, wper = M.region_metrics(s, g, v)
    for k in M.REGION_COLUMNS:
        x, y = np.array([agg[k]] + per[k], np.float64), np.array([wagg[k]] + wper[k], np.float64)
        assert np.array_equal(np.isnan(x), np.isnan(y)), k
    if case == "phantom":
        assert all(math.isnan(per["mae_lung"][z]) and math.isnan(per["dice_enh"][z]) for z in AIR)


def test_one_region_equals_the_slice_ssim():
    """With lung everywhere the region SSIM mean is the slice SSIM of metrics_gpu.ssim."""
    v, s, g = (dev(x) for x in hu_triple((2, 70, 300), 3, round_noise=False))
    everything = M.RegionSpec(lung_min=-1e6, lung_max=1e6)
    sums, rmap = K.region_sums(v, s, g, everything.ranges())
    assert int((rmap & 3).max()) == 0
    _, slices = G.ssim(s, g)
    st = G.PairStats(s, g)
    ss = K.region_ssim_sums(s, g, rmap, float(G._rng32(st.bmin, st.bmax))).cpu().numpy()
    assert ss[:, 0].tolist() == [64 * 294] * 2 and np.all(ss[:, 2:6] == 0)
    err = np.abs(ss[:, 1] / ss[:, 0] - np.array(slices))
    print("region mean against slice SSIM", err.max())
    assert np.all(err <= SSIM_ATOL)
    h = sums.cpu().numpy()
    assert h[:, 0].tolist() == [70 * 300] * 2 and np.all(h[:, 4:12] == 0)
    pair = K.pair_stats(s, g).cpu().numpy()
    assert np.all(np.abs(h[:, 1] - pair[:, K.SUM_ABS]) <= RTOL * pair[:, K.SUM_ABS])


def test_a_side_below_seven_has_no_ssim_cell():
    v, s, g = (np.ascontiguousarray(x[:, :6, :]) for x in hu_triple((3, 33, 65), 3, round_noise=False))
    agg, per = G.region_metrics(s, g, v, device="cuda")
    wagg, wper = M.region_metrics(s, g, v)
    assert all(math.isnan(agg[f"ssim_{r}"]) and all(math.isnan(x) for x in per[f"ssim_{r}"]) for r in M.REGIONS)
    assert per["n_lung"] == wper["n_lung"] and per["n_enh"] == wper["n_enh"] and agg["n_rest"] == wagg["n_rest"]
    assert abs(agg["mae_soft"] - wagg["mae_soft"]) <= RTOL * wagg["mae_soft"]


def test_run_to_run_bit_identical():
    for case in ((2, 70, 300), (5, 61, 67)):
        v, s, g = (dev(x) for x in hu_triple(case, 3, round_noise=False))
        a, ma = K.region_sums(v, s, g, SPEC.ranges())
        b, mb = K.region_sums(v, s, g, SPEC.ranges())
        assert torch.equal(a, b) and torch.equal(ma, mb)
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
        x, y = K.region_ssim_sums(s, g, ma, 2500.0), K.region_ssim_sums(s, g, ma, 2500.0)
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


def test_bad_arguments_raise():
    v, s, g = (dev(x) for x in hu_triple((3, 33, 65), 3, round_noise=False))
    rng = SPEC.ranges()
    _, rmap = K.region_sums(v, s, g, rng)
    with pytest.raises(ValueError):
        K.region_sums(v.cpu(), s, g, rng)                    # host tensor
    with pytest.raises(ValueError):
        K.region_sums(v, s.double(), g, rng)                 # float64
    with pytest.raises(ValueError):
        K.region_sums(v, s, g[:, :, :60].contiguous(), rng)  # mismatched shapes
    with pytest.raises(ValueError):
        K.region_sums(v, s.transpose(1, 2).contiguous().transpose(1, 2), g, rng)   # not contiguous
    with pytest.raises(ValueError):
        K.region_sums(v, s, g, rng[:5])
    with pytest.raises(ValueError):
        K.region_ssim_sums(s.cpu(), g, rmap, 1.0)
    with pytest.raises(ValueError):
        K.region_ssim_sums(s, g.double(), rmap, 1.0)
    with pytest.raises(ValueError):
        K.region_ssim_sums(s, g, rmap[:2], 1.0)
    with pytest.raises(ValueError):
        K.region_ssim_sums(s, g, rmap.float(), 1.0)
    with pytest.raises(ValueError):
        K.region_ssim_sums(s[:, :, ::2], g[:, :, ::2], rmap[:, :, ::2], 1.0)
    small = s[:, :6, :].contiguous()
    with pytest.raises(ValueError):
        K.region_ssim_sums(small, small, rmap[:, :6, :].contiguous(), 1.0)
    # the C entry points refuse the same calls before any launch
    out = torch.zeros(3 * 21, dtype=torch.float64, device="cuda")
    ws = torch.zeros(256, dtype=torch.float64, device="cuda")
    ptr = lambda x: x.data_ptr()
    need = lib.query("dcs_met_region_workspace_size", 3, 33, 65)
    assert need == 8 * 3 * 21 and lib.query("dcs_met_region_workspace_size", 0, 33, 65) == 0
    assert lib.query("dcs_met_region_workspace_size", 2, 70, 300) == 8 * 2 * 10 * 8       # 2 x 5 tiles of 8 outgrow 3 chunks of 21
    bad = (ctypes.c_float * 6)(-1000, -150, -150, 250, float("nan"), -400)
    good = (ctypes.c_float * 6)(*rng)
    with pytest.raises(lib.HipLibraryError, match="1001"):
        lib.call("dcs_met_region_sums", ptr(v), ptr(s), ptr(g), 3, 33, 65, bad, ptr(out), None, ptr(ws), need, None)
    with pytest.raises(lib.HipLibraryError, match="1001"):
        lib.call("dcs_met_region_sums", None, ptr(s), ptr(g), 3, 33, 65, good, ptr(out), None, ptr(ws), need, None)
    with pytest.raises(lib.HipLibraryError, match="1002"):
        lib.call("dcs_met_region_sums", ptr(v), ptr(s), ptr(g), 3, 33, 65, good, ptr(out), None, ptr(ws), need - 8, None)
    with pytest.raises(lib.HipLibraryError, match="1001"):
        lib.call("dcs_met_region_ssim", ptr(s), ptr(g), ptr(rmap), 3, 6, 65, 1.0, ptr(out), ptr(ws), need, None)
    with pytest.raises(lib.HipLibraryError, match="1001"):
        lib.call("dcs_met_region_ssim", ptr(s), ptr(g), None, 3, 33, 65, 1.0, ptr(out), ptr(ws), need, None)
    with pytest.raises(lib.HipLibraryError, match="1002"):
        lib.call("dcs_met_region_ssim", ptr(s), ptr(g), ptr(rmap), 3, 33, 65, 1.0, ptr(out), ptr(ws), 8, None)
    torch.cuda.synchronize()


def _run_calculate(tmp_path, device):
    out = tmp_path / f"out_{device}"
    cmd = [sys.executable, os.path.join(PKG, "calculate.py"), "--input_dir_root", str(tmp_path / "in"),
           "--output_dir_root", str(out), "--dataset_names", "DS", "--device", device, "--regions"]
    subprocess.run(cmd, check=True, timeout=300, stdout=subprocess.DEVNULL)
    return out / "calculated"


def test_calculate_regions_on_both_devices(tmp_path):
    """calculate.py --regions with --device cuda and --device cpu, a fresh child process each: the
    same region CSV cell for cell at the bars above, empty cells in the same places, and the
    ordinary files of the cuda run next to the new ones."""
    series = write_cli_tree(tmp_path, ("out_cuda", "out_cpu"))
    sabs = abs_sums(series["vue"], series["std"], series["generated"])
    calc = {d: _run_calculate(tmp_path, d) for d in ("cuda", "cpu")}
    rows = {d: list(csv.reader(open(calc[d] / "regions" / "DS_P1_regions.csv"))) for d in calc}
    assert rows["cuda"][0] == rows["cpu"][0] == EXPECTED_HEADER and len(rows["cuda"]) == len(rows["cpu"]) == 4
    saw_empty = False
    for i in range(1, 4):
        for name, g, w in zip(rows["cpu"][0], rows["cuda"][i], rows["cpu"][i]):
            if w == "" or g == "":
                assert g == w == "", (name, i)
                saw_empty = True
            elif name == "Slice_Idx" or name.startswith("n_"):
                assert g == w, (name, i)
            elif name.startswith("ssim"):
                assert abs(float(g) - float(w)) <= SSIM_ATOL, (name, i)
            elif name.startswith(("bias", "enh_pred")):     # means of signed sums: against S_abs over the count
                r = 4 if name.startswith("enh_pred") else M.REGIONS.index(name.rsplit("_", 1)[1])
                n = int(rows["cpu"][i][rows["cpu"][0].index("n_" + name.rsplit("_", 1)[1])])
                assert abs(float(g) - float(w)) <= RTOL * sabs[i - 1, r] / n, (name, i)
            else:
                assert abs(float(g) - float(w)) <= RTOL * abs(float(w)), (name, i)
    assert saw_empty                                        # 16 x 16 slices have cells without lung or soft SSIM pixels
    for d in calc:
        assert not (calc[d] / "regions" / "DS_P2_regions.csv").exists()
        for name in ("detail/DS_P1_metrics.csv", "detail/DS_P2_metrics.csv", "result_all_metrics.pkl",
                     "summary_statistics.csv", "result_region_metrics.pkl", "summary_statistics_regions.csv"):
            assert (calc[d] / name).exists(), (d, name)
