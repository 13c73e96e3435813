#!/usr/bin/env python
"""Host against device timing of calculate.py's per-patient metrics (modules/metrics_gpu.py::evaluate_patient).

    python scripts/bench_metrics.py [--shape 128x512x512] [--reps 5] [--host_reps 5] [--skip_host] [--ms_ssim]
                                    [--lpips_weights PATH[,PATH]|random] [--regions]

One synthetic patient from modules/phantom.py (STD, a generated series = STD + rounded N(0, 20),
a VUE series) goes through
  * the host path (``device=None``: numpy / scipy of modules/metrics.py, this process's threads),
    median of --host_reps after one warm-up;
  * the device path end to end: upload of the three float32 series, kernels, download of the
    per-slice vectors, median of --reps after one warm-up;
  * every kernel alone on resident volumes, from HIP events, median of --reps after one warm-up,
    with its algorithmic bytes (both volumes read once, 8 bytes per voxel) over that time as a
    share of the 8 TB/s HBM peak.
The two paths' results are compared at the bars of tests/test_gpu_metrics.py.  Prints progress
lines and, last, one JSON line.

--ms_ssim turns the MS-SSIM switch of evaluate_patient on in every leg above (its column is then
compared at 1e-9 absolute, the bar of tests/test_gpu_msssim.py), and adds under "ms_ssim" the
metric alone on the STD / generated pair: host time, device time end to end and on resident
volumes, and the event time of the level kernel at each of the five levels and of the pooling
kernel between them (the level kernel reads both volumes once: 8 bytes per voxel of its level;
the pooling kernel reads both and writes a quarter: 10 bytes per input voxel).

--lpips_weights turns LPIPS on in every leg (its column is compared at 1e-5 relative: both paths hold
4 x the float32 ATen error against float64, tests/test_gpu_lpips.py, which is below that) and adds
under "lpips" the metric alone on the STD / generated pair: the host time (ATen, float32), the same
ATen restatement on the device in float32 on resident volumes (and its convolutions alone, layer
by layer), the HIP path end to end and resident, the event time of every launch of one resident run
summed per kernel and layer, and the
patient end to end and resident without the switch.  ``random`` takes the seeded stand-in weights
of the tests (modules/lpips_weights.py::random_state_dict).

--regions adds under "regions" the region-wise evaluation of calculate.py --regions on the same
patient (it changes no other leg): the host time, the device time end to end (upload of the three
series included) and on resident series, each as median, min and max of the repeats, the event time
of its two kernels next to pair_stats from the same run (region_sums reads three series and writes
the region byte: 13 bytes per voxel, 12 without the map; region_ssim reads two series and the byte:
9), and the two paths' raw arrays compared at the bars of tests/test_gpu_regions.py.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "ducosy-gan_amd"))

from modules import lpips_weights as LW  # noqa: E402
from modules import metrics as M  # noqa: E402
from modules import metrics_gpu as G  # noqa: E402
from modules import phantom  # noqa: E402
from modules.hip import metrics as K  # noqa: E402
from modules.hip import unet as U  # noqa: E402  (the launch timer the LPIPS driver shares)

HBM_PEAK = 8.0e12


def patient(shape, seed=0):
    d, h, w = shape
    assert h == w, "the phantom draws square slices"
    raw, slope, inter = phantom.ct_batch(seed, d, h, kinds=["chest"])
    std = raw.astype(np.float32) * slope[:, None, None] + inter[:, None, None]
    rng = np.random.default_rng(seed + 1)
    gen = (std + np.round(rng.normal(0, 20, std.shape))).astype(np.float32)
    vue = (std - np.where((std > 200) & (std < 400), 250, 0) + np.round(rng.normal(0, 10, std.shape))).astype(np.float32)
    return std, gen, vue


def _events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def _median_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    return statistics.median(_events(fn) for _ in range(reps))


def kernel_times(std, gen, reps):
    """Event time of every kernel on one resident pair, with its share of the HBM peak."""
    t, p = std, gen
    st = K.pair_stats(t, p)
    aff = G.PairStats(t, p).normalize_affine()
    D = t.shape[0]
    sa = torch.sort(t.reshape(D, -1), dim=1).values.reshape(t.shape)
    sb = torch.sort(p.reshape(D, -1), dim=1).values.reshape(p.shape)
    runs = {
        "pair_stats": lambda: K.pair_stats(t, p),
        "pair_stats_norm": lambda: K.pair_stats(t, p, aff),
        "ssim": lambda: K.ssim_sums(t, p, 2500.0),
        "ssim_norm": lambda: K.ssim_sums(t, p, 1.0, aff),
        "sobel_ts": lambda: K.sobel_ts(t, p),
        "ed": lambda: K.ed_sums(t, p, st),
        "sorted_l1": lambda: K.sorted_l1(sa, sb, (-1024.0, 4000.0, -1024.0, 4000.0)),
        "torch_sort_x2": lambda: (torch.sort(t.reshape(D, -1), dim=1), torch.sort(p.reshape(D, -1), dim=1)),
    }
    nbytes = 8 * t.numel()
    out = {}
    for name, fn in runs.items():
        ms = _median_ms(fn, reps)
        out[name] = {"ms": round(ms, 4)}
        if name != "torch_sort_x2":
            out[name]["algorithmic_GBps"] = round(nbytes / ms / 1e6, 1)
            out[name]["share_of_hbm_peak"] = round(nbytes / (ms * 1e-3) / HBM_PEAK, 3)
    return out


def ms_ssim_times(std, gen, reps):
    """Event time of the MS-SSIM kernels on the resident pair, level by level."""
    out = {}
    levels = G.ms_ssim_pyramid(std, gen)
    for i, (x, y) in enumerate(levels):
        runs = {f"msssim_level{i}": (lambda: K.msssim_level_sums(x, y, M.MS_SSIM_WINDOW, M.MS_SSIM_C1, M.MS_SSIM_C2),
                                     8 * x.numel())}
        if i + 1 < len(levels):
            runs[f"pool2_level{i}"] = (lambda: K.pool2(x, y), 10 * x.numel())
        for name, (fn, nbytes) in runs.items():
            ms = _median_ms(fn, reps)
            out[name] = {"ms": round(ms, 4), "shape": "x".join(str(v) for v in x.shape),
                         "algorithmic_GBps": round(nbytes / ms / 1e6, 1),
                         "share_of_hbm_peak": round(nbytes / (ms * 1e-3) / HBM_PEAK, 3)}
    return out


def lpips_aten_device(tn, pn, wdev, step=16):
    """The host restatement (modules/metrics.py) with ATen on the device in float32, resident volumes."""
    def chain(x):
        mn, mx = x.min(), x.max()
        return (x - mn) / ((mx - mn) + 1e-8) * 2 - 1
    xa, xb = chain(tn), chain(pn)
    vals = []
    with torch.no_grad():
        for i in range(0, xa.shape[0], step):
            fa, fb = M.lpips_features(xa[i:i + step], wdev), M.lpips_features(xb[i:i + step], wdev)
            vals.append(sum(M.lpips_tap(fa[k], fb[k], lin) for k, lin in enumerate(wdev.lins)))
    return torch.cat(vals).double().cpu().numpy()


def lpips_aten_conv_times(D, H, W, wdev, reps, step=16):
    """ATen's float32 convolution of every layer alone (bias included, no ReLU), per patient: the event
    time of one call on ``step`` maps times the 2 * D / step calls of lpips_aten_device."""
    import torch.nn.functional as F
    out, (h, w) = {}, (H, W)
    for k, (co, ci, ks, stride, pad, pool) in enumerate(LW.CONVS):
        if pool:
            h, w = (h - 3) // 2 + 1, (w - 3) // 2 + 1
        x = torch.rand(step, ci, h, w, device=wdev.lins[0].device)
        wt, b = wdev.convs[k]
        ms = _median_ms(lambda: F.conv2d(x, wt, b, stride=stride, padding=pad), reps)
        h, w = (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1
        out[f"conv{ks}x{ks} {ci}->{co} @{h}x{w}"] = round(ms * 2 * D / step, 3)
    return out


def lpips_kernel_times(tn, pn, weights):
    """Event time of every launch of one resident run, summed per label (kernel, layer and map size)."""
    G.lpips(tn, pn, weights)
    torch.cuda.synchronize()
    U.TIMES = []
    G.lpips(tn, pn, weights)
    torch.cuda.synchronize()
    out = {}
    for label, a, b in U.TIMES:
        out[label] = out.get(label, 0.0) + a.elapsed_time(b)
    U.TIMES = None
    return {k: round(v, 3) for k, v in out.items()}


def _spread(times, scale=1.0, digits=4):
    return {"median": round(statistics.median(times) * scale, digits), "min": round(min(times) * scale, digits),
            "max": round(max(times) * scale, digits)}


def region_times(std, gen, vue, ds, dg, dv, dev, reps, host_reps, skip_host):
    """calculate.py --regions on the patient: both paths, the two kernels, and their agreement."""
    spec = M.RegionSpec()

    def end_to_end():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = G.region_metrics(std, gen, vue, device=dev, spec=spec)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    end_to_end()
    out = {"device_end_to_end_s": _spread([end_to_end()[0] for _ in range(reps)])}
    resident = lambda: G.region_metrics(ds, dg, dv, device=dev, spec=spec)
    resident()
    torch.cuda.synchronize()
    out["device_resident_ms"] = _spread([_events(resident) for _ in range(reps)], digits=3)
    sums, rmap = K.region_sums(dv, ds, dg, spec.ranges())
    runs = {"pair_stats": (lambda: K.pair_stats(ds, dg), 8),
            "region_sums": (lambda: K.region_sums(dv, ds, dg, spec.ranges()), 13),
            "region_sums_no_map": (lambda: K.region_sums(dv, ds, dg, spec.ranges(), with_map=False), 12),
            "ssim": (lambda: K.ssim_sums(ds, dg, 2500.0), 8),
            "region_ssim": (lambda: K.region_ssim_sums(ds, dg, rmap, 2500.0), 9)}
    out["kernels"] = {}
    for fn, _ in runs.values():
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in runs}
    for _ in range(max(reps, 10)):                        # interleaved rounds: the kernels share the clock's drift
        for name, (fn, _) in runs.items():
            times[name].append(_events(fn))
    for name, (_, bpv) in runs.items():
        sp = _spread(times[name], digits=4)
        nbytes = bpv * ds.numel()
        out["kernels"][name] = {"ms": sp, "bytes_per_voxel": bpv,
                                "algorithmic_GBps": {k: round(nbytes / v / 1e6, 1) for k, v in sp.items()}}
    if not skip_host:
        times = []
        for i in range(host_reps + 1):
            t0 = time.perf_counter()
            M.region_metrics(std, gen, vue, spec)
            times.append(time.perf_counter() - t0)
            print(f"host regions run {i}{' (warm-up)' if i == 0 else ''}: {times[-1]:.2f} s", flush=True)
        out["host_s"] = _spread(times[1:], digits=3)
        want, want_ss = M.region_sums(vue, std, gen, spec), M.region_ssim_sums(vue, std, gen, spec)
        got, got_ss, _ = G.region_arrays(dv, ds, dg, spec)
        counts = [0, 4, 8, 12, 16, 17, 18]
        nonneg = [1, 2, 5, 6, 9, 10, 13, 14, 19]
        err = np.abs(got - want)
        worst = {"counts_equal": bool(np.array_equal(got[:, counts], want[:, counts])
                                      and np.array_equal(got_ss[:, 0::2], want_ss[:, 0::2])),
                 "rel_nonneg": float((err[:, nonneg] / np.maximum(want[:, nonneg], 1e-300)).max()),
                 "abs_signed_over_sum_abs": float((err[:, [3, 7, 11, 15]] / np.maximum(want[:, [1, 5, 9, 13]], 1e-300)).max()),
                 "ssim_mean_abs": float((np.abs(got_ss[:, 1::2] - want_ss[:, 1::2]) / np.maximum(want_ss[:, 0::2], 1)).max())}
        out["worst_error"] = worst
        out["agree"] = bool(worst["counts_equal"] and worst["rel_nonneg"] <= 1e-10
                            and worst["abs_signed_over_sum_abs"] <= 1e-10 and worst["ssim_mean_abs"] <= 1e-10)
        out["speedup_end_to_end"] = round(out["host_s"]["median"] / out["device_end_to_end_s"]["median"], 1)
        out["speedup_resident"] = round(out["host_s"]["median"] * 1e3 / out["device_resident_ms"]["median"], 1)
    return out


def _agree(got, want):
    worst = {"rel": 0.0, "ssim_abs": 0.0, "ms_ssim_abs": 0.0, "lpips_rel": 0.0}
    ok = True
    for k in M.METRICS:
        for gl, wl in zip(got[1][k], want[1][k]):
            g, w = np.array(gl, np.float64), np.array(wl, np.float64)
            ok &= g.shape == w.shape and np.array_equal(np.isfinite(g), np.isfinite(w))
            f = np.isfinite(w)
            if not f.any():
                continue
            err = np.abs(g[f] - w[f])
            if k == "lpips":
                worst["lpips_rel"] = max(worst["lpips_rel"], float((err / np.abs(w[f])).max()))
            elif k == "ms_ssim":
                worst["ms_ssim_abs"] = max(worst["ms_ssim_abs"], float(err.max()))
            elif k.startswith("ssim"):
                worst["ssim_abs"] = max(worst["ssim_abs"], float(err.max()))
            else:
                worst["rel"] = max(worst["rel"], float((err / np.maximum(np.abs(w[f]), 1e-300)).max()))
    return bool(ok and worst["rel"] <= 1e-10 and worst["ssim_abs"] <= 1e-10 and worst["ms_ssim_abs"] <= 1e-9
                and worst["lpips_rel"] <= 1e-5), worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="128x512x512")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host_reps", type=int, default=5)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--skip_host", action="store_true", help="device times only (no comparison)")
    ap.add_argument("--ms_ssim", action="store_true", help="with MS-SSIM in every leg, and its own times")
    ap.add_argument("--regions", action="store_true", help="add the region-wise evaluation's own times")
    ap.add_argument("--lpips_weights", default=None, metavar="PATH[,PATH]|random",
                    help="with LPIPS in every leg, and its own times; 'random': the tests' seeded stand-in weights")
    a = ap.parse_args()
    dev = torch.device(a.device)
    shape = tuple(int(x) for x in a.shape.split("x"))
    threads = min(16, len(os.sched_getaffinity(0)))
    torch.set_num_threads(threads)
    t0 = time.perf_counter()
    std, gen, vue = patient(shape)
    print(f"phantom patient {shape} in {time.perf_counter() - t0:.1f} s", flush=True)
    res = {"metric": "evaluate_patient_seconds", "device": torch.cuda.get_device_name(dev), "shape": a.shape,
           "host_threads": threads, "with_ms_ssim": a.ms_ssim, "with_lpips": a.lpips_weights is not None}
    lw = None
    if a.lpips_weights:
        lw = LW.from_state_dicts(LW.random_state_dict(3)) if a.lpips_weights == "random" else LW.load(a.lpips_weights)

    def device_run(weights=lw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = G.evaluate_patient(std, gen, vue, device=dev, ms_ssim=a.ms_ssim, lpips_weights=weights)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    device_run()
    times = []
    for i in range(a.reps):
        dt, got = device_run()
        times.append(dt)
        print(f"device run {i}: {dt:.4f} s", flush=True)
    res["device_end_to_end_s"] = round(statistics.median(times), 4)
    res["device_end_to_end_spread_s"] = _spread(times)

    ds, dg, dv = (G.to_device(v, dev) for v in (std, gen, vue))
    resident = lambda weights=lw: G.evaluate_patient(ds, dg, dv, device=dev, ms_ssim=a.ms_ssim, lpips_weights=weights)
    resident()
    torch.cuda.synchronize()
    times = [_events(resident) for _ in range(a.reps)]
    res["device_resident_ms"] = round(statistics.median(times), 3)
    res["device_resident_spread_ms"] = _spread(times, digits=3)
    res["kernels"] = kernel_times(ds, dg, a.reps)
    if a.ms_ssim:
        def alone():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            val = G.ms_ssim(G.to_device(std, dev), G.to_device(gen, dev))
            torch.cuda.synchronize()
            return time.perf_counter() - t0, val
        alone()
        runs = [alone() for _ in range(a.reps)]
        ms = {"device_end_to_end_s": round(statistics.median(r[0] for r in runs), 4), "device_value": runs[-1][1][0],
              "device_resident_ms": round(_median_ms(lambda: G.ms_ssim(ds, dg), a.reps), 3)}
        res["kernels"].update(ms_ssim_times(ds, dg, a.reps))
        res["ms_ssim"] = ms
    if a.regions:
        res["regions"] = region_times(std, gen, vue, ds, dg, dv, dev, a.reps, a.host_reps, a.skip_host)
        print("regions:", json.dumps(res["regions"]), flush=True)
    if lw is not None:
        def alone():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            val = G.lpips(G.normalize(G.to_device(std, dev)), G.normalize(G.to_device(gen, dev)), lw)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, val
        alone()
        runs = [alone() for _ in range(a.reps)]
        tn, pn = G.normalize(ds), G.normalize(dg)
        wdev = LW.LpipsWeights([(w.to(dev), b.to(dev)) for w, b in lw.convs], [l.to(dev) for l in lw.lins])
        aten = lpips_aten_device(tn, pn, wdev)   # warm-up: the library picks its kernels
        lp = {"device_end_to_end_s": round(statistics.median(r[0] for r in runs), 4), "device_value": runs[-1][1][0],
              "device_resident_ms": round(_median_ms(lambda: G.lpips(tn, pn, lw), a.reps), 3),
              "aten_device_f32_resident_ms": round(_median_ms(lambda: lpips_aten_device(tn, pn, wdev), a.reps), 3),
              "aten_device_f32_value": float(aten.mean()),
              "chunk_slices": G.L.default_chunk(*ds.shape),
              "kernels_ms_per_run": lpips_kernel_times(tn, pn, lw),
              "aten_conv_ms_per_run": lpips_aten_conv_times(*ds.shape, wdev, a.reps)}
        lp["hip_over_aten_resident"] = round(lp["aten_device_f32_resident_ms"] / lp["device_resident_ms"], 2)
        without = [device_run(None)[0] for _ in range(a.reps + 1)][1:]
        lp["patient_without_switch"] = {"device_end_to_end_s": round(statistics.median(without), 4),
                                        "device_resident_ms": round(_median_ms(lambda: resident(None), a.reps), 3)}
        res["lpips"] = lp
        print("lpips:", json.dumps(lp), flush=True)
        del tn, pn
    del ds, dg, dv
    print("device:", json.dumps({k: res[k] for k in ("device_end_to_end_s", "device_resident_ms")}), flush=True)

    if not a.skip_host:
        times = []
        for i in range(a.host_reps + 1):
            t0 = time.perf_counter()
            want = G.evaluate_patient(std, gen, vue, device=None, ms_ssim=a.ms_ssim, lpips_weights=lw)
            dt = time.perf_counter() - t0
            print(f"host run {i}{' (warm-up)' if i == 0 else ''}: {dt:.2f} s", flush=True)
            if i:
                times.append(dt)
        res["host_s"] = round(statistics.median(times), 3)
        res["agree"], res["worst_error"] = _agree(got, want)
        res["speedup_end_to_end"] = round(res["host_s"] / res["device_end_to_end_s"], 1)
        res["speedup_resident"] = round(res["host_s"] * 1e3 / res["device_resident_ms"], 1)
        if a.ms_ssim:
            times = []
            for i in range(a.host_reps + 1):
                t0 = time.perf_counter()
                val = M.ms_ssim(std, gen)
                times.append(time.perf_counter() - t0)
            res["ms_ssim"].update({"host_s": round(statistics.median(times[1:]), 3), "host_value": val[0],
                                   "abs_error": abs(val[0] - res["ms_ssim"]["device_value"])})
        if lw is not None:
            tn, pn = M.normalize(std), M.normalize(gen)
            times = []
            for i in range(a.host_reps + 1):
                t0 = time.perf_counter()
                val = M.lpips(tn, pn, lw)
                times.append(time.perf_counter() - t0)
                print(f"host lpips run {i}{' (warm-up)' if i == 0 else ''}: {times[-1]:.2f} s", flush=True)
            res["lpips"].update({"host_s": round(statistics.median(times[1:]), 3), "host_value": val[0],
                                 "rel_error": abs(val[0] - res["lpips"]["device_value"]) / val[0]})
    print(json.dumps(res))
    if not a.skip_host and not (res["agree"] and res.get("regions", {}).get("agree", True)):
        sys.exit(1)


if __name__ == "__main__":
    main()
