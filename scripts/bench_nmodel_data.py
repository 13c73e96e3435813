#!/usr/bin/env python
"""Timing of the training-set builder of the normal-map U-Net (prepare_nmodel_data.py) on one patient.

    python scripts/bench_nmodel_data.py [--shape 128x512x512] [--reps 10] [--patient_reps 3] [--skip_patient]

One synthetic patient: --distinct phantom slices (modules/phantom.py, int16, slopes 1 and 0.5)
repeated to the depth of --shape, a uint16 CECT (the NCCT in HU plus 60 HU in the soft tissue, N(0, 6)
noise and a few voxels above 4000), and a stand-in for the merged sCECT (its values do not matter
to the time).

  * The kernel (csrc/nmodel_data.hip through modules/hip/nmodel_data.py) on resident series, with
    the sCECT (16 bytes per voxel: 2 + 2 + 4 read, 4 + 4 written) and without it (12), and the same
    arithmetic composed from torch elementwise operations and reductions on the device, in one
    process, alternating round by round after a warm-up of each: HIP events around one call,
    median, min and max of --reps rounds, and the algorithm's bytes over that time against the
    8 TB/s HBM peak.  The composition's results are compared with the kernel's and the comparison is
    reported: vue and diff bit for bit, the counts equal, the sums' worst relative difference.  The
    run fails when vue differs, diff differs by more than one float32 rounding (ATen's division is
    not this project's to pin) or a sum by more than 1e-6.
  * The per-patient wall time of prepare_nmodel_data.py::build_dataset --against scect, split into
    read (DICOM files to stored arrays), translate (the resident pipeline with two seeded 9-block
    Generators, cin 3 and cin 2, at the slice size), targets (upload of both series and the kernel),
    download and save (np.save of both volumes and the per-slice CSV): the patient is written as a
    DICOM tree to a temporary directory and built --patient_reps + 1 times with --overwrite, the
    first a warm-up; wall clock around a device synchronise per step, the median of the rest.

Prints progress lines and, last, one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PKG = os.path.join(ROOT, "ducosy-gan_amd")
sys.path.insert(0, PKG)

from modules import dicom, phantom  # noqa: E402
from modules.hip import nmodel_data as ND  # noqa: E402
from modules.model import Generator  # noqa: E402

HBM_PEAK = 8.0e12
F = np.float32


def patient(shape, distinct, seed=0):
    """(ncct int16, sn, in, cect uint16, sc, ic, merged float32)"""
    d, h, w = shape
    assert h == w, "the phantom draws square slices"
    k = min(distinct, d)
    raw, sn, in_ = phantom.ct_batch(seed, k, h, kinds=["chest"])
    take = np.arange(d) % k
    raw, sn, in_ = raw[take], sn[take], in_[take]
    hu = raw.astype(F) * sn[:, None, None] + in_[:, None, None]
    rng = np.random.default_rng(seed + 1)
    soft = (hu > 0) & (hu < 200)
    c_hu = hu + np.where(soft, F(60), F(0)) + rng.normal(0, 6, hu.shape).astype(F)
    c_hu.reshape(d, -1)[:, :: h * w // 7] += 4500
    cect = np.clip(np.round(c_hu + 1024), 0, 65535).astype(np.uint16)
    merged = raw.astype(F) + np.where(soft, F(30.25), F(0))
    return raw, sn, in_, cect, np.ones(d, F), np.full(d, -1024.0, F), merged


def torch_composition(ncct, sn, in_, cect_bits, sc, ic, merged, thr=8.0):
    """The kernel's arithmetic from torch operations: float32 elementwise steps, float64 sums."""
    a, b, c, e = (v[:, None, None] for v in (sn, in_, sc, ic))
    x = ncct.float() * a + b
    y = (cect_bits.int() & 0xFFFF).float() * c + e
    g = x if merged is None else merged * a + b
    d = (y - g) / a
    x64, y64 = x.double(), y.double()
    s = lambda t: t.sum((1, 2))
    stats = torch.stack([torch.full((x.shape[0],), float(x.shape[1] * x.shape[2]), dtype=torch.float64, device=x.device),
                         s(d >= thr).double(), s(d < 0).double(), s(d > 4000).double(),
                         s(d.clamp(0, 4000).double()), s(d.abs().double()), s(x64), s(y64), s(x64 * x64), s(y64 * y64),
                         s(x64 * y64)], 1)
    return x, d, stats


def _events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def _spread(times, digits=4):
    return {"median": round(statistics.median(times), digits), "min": round(min(times), digits),
            "max": round(max(times), digits)}


def kernel_legs(p, dev, reps):
    ncct, sn, in_, cect, sc, ic, merged = p
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    dn, dc, dm = up(ncct), up(cect.view(np.int16)), up(merged)
    ds = [up(v) for v in (sn, in_, sc, ic)]
    runs = {"kernel": (lambda: ND.residual_targets(dn, ds[0], ds[1], dc, ds[2], ds[3], dm, cect_unsigned=True), 16),
            "kernel_no_merged": (lambda: ND.residual_targets(dn, ds[0], ds[1], dc, ds[2], ds[3], None, cect_unsigned=True), 12),
            "torch_composition": (lambda: torch_composition(dn, ds[0], ds[1], dc, ds[2], ds[3], dm), 16),
            "torch_composition_no_merged": (lambda: torch_composition(dn, ds[0], ds[1], dc, ds[2], ds[3], None), 12)}
    outs = {}
    for name, (fn, _) in runs.items():          # warm-up of every leg, and the results to compare
        outs[name] = fn()
    torch.cuda.synchronize()
    times = {name: [] for name in runs}
    for _ in range(reps):                        # interleaved rounds: the legs share the clock's drift
        for name, (fn, _) in runs.items():
            times[name].append(_events(fn))
    res = {}
    for name, (_, bpv) in runs.items():
        sp = _spread(times[name])
        nbytes = bpv * dn.numel()
        res[name] = {"ms": sp, "bytes_per_voxel": bpv,
                     "algorithmic_GBps": {k: round(nbytes / v / 1e6, 1) for k, v in sp.items()},
                     "share_of_hbm_peak": round(nbytes / (sp["median"] * 1e-3) / HBM_PEAK, 3)}
    for tag in ("", "_no_merged"):
        res[f"composition_over_kernel{tag}"] = round(res[f"torch_composition{tag}"]["ms"]["median"]
                                                     / res[f"kernel{tag}"]["ms"]["median"], 2)
    agree = {}
    for tag in ("", "_no_merged"):
        (kv, kd, ks), (tv, td, ts) = outs[f"kernel{tag}"], outs[f"torch_composition{tag}"]
        ks, ts = ks.cpu().numpy(), ts.cpu().numpy()
        rel = float((np.abs(ks[:, 4:] - ts[:, 4:]) / np.maximum(np.abs(ks[:, 4:]), 1e-300)).max())
        agree[f"vue_equal{tag}"], agree[f"diff_equal{tag}"] = bool(torch.equal(kv, tv)), bool(torch.equal(kd, td))
        agree[f"counts_equal{tag}"], agree[f"sums_rel{tag}"] = bool(np.array_equal(ks[:, :4], ts[:, :4])), rel
        agree[f"diff_rel{tag}"] = float(((kd - td).abs() / kd.abs().clamp_min(1e-30)).max())
    res["agreement"] = agree
    res["agree"] = all(agree[f"vue_equal{t}"] and agree[f"diff_rel{t}"] <= 2.0 ** -23 and agree[f"sums_rel{t}"] <= 1e-6
                       for t in ("", "_no_merged"))
    return res


def patient_legs(p, reps, dev):
    """build_dataset --against scect on the patient as a DICOM tree; seconds per step."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("dcs_prepare_nmodel_data", os.path.join(PKG, "prepare_nmodel_data.py"))
    builder = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(builder)
    ncct, sn, in_, cect, sc, ic, _ = p
    d, h, _ = ncct.shape
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        for folder, px, a, b in (("POST VUE", ncct, sn, in_), ("POST STD", cect, sc, ic)):
            os.makedirs(os.path.join(tmp, "in", "DS", "P0", folder))
            for z in range(d):
                dicom.new_ct_slice(px[z], float(a[z]), float(b[z]), instance=z + 1, uid_suffix=f"{folder[-1]}.{z}") \
                     .save_as(os.path.join(tmp, "in", "DS", "P0", folder, f"IM{z:04d}.dcm"))
        print(f"DICOM tree written in {time.perf_counter() - t0:.1f} s", flush=True)
        torch.manual_seed(0)
        for name, g in (("soft", Generator(3, 9)), ("lung", Generator(2, 9))):
            torch.save(g.state_dict(), os.path.join(tmp, f"{name}.pth"))
        args = builder.get_args(["--input_dir_root", os.path.join(tmp, "in"), "--dataset_names", "DS", "--data_dir",
                                 os.path.join(tmp, "data"), "--img_size", str(h), "--gpu_id", str(dev.index or 0),
                                 "--model_path_soft", os.path.join(tmp, "soft.pth"), "--model_path_lung",
                                 os.path.join(tmp, "lung.pth"), "--overwrite"])
        translate = builder.resident_translate(args)          # the checkpoints are loaded once, outside the split
        laps = []
        for i in range(reps + 1):
            row = builder.build_dataset(args, translate)[0]
            assert row["status"] == "written", row
            if i:
                laps.append(row["seconds"])
            print(f"patient run {i}{' (warm-up)' if i == 0 else ''}: " +
                  ", ".join(f"{k} {v:.3f} s" for k, v in row["seconds"].items()), flush=True)
    out = {k: _spread([lap[k] for lap in laps]) for k in laps[0]}
    out["total"] = _spread([sum(lap.values()) for lap in laps])
    out["manifest"] = {k: row[k] for k in ("n_apply", "n_neg", "n_over", "mean_clipped", "share_apply", "corr")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="128x512x512")
    ap.add_argument("--distinct", type=int, default=16, help="phantom slices drawn; the series repeats them")
    ap.add_argument("--reps", type=int, default=10, help="rounds of the kernel legs")
    ap.add_argument("--patient_reps", type=int, default=3)
    ap.add_argument("--skip_patient", action="store_true", help="the kernel legs only")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_nmodel_data.py needs a GPU")
    dev = torch.device(a.device)
    shape = tuple(int(x) for x in a.shape.split("x"))
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    t0 = time.perf_counter()
    p = patient(shape, a.distinct)
    print(f"phantom patient {shape} in {time.perf_counter() - t0:.1f} s", flush=True)
    res = {"metric": "nmodel_data_patient", "device": torch.cuda.get_device_name(dev), "shape": a.shape}
    with torch.cuda.device(dev):
        res["kernels"] = kernel_legs(p, dev, a.reps)
        print("kernels:", json.dumps(res["kernels"]), flush=True)
        if not a.skip_patient:
            res["patient_seconds"] = patient_legs(p, a.patient_reps, dev)
    print(json.dumps(res))
    if not res["kernels"]["agree"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
