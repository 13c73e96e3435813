"""Evaluation entry point: a drop-in for the reference's calculate.py.

    python ducosy-gan_amd/calculate.py --input_dir_root ... --output_dir_root ... \
        --dataset_names NAME [--device cuda]

It converts the VUE, STD and generated DICOM series of every patient to ``.npy`` stacks sorted by
ImagePositionPatient[2], computes MAE, PSNR, SSIM (raw and normalised) for the three pairs and
EMD, texture similarity, cosine similarity and Euclidean distance (with --ms_ssim, MS-SSIM too)
for STD against Generated, and writes the reference's files under ``<output_dir_root>/calculated``:
``data/{dataset}_{patient}_{category}.npy``, ``detail/{dataset}_{patient}_metrics.csv``,
``result_all_metrics.pkl`` and ``summary_statistics.csv``.

Differences from the reference, all deliberate:
  * --device cuda computes the metrics on the MI355X (modules/metrics_gpu.py, csrc/metrics.hip);
    the default, cpu, runs the numpy / scipy path of modules/metrics.py.  Both follow the
    arithmetic fixed in modules/metrics.py;
  * patients run one after another in this process (no process pool: --num_workers is accepted
    and ignored);
  * MS-SSIM is computed only with --ms_ssim (off by default, which keeps the files of earlier
    runs unchanged), on either --device, from a restatement of torchmetrics' defaults
    (modules/metrics.py::ms_ssim_levels; torchmetrics is not installed, so parity with the
    reference's own numbers is unpinned); without the flag its column is empty.  It is defined
    for slices of at least 176 x 176 and is empty below that, as in the reference;
  * LPIPS is computed only with --lpips_weights PATH[,PATH], on either --device: the lpips library
    is not needed, the metric (lpips.LPIPS(net='alex')) is restated from the package's defaults
    (modules/metrics.py::lpips_taps) on the weights in the named torch.save'd state dicts, either
    lpips.LPIPS(net='alex').state_dict() or torchvision's alexnet plus the package's alex.pth
    (modules/lpips_weights.py); parity with the reference's own numbers is unpinned.  Without the
    flag its column is empty, as the reference leaves it without the library, and so it is for
    slices below 31 x 31; the box and scatter plots need seaborn and are skipped;
  * --regions (off by default; the files above are the same with and without it) adds a region-wise
    evaluation of this package's own, which the reference does not have, on either --device: MAE, bias,
    PSNR and SSIM per owner of the dual-range synthesis (lung, soft tissue, rest: the NCCT HU ranges
    of generate.py, --lung_hu_min ... --soft_hu_max) and over the truly enhancing voxels
    (--enhancement_threshold, --enhancement_min_hu), with the Dice overlap of the predicted and the
    true enhancement (modules/metrics.py::REGIONS).  It needs a VUE series and writes
    ``regions/{dataset}_{patient}_regions.csv``, ``result_region_metrics.pkl`` and
    ``summary_statistics_regions.csv``; an empty region is an empty cell.  --mask composes with it;
    regions from anatomical masks or organ labels are out of scope;
  * nothing happens at import or while parsing arguments: no environment variable is set and no
    directory is created before the conversion starts.
DICOM files are read with modules/dicom.py.
"""
import argparse
import csv
import glob
import os
import pickle
import shutil
import sys
import traceback

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

from modules import dicom  # noqa: E402
from modules import metrics as M  # noqa: E402

CATEGORIES = ("vue", "std", "generated")


def get_args(argv=None):
    p = argparse.ArgumentParser(description="Metrics of generated contrast-enhanced CT series")
    p.add_argument("--data_dir_root", type=str, default="./data", help="Root directory of the data")
    p.add_argument("--input_dir_root", type=str, default="./data/input", help="Root directory of the input datasets")
    p.add_argument("--working_dir_root", type=str, default="./data/working", help="Root directory of inference results")
    p.add_argument("--output_dir_root", type=str, default="./data/output",
                   help="Root directory of the merged results and of the metrics")
    p.add_argument("--dataset_names", type=str, nargs="+", default=["Kyunghee_Univ"], help="Dataset folder names")
    p.add_argument("--ncct_folder", type=str, default="POST VUE", help="Folder name of the non-contrast CT")
    p.add_argument("--cect_folder", type=str, default="POST STD", help="Folder name of the contrast-enhanced CT")
    p.add_argument("--apply_masking", action="store_true", help="Accepted for compatibility")
    p.add_argument("--img_size", type=int, default=512, help="Accepted for compatibility")
    p.add_argument("--batch_size", type=int, default=4, help="Accepted for compatibility")
    p.add_argument("--nmodel_path", type=str, default="./checkpoints/Normal_Map_Unet.pth",
                   help="Accepted for compatibility")
    p.add_argument("--gpu_id", type=int, default=0, help="GPU used by --device cuda")
    p.add_argument("--fast", action="store_true", help="Accepted for compatibility")
    p.add_argument("--reset", action="store_true", help="Remove the calculation output directory first")
    p.add_argument("--mask", action="store_true", help="Calculate the metrics on the masked series")
    p.add_argument("--skip_convert", action="store_true", help="Reuse the .npy stacks of an earlier run")
    p.add_argument("--use_gpu", action="store_true", help="Accepted for compatibility (the metrics, MS-SSIM and LPIPS run where --device says; see --ms_ssim "
                        "and --lpips_weights)")
    p.add_argument("--num_workers", type=int, default=1, help="Accepted for compatibility (patients run in sequence)")
    p.add_argument("--device", choices=["cpu", "cuda"], default="cpu",
                   help="cuda: compute the metrics with the HIP kernels; cpu: numpy / scipy on the host")
    p.add_argument("--ms_ssim", action="store_true",
                   help="Compute MS-SSIM of STD against Generated (slices of at least 176 x 176), on either --device")
    p.add_argument("--lpips_weights", type=str, default=None, metavar="PATH[,PATH]",
                   help="Compute LPIPS (AlexNet) of STD against Generated (slices of at least 31 x 31), on either "
                        "--device, with the weights in these torch.save'd state dicts: lpips.LPIPS(net='alex')'s, "
                        "or torchvision's alexnet and the lpips package's alex.pth")
    p.add_argument("--regions", action="store_true",
                   help="Also write region-wise metrics (per HU-range owner of the synthesis: lung, soft, rest; and over "
                        "the truly enhancing voxels) of every patient with a VUE series, on either --device, to files "
                        "of their own")
    p.add_argument("--soft_hu_min", type=int, default=-150, help="--regions: the soft-tissue model's HU range")
    p.add_argument("--soft_hu_max", type=int, default=250)
    p.add_argument("--lung_hu_min", type=int, default=-1000, help="--regions: the lung model's HU range")
    p.add_argument("--lung_hu_max", type=int, default=-150)
    p.add_argument("--enhancement_threshold", type=float, default=5.0,
                   help="--regions: a voxel enhances where CECT - NCCT exceeds this many HU")
    p.add_argument("--enhancement_min_hu", type=float, default=-400.0,
                   help="--regions: and only where the NCCT HU exceeds this")
    return p.parse_args(argv)


def hu_array(dcm) -> np.ndarray:
    intercept = dcm.RescaleIntercept if "RescaleIntercept" in dcm else 0
    slope = dcm.RescaleSlope if "RescaleSlope" in dcm else 1
    return dcm.pixel_array.astype(np.float32) * slope + intercept


def series_dir(args, category, patient_dir):
    if category == "std":
        return os.path.join(patient_dir, args.cect_folder)
    if category == "vue":
        return os.path.join(patient_dir, args.ncct_folder)
    sub = os.path.join(patient_dir, "generated")
    return sub if os.path.exists(sub) else patient_dir


def read_series(dcm_dir):
    """The HU slices of a folder stacked in ImagePositionPatient[2] order, or None."""
    slices = []
    for path in sorted(glob.glob(os.path.join(dcm_dir, "*.dcm"))):
        try:
            dcm = dicom.dcmread(path)
            z = dcm.get("ImagePositionPatient", [0.0, 0.0, 0.0])[2]
            slices.append((hu_array(dcm), z))
        except Exception as e:
            print(f"Error reading {path}: {e}")
    if not slices:
        return None
    slices.sort(key=lambda s: s[1])
    return np.stack([s[0] for s in slices], axis=0)


def convert(args):
    """DICOM series -> .npy stacks.  Returns (output_dir, data_dir, [(dataset, patient), ...])."""
    print("Starting DICOM to NPY conversion...")
    out_dir = os.path.join(args.output_dir_root, "calculated_mask" if args.mask else "calculated")
    data_dir = os.path.join(out_dir, "data")
    if args.reset and os.path.exists(out_dir):
        shutil.rmtree(out_dir)
        print(f"Resetting output directory: {out_dir}")
    os.makedirs(data_dir, exist_ok=True)
    masked = os.path.join(args.output_dir_root, "masked")
    roots = {"vue": masked if args.mask else args.input_dir_root,
             "std": masked if args.mask else args.input_dir_root,
             "generated": masked if args.mask else args.output_dir_root}
    tasks = []
    for category in CATEGORIES:
        root = roots[category]
        if not os.path.exists(root):
            if category == "generated":
                print(f"Warning: Generated directory not found at {root}")
            continue
        print(f"\nProcessing Category: {category.upper()} in {root}")
        for dataset in args.dataset_names:
            base = os.path.join(root, dataset)
            if not os.path.exists(base):
                continue
            for patient_dir in sorted(d for d in glob.glob(os.path.join(base, "*")) if os.path.isdir(d)):
                patient = os.path.basename(patient_dir)
                if (dataset, patient) not in tasks:
                    tasks.append((dataset, patient))
                npy = os.path.join(data_dir, f"{dataset}_{patient}_{category}.npy")
                if args.skip_convert or os.path.exists(npy):
                    continue
                dcm_dir = series_dir(args, category, patient_dir)
                if not os.path.exists(dcm_dir):
                    continue
                stack = read_series(dcm_dir)
                if stack is not None:
                    np.save(npy, stack)
    return out_dir, data_dir, tasks


class RegionRun:
    """--regions: the HU ranges, the directory of the per-patient CSVs and the aggregates so far."""

    def __init__(self, args, out_dir):
        self.spec = M.RegionSpec(args.lung_hu_min, args.lung_hu_max, args.soft_hu_min, args.soft_hu_max,
                                 args.enhancement_threshold, args.enhancement_min_hu)
        self.dir = os.path.join(out_dir, "regions")
        self.result_path = os.path.join(out_dir, "result_region_metrics.pkl")
        self.summary = {"patient": [], **{k: [] for k in M.REGION_COLUMNS}}


def process_regions(dataset, patient, run, device, std, gen, vue):
    """Region metrics of one patient (series as arrays, or already on the device) and its CSV."""
    if vue is None:
        print(f"  {dataset} {patient}: no VUE series, skipped for regions")
        return
    try:
        if device is None:
            agg, per_slice = M.region_metrics(std, gen, vue, run.spec)
        else:
            from modules import metrics_gpu
            agg, per_slice = metrics_gpu.region_metrics(std, gen, vue, device=device, spec=run.spec)
        os.makedirs(run.dir, exist_ok=True)
        M.write_region_csv(os.path.join(run.dir, f"{dataset}_{patient}_regions.csv"), per_slice)
        run.summary["patient"].append(f"{dataset}_{patient}")
        for k in M.REGION_COLUMNS:
            run.summary[k].append(agg[k])
    except Exception as e:
        print(f"Error in the region metrics of {patient}: {e}")
        traceback.print_exc()


def process_patient(dataset, patient, data_dir, detail_dir, device, ms_ssim=False, lpips_weights=None, regions=None,
                    metrics=True):
    """Metrics of one patient and its detail CSV; None when the STD or generated stack is missing.
    regions: a RegionRun, for the region metrics as well (metrics=False: for those alone)."""
    path = lambda c: os.path.join(data_dir, f"{dataset}_{patient}_{c}.npy")
    if not (os.path.exists(path("std")) and os.path.exists(path("generated"))):
        return None
    try:
        std, gen = np.load(path("std")), np.load(path("generated"))
        vue = np.load(path("vue")) if os.path.exists(path("vue")) else None
        if regions is not None and device is not None:   # one upload serves both calls
            from modules import metrics_gpu
            std, gen, vue = (None if v is None else metrics_gpu.to_device(v, device) for v in (std, gen, vue))
        if not metrics:
            process_regions(dataset, patient, regions, device, std, gen, vue)
            return None
        if device is None:
            patient_metrics, csv_data = M.evaluate_patient(std, gen, vue, ms_ssim, lpips_weights)
        else:
            from modules import metrics_gpu
            patient_metrics, csv_data = metrics_gpu.evaluate_patient(std, gen, vue, device=device, ms_ssim=ms_ssim,
                                                                    lpips_weights=lpips_weights)
        try:
            M.write_detail_csv(os.path.join(detail_dir, f"{dataset}_{patient}_metrics.csv"), csv_data, vue is not None)
        except Exception as e:
            print(f"Error saving CSV for {patient}: {e}")
        if regions is not None:
            process_regions(dataset, patient, regions, device, std, gen, vue)
        return patient_metrics
    except Exception as e:
        print(f"Error processing {patient}: {e}")
        traceback.print_exc()
        return None


def calculate(out_dir, data_dir, tasks, device, ms_ssim=False, lpips_weights=None, regions=None):
    print(f"\nCalculating metrics for generated images (device: {device or 'cpu'})...")
    result_path = os.path.join(out_dir, "result_all_metrics.pkl")
    detail_dir = os.path.join(out_dir, "detail")
    os.makedirs(detail_dir, exist_ok=True)
    if os.path.exists(result_path):
        with open(result_path, "rb") as f:
            summary = pickle.load(f)
        # as the reference: drop patients whose VUE and STD series are the same
        drop = {i for i, v in enumerate(summary["mae"]) if len(v) > 1 and v[1] == 0.0}
        summary = {k: [v for i, v in enumerate(vals) if i not in drop] for k, vals in summary.items()}
        print(f"Existing results found at {result_path}. Loaded previous calculations.")
        if regions is not None and not os.path.exists(regions.result_path):
            for dataset, patient in tasks:
                process_patient(dataset, patient, data_dir, detail_dir, device, regions=regions, metrics=False)
    else:
        summary = {k: [] for k in M.METRICS}
        valid = 0
        for n, (dataset, patient) in enumerate(tasks, 1):
            res = process_patient(dataset, patient, data_dir, detail_dir, device, ms_ssim, lpips_weights, regions)
            print(f"  [{n}/{len(tasks)}] {dataset} {patient}: {'done' if res is not None else 'skipped'}")
            if res is None:
                continue
            valid += 1
            for k in summary:
                summary[k].append(res[k])
        if valid == 0:
            print("No valid results found.")
            return
        with open(result_path, "wb") as f:
            pickle.dump(summary, f)
        print(f"Calculations complete. Valid patients: {valid}. Results saved to {result_path}")
    if regions is not None and regions.summary["patient"]:
        with open(regions.result_path, "wb") as f:
            pickle.dump(regions.summary, f)
        print(f"Region metrics of {len(regions.summary['patient'])} patients saved to {regions.result_path}")
    try:
        print("\n[Global Average: CECT(STD) vs Generated]")
        for name, key in (("MAE ", "mae"), ("PSNR", "psnr"), ("SSIM", "ssim")):
            print(f"{name} : {np.mean([x[0] for x in summary[key]]):.4f}")
    except Exception:
        print("Could not compute averages.")
    print("Plots skipped: the reference draws them with seaborn, which is not installed.")


def summary_statistics(detail_dir, summary_csv_path, pattern="*_metrics.csv"):
    """Mean, std, min, max, median and count of every column of the CSVs ``pattern`` names in
    detail_dir (the detail CSVs by default) over all patients."""
    print(f"\nComputing summary statistics from {detail_dir}...")
    files = sorted(glob.glob(os.path.join(detail_dir, pattern))) if os.path.exists(detail_dir) else []
    if not files:
        print("No CSV files found in detail result directory.")
        return
    columns = {}
    for path in files:
        try:
            with open(path, "r") as f:
                for row in csv.DictReader(f):
                    for key, value in row.items():
                        if key == "Slice_Idx":
                            continue
                        try:
                            columns.setdefault(key, []).append(float(value))
                        except (ValueError, TypeError):
                            pass
        except Exception as e:
            print(f"Error reading {path}: {e}")
    rows = []
    for name, values in columns.items():
        ok = [v for v in values if np.isfinite(v)]
        if ok:
            rows.append({"Metric": name, "Mean": f"{np.mean(ok):.4f}", "Std": f"{np.std(ok):.4f}",
                         "Min": f"{np.min(ok):.4f}", "Max": f"{np.max(ok):.4f}", "Median": f"{np.median(ok):.4f}",
                         "Count": len(ok)})
    if not rows:
        print("No valid data to summarize.")
        return
    with open(summary_csv_path, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=["Metric", "Mean", "Std", "Min", "Max", "Median", "Count"])
        w.writeheader()
        w.writerows(rows)
    print(f"Summary statistics saved to {summary_csv_path}")


def main(argv=None):
    args = get_args(argv)
    device = f"cuda:{args.gpu_id}" if args.device == "cuda" else None
    lpips_weights = None
    if args.lpips_weights:   # loaded once, before any work: a bad file fails here
        from modules import lpips_weights as LW
        lpips_weights = LW.load(args.lpips_weights)
    out_dir, data_dir, tasks = convert(args)
    regions = RegionRun(args, out_dir) if args.regions else None
    if tasks:
        calculate(out_dir, data_dir, tasks, device, args.ms_ssim, lpips_weights, regions)
    else:
        print("No tasks found. Please check input directories and arguments.")
    summary_statistics(os.path.join(out_dir, "detail"),
                       os.path.join(out_dir, "summary_statistics_masked.csv" if args.mask else "summary_statistics.csv"))
    if regions is not None:
        summary_statistics(regions.dir, os.path.join(out_dir, "summary_statistics_regions.csv"), "*_regions.csv")


if __name__ == "__main__":
    main()
