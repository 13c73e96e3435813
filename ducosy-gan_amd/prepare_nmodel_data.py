"""Build the training set of the normal-map U-Net (train_nmodel.py) from DICOM pairs.

    python prepare_nmodel_data.py --input_dir_root ... --dataset_names NAME --data_dir data \
        --model_path_soft ckpt_soft.pth --model_path_lung ckpt_lung.pth

Per patient of each dataset the NCCT series (--ncct_folder, POST VUE) and the CECT series
(--cect_folder, POST STD) are read with modules/dicom.py and ordered with
modules/dataset.py::_sort_slices, the pairing the CycleGAN training uses; the two are
reconstructions of one acquisition, so the pair is voxel-aligned and nothing is registered.  Written:

    <data_dir>/vue_files/{dataset}_{patient}_vue.npy    the NCCT in HU, float32 [D,H,W]
    <data_dir>/diff_map/{dataset}_{patient}_diff.npy    the target, float32 [D,H,W]
    <data_dir>/stats/{dataset}_{patient}_slices.csv     the per-slice record and correlation
    <data_dir>/manifest.csv                             one row per patient of this run

The target is this project's definition (modules/nmodel/prepare.py; the reference has no recipe):
with --against scect (the default) real CECT - merged sCECT before the smoothing, in the units
apply_diffmap adds; the sCECT comes from the resident pipeline of generate.py
(modules/inference.py::translate_volume_device, --synthesis range or enhancement) and stays on the
GPU, the CECT stored values go up once, one kernel pass (csrc/nmodel_data.hip) writes both volumes
and the statistics, and the two volumes come down.  That mode needs the GPU and both Generator
checkpoints.  With --against ncct the target is the plain enhancement CECT - NCCT: no Generator is
loaded, --device cuda runs the same kernel without the sCECT and --device cpu the host function;
both write byte-identical .npy files.

A patient is skipped, with the reason in its manifest row, when a series is missing or empty, the
slice counts differ, the slices are not all of one shape across both series, a series mixes stored
dtypes, or (--min_corr) the volume's NCCT / CECT correlation is below the gate: a reversed or
foreign series shows up as a low correlation.  An existing pair of files is left alone unless
--overwrite is given, and its manifest row says so.
"""
import argparse
import csv
import glob
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

from modules.nmodel import prepare  # noqa: E402

MANIFEST_COLUMNS = ("id", "dataset", "patient", "D", "H", "W", "against", "synthesis", "n", "n_apply", "n_neg",
                    "n_over", "mean_clipped", "share_apply", "corr", "status")
SLICE_COLUMNS = ("slice",) + prepare.STAT_NAMES + ("corr",)
NEEDS_GPU = ("--against scect needs the GPU and both Generator checkpoints (the sCECT comes from the resident "
             "pipeline): run it with --device cuda, or build the plain enhancement with --against ncct")


class Skip(Exception):
    """A patient that cannot be built; the message is the manifest's reason."""


def read_series(folder, what):
    """(stored [D,H,W], slopes, intercepts) of one series in _sort_slices order."""
    from modules import dicom
    from modules.dataset import _sort_slices
    files = sorted(glob.glob(os.path.join(folder, "*.dcm"))) if os.path.isdir(folder) else []
    if not files:
        raise Skip(f"{what} series missing or empty")
    dcms = [dicom.dcmread(p) for p in _sort_slices(files)]
    pixels = [d.pixel_array for d in dcms]
    return (pixels, [float(getattr(d, "RescaleSlope", 1)) for d in dcms],
            [float(getattr(d, "RescaleIntercept", 0)) for d in dcms])


def read_pair(patient_dir, args):
    """Both series of a patient as (ncct, sn, in, cect, sc, ic), the checks of the module doc applied."""
    n_px, sn, in_ = read_series(os.path.join(patient_dir, args.ncct_folder), "NCCT")
    c_px, sc, ic = read_series(os.path.join(patient_dir, args.cect_folder), "CECT")
    if len(n_px) != len(c_px):
        raise Skip(f"slice counts differ: {len(n_px)} NCCT, {len(c_px)} CECT")
    shapes = {p.shape for p in n_px} | {p.shape for p in c_px}
    if len(shapes) != 1:
        raise Skip("slices differ in shape: " + ", ".join("x".join(map(str, s)) for s in sorted(shapes)))
    for what, px in (("NCCT", n_px), ("CECT", c_px)):
        kinds = sorted({p.dtype.name for p in px})
        if len(kinds) != 1:
            raise Skip(f"{what} series mixes stored dtypes: {', '.join(kinds)}")
        if px[0].dtype not in (np.int16, np.uint16):
            raise Skip(f"{what} series has stored dtype {kinds[0]} (int16 or uint16 expected)")
    if any(s == 0 or not np.isfinite(s) for s in sn):
        raise Skip("NCCT series has a zero or non-finite RescaleSlope")
    return np.stack(n_px), sn, in_, np.stack(c_px), sc, ic


def load_generator(path, device):
    """A Generator shaped by its checkpoint: the input channel count as generate.py reads it, and the
    number of residual blocks and whether they carry CBAM from the keys (generate.py builds the
    reference's 9 blocks; a checkpoint of train.py --num_residual_blocks N loads here as well)."""
    import torch
    from modules.model import Generator
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if all(k.startswith("module.") for k in sd):
        sd = {k[len("module."):]: v for k, v in sd.items()}
    blocks = len({k.split(".")[1] for k in sd if ".block." in k})
    g = Generator(input_channels=int(sd["model.1.weight"].shape[1]), num_residual_blocks=blocks,
                  use_cbam=any(".cbam." in k for k in sd))
    g.load_state_dict(sd)
    return g.to(device).eval()


def resident_translate(args):
    """The default ``translate``: (stored NCCT, slopes, intercepts) -> the merged sCECT before the
    smoothing, a float32 device tensor, from generate.py's resident pipeline without the
    difference-map stage."""
    import torch
    from modules.inference import translate_volume_device
    device = torch.device(f"cuda:{args.gpu_id}")
    soft = load_generator(args.model_path_soft, device)
    lung = load_generator(args.model_path_lung, device)
    soft_range, lung_range = (args.soft_hu_min, args.soft_hu_max), (args.lung_hu_min, args.lung_hu_max)

    def translate(raw, slopes, intercepts):
        return translate_volume_device(soft, lung, raw, slopes, intercepts, soft_range, lung_range, args.img_size,
                                       int(args.slice_batch), device, synthesis=args.synthesis,
                                       enhancement_threshold=args.enhancement_threshold,
                                       enhancement_min_hu=args.enhancement_min_hu)
    return translate


def patient_targets(pair, args, translate, seconds):
    """(vue, diff, stats) as numpy arrays; ``seconds`` takes the wall time of every step."""
    ncct, sn, in_, cect, sc, ic = pair
    clock = _Clock(seconds, sync=args.device == "cuda")
    merged = None
    if args.against == "scect":
        merged = translate(ncct, sn, in_)
        clock.lap("translate")
    if args.device == "cpu":
        if merged is not None and not isinstance(merged, np.ndarray):
            merged = merged.detach().cpu().numpy()
        out = prepare.residual_targets(ncct, sn, in_, cect, sc, ic, merged, args.diffmap_threshold)
        clock.lap("targets")
        return out
    import torch
    from modules.hip import nmodel_data as ND
    dev = torch.device(f"cuda:{args.gpu_id}")
    with torch.cuda.device(dev):
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(dev)
        if merged is not None and not isinstance(merged, torch.Tensor):
            merged = torch.from_numpy(np.ascontiguousarray(merged, dtype=np.float32))
        if merged is not None:
            merged = merged.to(dev)
        vue, diff, stats = ND.residual_targets(up(ncct), sn, in_, up(cect), sc, ic, merged, args.diffmap_threshold,
                                               ncct_unsigned=ncct.dtype == np.uint16,
                                               cect_unsigned=cect.dtype == np.uint16)
        clock.lap("targets")
        out = vue.cpu().numpy(), diff.cpu().numpy(), stats.cpu().numpy()
        clock.lap("download")
    return out


class _Clock:
    def __init__(self, seconds, sync=False):
        self.seconds, self.sync, self.t = seconds, sync, time.perf_counter()

    def lap(self, name):
        if self.sync:
            import torch
            torch.cuda.synchronize()
        now = time.perf_counter()
        self.seconds[name] = self.seconds.get(name, 0.0) + now - self.t
        self.t = now


def _cell(v):
    if isinstance(v, float):
        return "" if np.isnan(v) else repr(v)
    return v


def write_slice_stats(path, stats):
    corr = prepare.pearson_from_sums(stats)
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(SLICE_COLUMNS)
        for z, row in enumerate(stats):
            cells = [int(v) if k in prepare.COUNT_COLS else float(v) for k, v in enumerate(row)]
            w.writerow([z] + [_cell(c) for c in cells] + [_cell(float(corr[z]))])


def build_dataset(args, translate=None):
    """The loop of the module doc.  ``translate``: the callable that maps (stored NCCT [D,H,W],
    slopes, intercepts) to the merged volume (a float32 device tensor or array in stored-value units of
    the NCCT); the default is the resident pipeline (``resident_translate``).  Returns the manifest
    rows (dicts; "seconds" holds the wall time of each step of a patient and is not written)."""
    if args.against == "scect" and translate is None:
        if args.device != "cuda":
            sys.exit(NEEDS_GPU)
        translate = resident_translate(args)
    dirs = {k: os.path.join(args.data_dir, k) for k in ("vue_files", "diff_map", "stats")}
    for d in dirs.values():
        os.makedirs(d, exist_ok=True)
    rows = []
    for dataset in args.dataset_names:
        input_dir = os.path.join(args.input_dir_root, dataset)
        for patient_dir in sorted(d for d in glob.glob(os.path.join(input_dir, "*")) if os.path.isdir(d)):
            patient = os.path.basename(patient_dir)
            pid = f"{dataset}_{patient}"
            row = {"id": pid, "dataset": dataset, "patient": patient, "against": args.against,
                   "synthesis": args.synthesis if args.against == "scect" else "", "seconds": {}}
            rows.append(row)
            vue_path = os.path.join(dirs["vue_files"], f"{pid}_vue.npy")
            diff_path = os.path.join(dirs["diff_map"], f"{pid}_diff.npy")
            if not args.overwrite and os.path.exists(vue_path) and os.path.exists(diff_path):
                row["status"] = "kept: files exist (--overwrite rewrites them)"
                print(f"{pid}: {row['status']}")
                continue
            try:
                clock = _Clock(row["seconds"])
                pair = read_pair(patient_dir, args)
                clock.lap("read")
                row["D"], row["H"], row["W"] = pair[0].shape
                vue, diff, stats = patient_targets(pair, args, translate, row["seconds"])
                row.update(prepare.volume_summary(stats))
                if args.min_corr is not None and not row["corr"] >= args.min_corr:
                    raise Skip(f"correlation {row['corr']:.4f} below --min_corr {args.min_corr:g}")
            except Skip as e:
                row["status"] = f"skipped: {e}"
                print(f"{pid}: {row['status']}")
                continue
            clock = _Clock(row["seconds"])
            np.save(vue_path, vue)
            np.save(diff_path, diff)
            write_slice_stats(os.path.join(dirs["stats"], f"{pid}_slices.csv"), stats)
            clock.lap("save")
            row["status"] = "written"
            print(f"{pid}: {row['D']}x{row['H']}x{row['W']}, mean clipped target {row['mean_clipped']:.3f}, "
                  f"{100 * row['share_apply']:.2f} % at or above {args.diffmap_threshold:g}, correlation {row['corr']:.4f}")
    with open(os.path.join(args.data_dir, "manifest.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(MANIFEST_COLUMNS)
        for row in rows:
            w.writerow([_cell(row.get(k, "")) for k in MANIFEST_COLUMNS])
    done = sum(r["status"] == "written" for r in rows)
    print(f"\n{done} of {len(rows)} patients written to {args.data_dir}.")
    return rows


def get_args(argv=None):
    p = argparse.ArgumentParser(description="Training set of the normal-map U-Net from DICOM pairs (MI355X)")
    p.add_argument("--input_dir_root", default="/archive/Dataset_DuCoSyGAN")
    p.add_argument("--dataset_names", nargs="+", default=["Kangwon_National_Univ_Masked_10"])
    p.add_argument("--ncct_folder", default="POST VUE")
    p.add_argument("--cect_folder", default="POST STD")
    p.add_argument("--data_dir", default="data", help="where vue_files/, diff_map/, stats/ and manifest.csv go "
                                                      "(train_nmodel.py --data_dir)")
    p.add_argument("--against", choices=["scect", "ncct"], default="scect",
                   help="scect: CECT - merged sCECT before the smoothing (needs the GPU and both checkpoints); "
                        "ncct: the plain enhancement CECT - NCCT (no Generator)")
    p.add_argument("--device", choices=["cuda", "cpu"], default="cuda",
                   help="where the targets are computed (cuda: cuda:{gpu_id}); --against ncct writes the same bytes on both")
    p.add_argument("--diffmap_threshold", type=float, default=8,
                   help="apply_diffmap's threshold; only the n_apply statistic uses it")
    p.add_argument("--min_corr", type=float, default=None,
                   help="skip a patient whose NCCT / CECT correlation over the volume is below this (default: no gate)")
    p.add_argument("--overwrite", action="store_true", help="rewrite existing vue / diff files")
    p.add_argument("--img_size", type=int, default=512)
    p.add_argument("--gpu_id", type=int, default=0)
    p.add_argument("--slice_batch", type=int, default=16, help="slices per Generator call")
    p.add_argument("--model_path_soft", default="./checkpoints/v3/Soft_Tissue_Generator_A2B.pth")
    p.add_argument("--model_path_lung", default="./checkpoints/v3/Lung_Generator_A2B.pth")
    p.add_argument("--soft_hu_min", type=int, default=-150)
    p.add_argument("--soft_hu_max", type=int, default=250)
    p.add_argument("--lung_hu_min", type=int, default=-1000)
    p.add_argument("--lung_hu_max", type=int, default=-150)
    p.add_argument("--synthesis", choices=["range", "enhancement"], default="range",
                   help="the synthesis whose merged volume the target is taken against (generate.py --synthesis)")
    p.add_argument("--enhancement_threshold", type=float, default=5.0)
    p.add_argument("--enhancement_min_hu", type=float, default=-400.0)
    return p.parse_args(argv)


if __name__ == "__main__":
    build_dataset(get_args())
