"""Inference entry point — mirror of the reference's generate.py (generate(), synthesis(), synthesis_test()).

    python ducosy-gan_amd/generate.py --input_dir_root ... --dataset_names NAME \
        --model_path_soft ckpt_soft.pth --model_path_lung ckpt_lung.pth

Differences from the reference, all deliberate:
  * slices of a patient are translated in batches on the MI355X Generator kernels
    (modules/inference.py) instead of one slice per call;
  * the Generators are built with the input channel count found in the checkpoint
    (generate.py:29-30 hard-codes 1, which cannot load the mask-conditioned cin 3 / cin 2
    checkpoints that train.py writes); a mask-conditioned Generator gets the anatomical masks
    of the NCCT slice in its training order (soft tissue: bone, mediastinum; lung: lung;
    modules/argmanager.py) from the GPU mask kernel, as the training data pipeline built them;
  * checkpoints are read with torch.load(weights_only=True);
  * --postprocess_device cuda runs the synthesis stage's HU-range merge and volume smoothing on
    the GPU (modules/postprocess_gpu.py, csrc/volume.hip) instead of scipy on the host: one
    upload of the three series, one download of the int16 volume, identical output files;
  * --pipeline resident (generate_synthesis) runs both stages in one pass per patient: stored
    NCCT pixels go up once, HU transform, masks, resizes, both Generators, the output -> stored
    value map, the merge and the smoothing stay on the GPU (csrc/slices.hip, csrc/volume.hip), the
    int16 volume comes down once; no working series is written unless --write_working is given;
  * --apply_diffmap runs the reference's difference-map stage (commented out in its synthesis()):
    the normal-map U-Net of --nmodel_path predicts a contrast difference map from the NCCT HU
    series (modules/nmodel, csrc/unet.hip) and apply_diffmap adds it to the merged volume before
    the smoothing; --save_diff keeps the map as diff.npy in the patient's working directory;
  * --synthesis enhancement runs the reference's second synthesis stage (synthesis_test, never
    called by its __main__) in place of synthesis(): the NCCT is kept everywhere, and where a model
    raised the HU by more than --enhancement_threshold (5) and the NCCT is above
    --enhancement_min_hu (-400) that model's gain is added; the series is written as
    "DuCoSyGAN sCECT v3".  Staged on the host, staged with --postprocess_device cuda
    (csrc/volume.hip) and --pipeline resident (csrc/slices.hip) write identical files.
DICOM reading/writing uses modules/dicom.py (pydicom is not installed in this image).
"""
import argparse
import glob
import os
import shutil
import sys
import traceback
from copy import deepcopy

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from modules.inference import (MASK_TYPES, _conditioning, hu_from_stored, normalise_hu,  # noqa: E402,F401
                               smooth_volume, smooth_volume_device, stored_from_output, synthesize,
                               synthesize_enhancement, synthesize_volume, translate_slices,
                               translate_volume_device)
from modules.model import Generator  # noqa: E402
from modules.nmodel import load_model, predict_volume  # noqa: E402
from modules.postprocess import apply_diffmap  # noqa: E402
from modules.postprocess_gpu import apply_diffmap_device  # noqa: E402


def load_generator(path, device, num_residual_blocks=9):
    """Generator with the checkpoint's own input channel count (module.-prefix tolerant)."""
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if all(k.startswith("module.") for k in sd):
        sd = {k[len("module."):]: v for k, v in sd.items()}
    cin = int(sd["model.1.weight"].shape[1])
    g = Generator(input_channels=cin, num_residual_blocks=num_residual_blocks)
    g.load_state_dict(sd)
    return g.to(device).eval()


def _model_args(args, soft_tissue_args, lung_args):
    """The reference passes the per-model settings as two extra namespaces (model_path, hu_min,
    hu_max; modules/argmanager.py:52-82); this build's single parser carries them as
    --model_path_soft / --soft_hu_min / ... on ``args``.  Either form is accepted."""
    if soft_tissue_args is None:
        soft_tissue_args = argparse.Namespace(model_path=args.model_path_soft, hu_min=args.soft_hu_min,
                                              hu_max=args.soft_hu_max)
    if lung_args is None:
        lung_args = argparse.Namespace(model_path=args.model_path_lung, hu_min=args.lung_hu_min,
                                       hu_max=args.lung_hu_max)
    return soft_tissue_args, lung_args


def _load_nmodel(args, device):
    """The difference-map U-Net when --apply_diffmap is given, else None."""
    if not getattr(args, "apply_diffmap", False):
        return None
    return load_model(args.nmodel_path, device)[0]


def generate(args, soft_tissue_args=None, lung_args=None):
    """generate.py:21-137 (same signature): per patient, translate every NCCT slice with both
    models and write raw / soft_tissue / lung DICOM copies under working_dir_root."""
    from modules import dicom
    sa, la = _model_args(args, soft_tissue_args, lung_args)
    device = torch.device(f"cuda:{args.gpu_id}")
    soft = load_generator(sa.model_path, device)
    lung = load_generator(la.model_path, device)
    batch = int(getattr(args, "slice_batch", 16))
    for dataset_name in args.dataset_names:
        input_dir = os.path.join(args.input_dir_root, dataset_name)
        working_dir = os.path.join(args.working_dir_root, dataset_name)
        for patient_dir in sorted(d for d in glob.glob(os.path.join(input_dir, "*")) if os.path.isdir(d)):
            ncct = os.path.join(patient_dir, args.ncct_folder)
            if not os.path.isdir(ncct):
                continue
            out_dirs = {k: os.path.join(working_dir, os.path.basename(patient_dir), k)
                        for k in ("raw", "soft_tissue", "lung")}
            for d in out_dirs.values():
                os.makedirs(d, exist_ok=True)
            paths = sorted(glob.glob(os.path.join(ncct, "*.dcm")))
            dcms = [dicom.dcmread(p) for p in paths]
            hu = [hu_from_stored(d.pixel_array, d.RescaleSlope, d.RescaleIntercept) for d in dcms]
            outs = {}
            for name, model, lo, hi in (("soft_tissue", soft, sa.hu_min, sa.hu_max),
                                        ("lung", lung, la.hu_min, la.hu_max)):
                outs[name] = (translate_slices(model, [normalise_hu(h, lo, hi) for h in hu], args.img_size,
                                               batch, device, _conditioning(model, name, hu, device)),
                              lo, hi)
            for i, (p, d) in enumerate(zip(paths, dcms)):
                try:
                    shutil.copy(p, os.path.join(out_dirs["raw"], os.path.basename(p)))
                    for name, (ys, lo, hi) in outs.items():
                        px = stored_from_output(ys[i], lo, hi, d.RescaleSlope, d.RescaleIntercept,
                                                d.pixel_array.dtype)
                        o = deepcopy(d)
                        o.SeriesDescription = f"Synthetic CECT (from {d.get('SeriesDescription', '')})"
                        o.file_meta.TransferSyntaxUID = dicom.EXPLICIT_VR_LE
                        o.SmallestImagePixelValue, o.LargestImagePixelValue = int(px.min()), int(px.max())
                        o.PixelData = px.tobytes()
                        o.save_as(os.path.join(out_dirs[name], os.path.basename(p)))
                except Exception as e:  # the reference reports and continues (generate.py:131-135)
                    print(f"Could not process file {p}. Error: {e}")
                    traceback.print_exc()
    print("\nGeneration complete.")


DESCRIPTIONS = {"range": "DuCoSyGAN sCECT v2", "enhancement": "DuCoSyGAN sCECT v3"}


def _rescale(d):
    return getattr(d, "RescaleSlope", 1), getattr(d, "RescaleIntercept", 0)


def synthesis(args, soft_tissue_args=None, lung_args=None):
    """generate.py:137-297 (same signature): merge the two translations inside their HU ranges
    over the NCCT, z-smooth the volume (modules/postprocess.py) and write
    output/{dataset}/{patient}/{idx:04d}.dcm."""
    _synthesis_stage(args, soft_tissue_args, lung_args, "range")


def synthesis_test(args, soft_tissue_args=None, lung_args=None):
    """generate.py:302-477 (same signature), "sCECT v3": keep the NCCT and add each translation's
    HU gain where it exceeds --enhancement_threshold and the NCCT HU exceeds --enhancement_min_hu
    (modules/inference.py::synthesize_enhancement); then the same smoothing, header edits and
    files as synthesis().  Honours --postprocess_device, --apply_diffmap, --save_diff and
    --diffmap_threshold like synthesis()."""
    _synthesis_stage(args, soft_tissue_args, lung_args, "enhancement")


def _synthesis_stage(args, soft_tissue_args, lung_args, mode):
    """The staged synthesis stage; ``mode``: "range" (synthesis) or "enhancement" (synthesis_test)."""
    from modules import dicom
    sa, la = _model_args(args, soft_tissue_args, lung_args)
    post_dev = f"cuda:{args.gpu_id}" if getattr(args, "postprocess_device", "cpu") == "cuda" else None
    nmodel = _load_nmodel(args, torch.device(f"cuda:{args.gpu_id}"))
    thr_e, min_hu_e = getattr(args, "enhancement_threshold", 5.0), getattr(args, "enhancement_min_hu", -400.0)
    for dataset_name in args.dataset_names:
        working_dir = os.path.join(args.working_dir_root, dataset_name)
        output_dir = os.path.join(args.output_dir_root, dataset_name)
        for patient_dir in sorted(d for d in glob.glob(os.path.join(working_dir, "*")) if os.path.isdir(d)):
            lists = [sorted(glob.glob(os.path.join(patient_dir, k, "*.dcm"))) for k in ("raw", "soft_tissue", "lung")]
            if not all(lists) or len({len(x) for x in lists}) != 1:
                print(f"Skipping {patient_dir}: missing or mismatched slices")
                continue
            merged, series, rescale, raw_hu_series, own_pairs = [], [], [], [], []
            for rp, sp, lp in zip(*lists):
                raw, st, lg = dicom.dcmread(rp), dicom.dcmread(sp), dicom.dcmread(lp)
                if nmodel is not None:
                    raw_hu_series.append(hu_from_stored(raw.pixel_array, *_rescale(raw)))
                if mode == "enhancement":  # the reference reads each translated file's own rescale pair
                    own_pairs.append((_rescale(st), _rescale(lg)))
                if post_dev is not None:
                    series.append((raw.pixel_array, st.pixel_array, lg.pixel_array))
                    rescale.append(_rescale(raw))
                    continue
                if mode == "enhancement":
                    merged.append(synthesize_enhancement(raw.pixel_array, st.pixel_array, lg.pixel_array,
                                                         *_rescale(raw), thr_e, min_hu_e, *own_pairs[-1]))
                    continue
                raw_hu = hu_from_stored(raw.pixel_array, *_rescale(raw))
                merged.append(synthesize(raw.pixel_array, raw_hu, st.pixel_array, lg.pixel_array,
                                         (sa.hu_min, sa.hu_max), (la.hu_min, la.hu_max)))
            if post_dev is not None:
                raw_v, soft_v, lung_v = (np.stack(x) for x in zip(*series))
                f32 = lambda pair: tuple(np.float32(v) for v in pair)
                if any(f32(p) != f32(r) for own, r in zip(own_pairs, rescale) for p in own):
                    # the kernel reads all three series with the NCCT's pair
                    print(f"{os.path.basename(patient_dir)}: the translated series carry their own rescale pairs; "
                          "merging on the host")
                    on_dev = torch.from_numpy(np.stack([
                        synthesize_enhancement(r, s, g, a, b, thr_e, min_hu_e, *own)
                        for r, s, g, (a, b), own in zip(raw_v, soft_v, lung_v, rescale, own_pairs)])).to(post_dev)
                else:
                    on_dev = synthesize_volume(raw_v, [a for a, _ in rescale], [b for _, b in rescale], soft_v, lung_v,
                                               (sa.hu_min, sa.hu_max), (la.hu_min, la.hu_max), device=post_dev,
                                               keep_on_device=True, mode=mode, threshold=thr_e, min_hu=min_hu_e)
            if nmodel is not None:  # the difference-map stage: after the merge, before the smoothing
                diff = predict_volume(nmodel, np.stack(raw_hu_series), f"cuda:{args.gpu_id}")
                if getattr(args, "save_diff", False):
                    np.save(os.path.join(patient_dir, "diff.npy"), diff)
                thr = getattr(args, "diffmap_threshold", 8)
                if post_dev is not None:
                    on_dev = apply_diffmap_device(on_dev, torch.from_numpy(diff).to(post_dev), thr)
                else:
                    merged = apply_diffmap(np.stack(merged), diff, thr)
            if post_dev is not None:
                vol = smooth_volume(on_dev, device=post_dev)
            else:
                vol = smooth_volume(merged)
            out_base = os.path.join(output_dir, os.path.basename(patient_dir))
            os.makedirs(out_base, exist_ok=True)
            for idx, sp in enumerate(lists[1]):
                o = dicom.dcmread(sp)
                px = vol[idx]
                o.PixelData = px.tobytes()
                vr = "US" if o.PixelRepresentation == 0 else "SS"
                o.add_new((0x0028, 0x0106), vr, int(px.min()))
                o.add_new((0x0028, 0x0107), vr, int(px.max()))
                o.WindowWidth, o.WindowCenter = 1250, -375.0   # generate.py:279-282
                o.SeriesDescription = DESCRIPTIONS[mode]
                o.save_as(os.path.join(out_base, f"{idx:04d}.dcm"))
    print("\nSynthesis complete.")


def _write_translation(d, px, path):
    """One slice of a working series, as generate() writes it."""
    from modules import dicom
    o = deepcopy(d)
    o.SeriesDescription = f"Synthetic CECT (from {d.get('SeriesDescription', '')})"
    o.file_meta.TransferSyntaxUID = dicom.EXPLICIT_VR_LE
    o.SmallestImagePixelValue, o.LargestImagePixelValue = int(px.min()), int(px.max())
    o.PixelData = px.tobytes()
    o.save_as(path)


def generate_synthesis(args, soft_tissue_args=None, lung_args=None):
    """--pipeline resident: generate() and synthesis() in one pass per patient, with everything
    between the upload of the NCCT stored values and the download of the smoothed int16 volume
    resident on the GPU (modules/inference.py::translate_volume_device, smooth_volume_device).
    Writes output/{dataset}/{patient}/{idx:04d}.dcm with the pixels and header edits the staged
    path ends up with, and no working series unless --write_working asks for them.

    Slices of one patient that differ in size or stored dtype are processed as one volume per
    (size, dtype) group, each smoothed along z on its own, and written under their series index."""
    from modules import dicom
    sa, la = _model_args(args, soft_tissue_args, lung_args)
    device = torch.device(f"cuda:{args.gpu_id}")
    soft = load_generator(sa.model_path, device)
    lung = load_generator(la.model_path, device)
    nmodel = _load_nmodel(args, device)
    save_diff = nmodel is not None and bool(getattr(args, "save_diff", False))
    batch = int(getattr(args, "slice_batch", 16))
    write_working = bool(getattr(args, "write_working", False))
    mode = getattr(args, "synthesis", "range")
    soft_range, lung_range = (sa.hu_min, sa.hu_max), (la.hu_min, la.hu_max)
    for dataset_name in args.dataset_names:
        input_dir = os.path.join(args.input_dir_root, dataset_name)
        working_dir = os.path.join(args.working_dir_root, dataset_name)
        output_dir = os.path.join(args.output_dir_root, dataset_name)
        for patient_dir in sorted(d for d in glob.glob(os.path.join(input_dir, "*")) if os.path.isdir(d)):
            ncct = os.path.join(patient_dir, args.ncct_folder)
            if not os.path.isdir(ncct):
                continue
            patient = os.path.basename(patient_dir)
            paths = sorted(glob.glob(os.path.join(ncct, "*.dcm")))
            if not paths:
                continue
            dcms = [dicom.dcmread(p) for p in paths]
            pixels = [d.pixel_array for d in dcms]
            groups = {}
            for i, px in enumerate(pixels):
                groups.setdefault((px.shape, px.dtype.str), []).append(i)
            if len(groups) > 1:
                print(f"{patient}: {len(groups)} slice formats; each is translated and smoothed as its own volume")
            out_base = os.path.join(output_dir, patient)
            os.makedirs(out_base, exist_ok=True)
            work = {k: os.path.join(working_dir, patient, k) for k in ("raw", "soft_tissue", "lung")}
            if write_working:
                for d in work.values():
                    os.makedirs(d, exist_ok=True)
            for gi, idxs in enumerate(groups.values()):
                raw = np.stack([pixels[i] for i in idxs])
                stage = {} if nmodel is None else dict(nmodel=nmodel, want_diff=save_diff,
                                                       diffmap_threshold=getattr(args, "diffmap_threshold", 8))
                if mode == "enhancement":
                    stage.update(synthesis=mode, enhancement_threshold=getattr(args, "enhancement_threshold", 5.0),
                                 enhancement_min_hu=getattr(args, "enhancement_min_hu", -400.0))
                res = translate_volume_device(
                    soft, lung, raw, [getattr(dcms[i], "RescaleSlope", 1) for i in idxs],
                    [getattr(dcms[i], "RescaleIntercept", 0) for i in idxs], soft_range, lung_range,
                    args.img_size, batch, device, want_stored=write_working, **stage)
                merged = res[0] if (write_working or save_diff) else res
                if save_diff:  # one file per slice format; a uniform series writes diff.npy
                    os.makedirs(os.path.join(working_dir, patient), exist_ok=True)
                    name = "diff.npy" if len(groups) == 1 else f"diff_{gi}.npy"
                    np.save(os.path.join(working_dir, patient, name), res[-1].cpu().numpy())
                vol = smooth_volume_device(merged).cpu().numpy()
                if write_working:
                    series = {k: t.cpu().numpy().view(raw.dtype) for k, t in (("soft_tissue", res[1]), ("lung", res[2]))}
                for k, i in enumerate(idxs):
                    d, name = dcms[i], os.path.basename(paths[i])
                    if write_working:
                        shutil.copy(paths[i], os.path.join(work["raw"], name))
                        for kind, s in series.items():
                            _write_translation(d, s[k], os.path.join(work[kind], name))
                    o, px = deepcopy(d), vol[k]
                    o.file_meta.TransferSyntaxUID = dicom.EXPLICIT_VR_LE
                    o.PixelData = px.tobytes()
                    vr = "US" if o.PixelRepresentation == 0 else "SS"
                    o.add_new((0x0028, 0x0106), vr, int(px.min()))
                    o.add_new((0x0028, 0x0107), vr, int(px.max()))
                    o.WindowWidth, o.WindowCenter = 1250, -375.0   # generate.py:279-282
                    o.SeriesDescription = DESCRIPTIONS[mode]
                    o.save_as(os.path.join(out_base, f"{i:04d}.dcm"))
    print("\nGeneration and synthesis complete.")


def get_args(argv=None):
    """The reference's inference arguments (modules/argmanager.py:4-81) in one parser (the
    reference parses sys.argv three times with three parsers, generate.py:483-485)."""
    p = argparse.ArgumentParser(description="CycleGAN Inference for CT Scans (MI355X)")
    p.add_argument("--input_dir_root", default="/archive/Dataset_DuCoSyGAN")
    p.add_argument("--working_dir_root", default="./data/working")
    p.add_argument("--output_dir_root", default="./data/output")
    p.add_argument("--dataset_names", nargs="+", default=["Kangwon_National_Univ_Masked_10"])
    p.add_argument("--ncct_folder", default="POST VUE")
    p.add_argument("--img_size", type=int, default=512)
    p.add_argument("--gpu_id", type=int, default=0)
    p.add_argument("--slice_batch", type=int, default=16, help="slices per Generator call")
    p.add_argument("--model_path_soft", default="./checkpoints/v3/Soft_Tissue_Generator_A2B.pth")
    p.add_argument("--model_path_lung", default="./checkpoints/v3/Lung_Generator_A2B.pth")
    p.add_argument("--soft_hu_min", type=int, default=-150)
    p.add_argument("--soft_hu_max", type=int, default=250)
    p.add_argument("--lung_hu_min", type=int, default=-1000)
    p.add_argument("--lung_hu_max", type=int, default=-150)
    p.add_argument("--skip_convert", action="store_true", help="only run the synthesis stage")
    p.add_argument("--postprocess_device", choices=["cpu", "cuda"], default="cpu",
                   help="where the synthesis stage merges and smooths the volume (cuda: cuda:{gpu_id})")
    p.add_argument("--pipeline", choices=["staged", "resident"], default="staged",
                   help="staged: generate() then synthesis() through the working directory; resident: one pass "
                        "per patient on the GPU (generate_synthesis), no working series unless --write_working; "
                        "with --skip_convert the staged synthesis() runs on the working series either way")
    p.add_argument("--write_working", action="store_true",
                   help="--pipeline resident: also write the raw / soft_tissue / lung working series")
    p.add_argument("--apply_diffmap", action="store_true",
                   help="run the difference-map stage: the U-Net of --nmodel_path predicts a contrast difference map "
                        "from the NCCT series and apply_diffmap adds it to the merged volume before the smoothing")
    p.add_argument("--nmodel_path", type=str, default="./checkpoints/Normal_Map_Unet.pth",
                   help="--apply_diffmap: checkpoint of the normal-map U-Net (UNet3D or UNet3DLight)")
    p.add_argument("--diffmap_threshold", type=float, default=8,
                   help="--apply_diffmap: difference-map values below this are dropped")
    p.add_argument("--save_diff", action="store_true",
                   help="--apply_diffmap: write the predicted difference map as diff.npy into the patient's working "
                        "directory")
    p.add_argument("--synthesis", choices=["range", "enhancement"], default="range",
                   help="range: overwrite the NCCT inside each model's HU range (synthesis, sCECT v2); enhancement: "
                        "keep the NCCT and add each model's HU gain where it is significant (synthesis_test, sCECT v3)")
    p.add_argument("--enhancement_threshold", type=float, default=5.0,
                   help="--synthesis enhancement: a model's HU gain over the NCCT must exceed this to be added")
    p.add_argument("--enhancement_min_hu", type=float, default=-400.0,
                   help="--synthesis enhancement: voxels whose NCCT HU does not exceed this are left as they are")
    return p.parse_args(argv)


if __name__ == "__main__":
    a = get_args()
    soft_a, lung_a = _model_args(a, None, None)
    if a.pipeline == "resident" and not a.skip_convert:
        generate_synthesis(a, soft_a, lung_a)
    else:
        if a.pipeline == "resident":
            print("--skip_convert: running the staged synthesis stage on the working series (--pipeline resident "
                  "has no stage of its own to skip to)")
        if not a.skip_convert:
            generate(a, soft_a, lung_a)
        (synthesis_test if a.synthesis == "enhancement" else synthesis)(a, soft_a, lung_a)
