"""Organ masking of the three evaluated series (reference masking.py::masking, :383-564).

    python masking.py --input_dir_root IN --output_dir_root OUT --dataset_names NAME [--device cuda]

For every patient of IN/{dataset} it reads the modified label volume
OUT/modified_mask/{dataset}/{patient}.nii (modify_heart_mask.py writes it), builds the organ mask
(modules/organ_masks.py::organ_mask: 34 labels filled and thickened per slice) and writes copies of
the NCCT, CECT and sCECT slices with the masked pixels set to 9999 to
OUT/masked/{dataset}/{patient}/{ncct_folder | cect_folder | generated}/{basename}, int16 Explicit VR
Little Endian, which is where ``calculate.py --mask`` reads them.  The directory layout, the slice
order (InstanceNumber) and the skip rules with their printed reasons are the reference's.

--device cpu (the default) computes on the host; --device cuda computes the organ mask and the
apply pass on the MI355X (modules/hip/organ_masks.py).  Both write byte-identical files.

generate() of the reference runs TotalSegmentator, whose weights are downloaded; it is not part
of this package, and its output, a plain multi-label NIfTI volume, is this stage's input.
"""
from __future__ import annotations

import argparse
import glob
import os

import numpy as np

from modules import dicom, nifti
from modules import organ_masks as OM
from modules.argmanager import get_common_infer_args


def get_args(argv=None):
    args = get_common_infer_args(argv)
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument("--device", choices=["cpu", "cuda"], default="cpu")
    extra, _ = p.parse_known_args(argv)
    args.device = extra.device
    return args


def generate(args):
    mask_dir = os.path.join(args.output_dir_root, "mask")
    raise RuntimeError(
        "masking.generate: TotalSegmentator is not part of this package (its weights are downloaded). Run it "
        f"elsewhere and place its multi-label volume at {os.path.join(mask_dir, '{dataset}', '{patient}.nii')}; "
        "modify_heart_mask.py and masking() take it from there.")


def label_volume(path: str) -> np.ndarray:
    """The label volume as uint8 [z, y, x].  Values that are no integer in 0..255 can equal no
    label (the reference compares the float volume with each label), so they read as 0."""
    data = nifti.read(path).get_fdata_zyx()
    ok = (data >= 0) & (data <= 255) & (data == np.floor(data))
    return np.ascontiguousarray(np.where(ok, data, 0).astype(np.uint8))


def _sorted_slices(folder: str):
    files = sorted(glob.glob(os.path.join(folder, "*.dcm")))
    files.sort(key=lambda f: int(dicom.dcmread(f, stop_before_pixels=True).InstanceNumber))
    return files


def _masked_series(labels, stacks, device):
    """The three int16 stacks [n, H, W] with the organ mask of ``labels`` [z, y, x] applied."""
    n = stacks[0].shape[0]
    if device is None:
        mask = OM.organ_mask(labels)[:n]
        return [OM.apply_organ_mask(s, mask) for s in stacks]
    import torch
    from modules.hip import organ_masks as G
    with torch.cuda.device(device):
        mask = G.organ_mask(torch.from_numpy(labels).to(device))[:n].contiguous()
        outs = G.apply_organ_mask(*(torch.from_numpy(s).to(device) for s in stacks), mask)
        return [o.cpu().numpy() for o in outs]


def _save(src_path: str, pixels: np.ndarray, dst_path: str):
    dcm = dicom.dcmread(src_path)
    dcm.file_meta.TransferSyntaxUID = dicom.EXPLICIT_VR_LE
    dcm.PixelData = pixels.astype("<i2").tobytes()
    if dcm.get("PhotometricInterpretation") in ("YBR_FULL_422", "YBR_FULL"):
        dcm.PhotometricInterpretation = "MONOCHROME2"
    dcm.save_as(dst_path)


def masking(args):
    device = f"cuda:{args.gpu_id}" if getattr(args, "device", "cpu") == "cuda" else None
    mask_dir = os.path.join(args.output_dir_root, "modified_mask")
    masked_dir = os.path.join(args.output_dir_root, "masked")
    os.makedirs(masked_dir, exist_ok=True)
    for dataset in args.dataset_names:
        original = os.path.join(args.input_dir_root, dataset)
        generated = os.path.join(args.output_dir_root, dataset)
        patients = sorted(d for d in glob.glob(os.path.join(original, "*")) if os.path.isdir(d))
        ncct_dirs = [os.path.join(d, args.ncct_folder) for d in patients]
        cect_dirs = [os.path.join(d, args.cect_folder) for d in patients]
        scect_dirs = sorted(d for d in glob.glob(os.path.join(generated, "*")) if os.path.isdir(d))
        if not len(ncct_dirs) == len(cect_dirs) == len(scect_dirs):
            print(f"Mismatch in number of patient directories among NCCT, CECT, and SCECT for dataset {dataset}. "
                  "Skipping.")
            continue
        os.makedirs(os.path.join(masked_dir, dataset), exist_ok=True)
        print(f"\nApplying masks for dataset: {dataset} (device: {device or 'cpu'})")
        for ncct_dir, cect_dir, scect_dir in zip(ncct_dirs, cect_dirs, scect_dirs):
            patient = os.path.basename(scect_dir)
            if patient not in cect_dir:
                print(f"Patient ID mismatch between CECT and SCECT directories: {cect_dir}, {scect_dir}. Skipping.")
                continue
            out_dirs = [os.path.join(masked_dir, dataset, patient, sub)
                        for sub in (args.ncct_folder, args.cect_folder, "generated")]
            for d in out_dirs:
                os.makedirs(d, exist_ok=True)
            files, missing = [], None
            for name, folder in (("NCCT", ncct_dir), ("CECT", cect_dir), ("SCECT", scect_dir)):
                found = _sorted_slices(folder)
                if not found and missing is None:
                    missing = name
                files.append(found)
            if missing:
                print(f"No {missing} DICOM files found for patient {patient}, skipping.")
                continue
            mask_path = os.path.join(mask_dir, dataset, patient + ".nii")
            if not os.path.exists(mask_path):
                print(f"Mask file not found for patient {patient}, skipping masking.")
                continue
            labels = label_volume(mask_path)
            nz = labels.shape[0]
            if len(files[1]) != nz and len(files[2]) != nz:
                print(f"Slice count mismatch for patient {patient}, skipping.")
                continue
            # the reference zips the three lists and indexes the mask by position
            n = min(nz, *(len(f) for f in files))
            stacks = [np.stack([dicom.dcmread(f).pixel_array for f in fl[:n]]).astype(np.int16) for fl in files]
            if any(s.shape[1:] != labels.shape[1:] for s in stacks):
                print(f"Slice shape mismatch for patient {patient}, skipping.")
                continue
            for fl, out_dir, masked in zip(files, out_dirs, _masked_series(labels, stacks, device)):
                for path, pixels in zip(fl, masked):
                    _save(path, pixels, os.path.join(out_dir, os.path.basename(path)))
    print("Masking process completed!")
    print(f"Masked DICOMs saved in: {masked_dir}")


def main(argv=None):
    masking(get_args(argv))


if __name__ == "__main__":
    main()
