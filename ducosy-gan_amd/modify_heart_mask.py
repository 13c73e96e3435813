"""Cut the outflow vessels off the heart label of a multi-label volume (reference
modify_heart_mask.py).

    python modify_heart_mask.py --output_dir_root OUT --dataset_names NAME [--device cuda]

Reads OUT/mask/{dataset}/{patient}.nii (TotalSegmentator's output) and writes
OUT/modified_mask/{dataset}/{patient}.nii, the input of masking.py, with the source header's
geometry kept.  The reference hard-codes its paths; here they come from the common inference
arguments.  It also loads the NCCT DICOM volume, but only for sample images whose writer is
commented out, so nothing else is read here.

--device cpu (the default) runs modules/organ_masks.py::modify_heart_label; --device cuda runs
modules/hip/organ_masks.py on the MI355X.  Both write byte-identical files.
"""
from __future__ import annotations

import argparse
import os

import numpy as np

from modules import nifti
from modules import organ_masks as OM
from modules.argmanager import get_common_infer_args


def get_args(argv=None):
    args = get_common_infer_args(argv)
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument("--device", choices=["cpu", "cuda"], default="cpu")
    extra, _ = p.parse_known_args(argv)
    args.device = extra.device
    return args


def modify_file(src: str, dst: str, device=None) -> None:
    vol = nifti.read(src)
    labels = vol.labels_zyx()
    if device is None:
        out_xyz = OM.modify_heart_label(labels.T)
    else:
        import torch
        from modules.hip import organ_masks as G
        with torch.cuda.device(device):
            out_xyz = G.modify_heart_label(torch.from_numpy(labels).to(device)).cpu().numpy().T
    nifti.write_labels(dst, np.asarray(out_xyz), vol)


def main(argv=None):
    args = get_args(argv)
    device = f"cuda:{args.gpu_id}" if args.device == "cuda" else None
    for dataset in args.dataset_names:
        mask_dir = os.path.join(args.output_dir_root, "mask", dataset)
        if not os.path.isdir(mask_dir):
            print(f"Mask directory not found: {mask_dir}. Skipping.")
            continue
        out_dir = os.path.join(args.output_dir_root, "modified_mask", dataset)
        os.makedirs(out_dir, exist_ok=True)
        for name in sorted(f for f in os.listdir(mask_dir) if f.endswith(".nii")):
            modify_file(os.path.join(mask_dir, name), os.path.join(out_dir, name), device)
            print(f"  {dataset} {name}: modified (device: {device or 'cpu'})")


if __name__ == "__main__":
    main()
