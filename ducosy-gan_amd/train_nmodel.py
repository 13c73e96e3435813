"""Train the normal-map U-Net (the model generate.py --apply_diffmap loads with --nmodel_path).

    python train_nmodel.py --model_type light --data_dir data --output_dir output

The flags are the fields of modules/nmodel/config.py (defaults: the preset of --model_type), plus
--resume [PATH] and --mma.  Data layout: <data_dir>/vue_files/<id>_vue.npy and
<data_dir>/diff_map/<id>_diff.npy (modules/nmodel/dataset.py); prepare_nmodel_data.py builds both from
DICOM pairs (NCCT and CECT series of one acquisition) into --data_dir.  Checkpoints go to
<output_dir>/checkpoints: latest.pth, best.pth, epoch_N.pth.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from modules.nmodel.config import LightConfig, StandardConfig  # noqa: E402

_FIXED = ("checkpoint_dir", "resume_path", "log_dir", "inference_checkpoint", "output_dir", "data_dir", "model_type",
          "resume")


def _flag(v: str) -> bool:
    if v.lower() in ("1", "true", "yes", "on"):
        return True
    if v.lower() in ("0", "false", "no", "off"):
        return False
    raise argparse.ArgumentTypeError(f"a boolean expected, got {v!r}")


def get_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model_type", choices=("light", "standard"), default="standard")
    ap.add_argument("--data_dir", default="data")
    ap.add_argument("--output_dir", default="output")
    ap.add_argument("--resume", nargs="?", const="", default=None, metavar="PATH",
                    help="continue from a checkpoint (default: <output_dir>/checkpoints/latest.pth)")
    ap.add_argument("--mma", default=None, help="operand mode of the device step (modules/hip/ops.py); default: f16 with "
                                                "--use_mixed_precision true, else the process's mode")
    ap.add_argument("--device", default="cuda")
    for key, value in vars(StandardConfig(make_dirs=False)).items():
        if key in _FIXED:
            continue
        if isinstance(value, bool):
            ap.add_argument(f"--{key}", type=_flag, default=None)
        elif isinstance(value, tuple):
            ap.add_argument(f"--{key}", type=int, nargs=len(value), default=None)
        else:
            ap.add_argument(f"--{key}", type=type(value), default=None)
    return ap.parse_args(argv)


def make_config(args):
    config = (LightConfig if args.model_type == "light" else StandardConfig)(make_dirs=False)
    for key in vars(config):
        v = getattr(args, key, None)
        if key not in _FIXED and v is not None:
            setattr(config, key, tuple(v) if isinstance(getattr(config, key), tuple) else v)
    config.data_dir = args.data_dir
    config.set_output_dir(args.output_dir)
    if args.resume is not None:
        config.resume = True
        config.resume_path = args.resume or config.resume_path
    return config


def main(argv=None):
    args = get_args(argv)
    config = make_config(args)
    import torch
    from modules.nmodel.dataset import get_dataloaders
    from modules.nmodel.trainer import UNetTrainer, build_model
    print(config)
    trainer = UNetTrainer(build_model(config), config, device=args.device, mma=args.mma)
    if config.resume:
        trainer.load(config.resume_path)
        print(f"resumed from {config.resume_path} at epoch {trainer.epoch}")
    train_loader, val_loader = get_dataloaders(config.data_dir, batch_size=config.batch_size,
                                               num_workers=config.num_workers, val_size=config.val_size,
                                               use_patches=config.use_patches, patch_size=tuple(config.patch_size),
                                               patches_per_volume=config.patches_per_volume)
    config.save(os.path.join(config.output_dir, "config.json"))
    history = trainer.fit(train_loader, val_loader)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    return history


if __name__ == "__main__":
    main()
