"""The difference-map model of the reference's modules/nmodel: the normal-map U-Net (model.py), its
inference entry points (inference.py), and its training (config.py, dataset.py, trainer.py)."""
from .config import Config, FastTrainConfig, LightConfig, StandardConfig  # noqa: F401
from .dataset import CTDiffDataset, get_dataloaders, split_ids  # noqa: F401
from .inference import (apply_predicted_diffmap_device, denormalize_diff, diffmap_tail, load_model,  # noqa: F401
                        normalize_hu, predict_volume, predict_volume_device)
from .model import UNet3D, UNet3DLight, fold, forward_folded  # noqa: F401
from .trainer import (UNetTrainer, build_model, reference_optimizer, reference_step, reference_update)  # noqa: F401
