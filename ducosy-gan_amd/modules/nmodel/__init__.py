"""The difference-map model of the reference's modules/nmodel: the normal-map U-Net (model.py) and
its inference entry points (inference.py)."""
from .inference import (apply_predicted_diffmap_device, denormalize_diff, diffmap_tail, load_model,  # noqa: F401
                        normalize_hu, predict_volume, predict_volume_device)
from .model import UNet3D, UNet3DLight, fold, forward_folded  # noqa: F401
