"""Training configuration of the normal-map U-Net: the fields, defaults and presets of the
reference's modules/nmodel/config.py (Config, LightConfig, StandardConfig, FastTrainConfig, save,
load), restated.

What the fields mean to this project's trainer (modules/nmodel/trainer.py) where the reference
leaves it open:

* the optimizer is Adam with torch's default betas and eps and no weight decay;
* ``gradient_clip_value`` is a global L2-norm clip (clip_grad_norm_);
* the loss is ``l1_weight`` * mean |output - target| over the micro-batch, divided by
  ``gradient_accumulation_steps``; ``ssim_weight`` must be 0;
* ``use_mixed_precision`` selects the ``f16`` operand mode of modules/hip/ops.py (accumulators stay
  float32, so there is no loss scaling);
* ``use_gradient_checkpointing`` is accepted and ignored.
"""
import json
import os
from datetime import datetime


class Config:
    def __init__(self, make_dirs: bool = True):
        # data
        self.data_dir = 'data'
        self.output_dir = 'output'
        # model: 'light' (UNet3DLight, base 16) or 'standard' (UNet3D, base 32)
        self.model_type = 'standard'
        self.in_channels = 1
        self.out_channels = 1
        self.base_channels = 16
        # patches: one slice per sample, every slice of a volume used
        self.use_patches = True
        self.patch_size = (1, 512, 512)   # (D, H, W)
        self.patches_per_volume = 128
        # schedule
        self.num_epochs = 100
        self.batch_size = 1
        self.learning_rate = 5e-5
        self.num_workers = 2
        self.gradient_accumulation_steps = 8
        self.use_mixed_precision = True
        self.use_gradient_checkpointing = True
        self.gradient_clip_value = 1.0
        # loss
        self.l1_weight = 1.0
        self.ssim_weight = 0.0
        # split: train / val only
        self.val_size = 0.15
        # checkpoints
        self.checkpoint_dir = os.path.join(self.output_dir, 'checkpoints')
        self.save_interval = 10
        self.resume = False
        self.resume_path = os.path.join(self.checkpoint_dir, 'latest.pth')
        # logs
        stamp = datetime.now().strftime('%Y%m%d_%H%M%S')
        self.log_dir = os.path.join(self.output_dir, 'logs', f'unet_{stamp}')
        # inference
        self.inference_checkpoint = os.path.join(self.checkpoint_dir, 'best.pth')
        if make_dirs:
            self.make_dirs()

    def make_dirs(self):
        for d in (self.checkpoint_dir, self.log_dir, self.output_dir):
            os.makedirs(d, exist_ok=True)

    def set_output_dir(self, output_dir: str, make_dirs: bool = True):
        """Point every derived path (checkpoints, logs, resume and inference checkpoints) below
        ``output_dir``: the constructor derives them from the default once."""
        self.output_dir = output_dir
        self.checkpoint_dir = os.path.join(output_dir, 'checkpoints')
        self.resume_path = os.path.join(self.checkpoint_dir, 'latest.pth')
        self.inference_checkpoint = os.path.join(self.checkpoint_dir, 'best.pth')
        self.log_dir = os.path.join(output_dir, 'logs', os.path.basename(self.log_dir))
        if make_dirs:
            self.make_dirs()

    def __repr__(self):
        bar = "=" * 50
        rows = "".join(f"{k:20s}: {v}\n" for k, v in self.__dict__.items())
        return f"{bar}\nConfiguration\n{bar}\n{rows}{bar}"

    def save(self, save_path):
        with open(save_path, 'w') as f:
            json.dump(self.__dict__, f, indent=4)
        print(f"Config saved to {save_path}")

    @classmethod
    def load(cls, load_path):
        config = cls()
        with open(load_path, 'r') as f:
            for key, value in json.load(f).items():
                setattr(config, key, value)
        print(f"Config loaded from {load_path}")
        return config


class LightConfig(Config):
    def __init__(self, make_dirs: bool = True):
        super().__init__(make_dirs)
        self.model_type = 'light'
        self.base_channels = 16
        self.batch_size = 1


class StandardConfig(Config):
    def __init__(self, make_dirs: bool = True):
        super().__init__(make_dirs)
        self.model_type = 'standard'
        self.base_channels = 32
        self.batch_size = 1


class FastTrainConfig(Config):
    def __init__(self, make_dirs: bool = True):
        super().__init__(make_dirs)
        self.model_type = 'light'
        self.base_channels = 8
        self.num_epochs = 10
        self.batch_size = 1
