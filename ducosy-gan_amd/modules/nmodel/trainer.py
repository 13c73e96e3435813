"""Training the normal-map U-Net (UNet3D / UNet3DLight) by the recipe of the reference's
modules/nmodel/config.py: depth-1 patches, L1 loss, gradient accumulation, a global-norm gradient
clip and Adam.  The reference ships the recipe's pieces and no trainer; what it leaves open is
fixed in config.py's docstring.

``reference_step`` / ``reference_update`` are the recipe in plain ATen on any device and dtype: the
CPU path and the test oracle.  ``UNetTrainer`` on a GPU runs the step on the HIP kernels
(modules/hip/unet_train.py) and validates through the inference plan (modules/hip/unet.py); on the
CPU it runs the ATen functions.  Checkpoints carry ``model_state_dict`` and ``config`` as
``load_model`` (here and in the reference) reads them, plus ``optimizer_state_dict``, ``epoch`` and
``best_val_loss``.
"""
from __future__ import annotations

import contextlib
import os
from typing import Optional

import torch

from .model import UNet3D, UNet3DLight


def build_model(config):
    """The model a Config describes: 'light' -> UNet3DLight, 'standard' -> UNet3D."""
    kinds = {"light": UNet3DLight, "standard": UNet3D}
    if config.model_type not in kinds:
        raise ValueError(f"model_type must be one of {sorted(kinds)}")
    return kinds[config.model_type](n_channels=config.in_channels, n_classes=config.out_channels,
                                    base_channels=config.base_channels)


def check_supported(model, config) -> None:
    """What the trainer covers; everything else is a ValueError, as on the inference path."""
    if int(tuple(config.patch_size)[0]) != 1:
        raise ValueError("the trainer covers depth-1 patches only (patch_size[0] == 1)")
    if float(config.ssim_weight) != 0.0:
        raise ValueError("the trainer covers the L1 loss only (ssim_weight == 0)")
    if not getattr(model, "trilinear", True):
        raise ValueError("the trainer covers trilinear=True models only")
    if getattr(model, "n_channels", 1) != 1 or getattr(model, "n_classes", 1) != 1:
        raise ValueError("the trainer covers one input channel and one output channel")
    if int(config.gradient_accumulation_steps) < 1:
        raise ValueError("gradient_accumulation_steps must be at least 1")


# ---------------------------------------------------------------------------------------
# the recipe in ATen
# ---------------------------------------------------------------------------------------
def reference_step(model, x, target, accumulation: int = 1, l1_weight: float = 1.0):
    """One micro-batch in training mode: loss = l1_weight * mean |model(x) - target| / accumulation,
    backward into the parameters' ``.grad`` (added to what is there).  Returns the detached loss."""
    model.train()
    loss = (model(x) - target).abs().mean() * (l1_weight / accumulation)
    loss.backward()
    return loss.detach()


def reference_optimizer(model, lr: float):
    return torch.optim.Adam(model.parameters(), lr=lr)


def reference_update(model, optimizer, clip: Optional[float] = None):
    """clip_grad_norm_ (when ``clip``), one optimizer step, gradients reset.  Returns the norm."""
    params = [p for p in model.parameters() if p.grad is not None]
    norm = torch.nn.utils.clip_grad_norm_(params, clip) if clip else \
        torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad) for p in params]))
    optimizer.step()
    optimizer.zero_grad(set_to_none=True)
    return norm


# ---------------------------------------------------------------------------------------
# the trainer
# ---------------------------------------------------------------------------------------
@contextlib.contextmanager
def _operand_mode(mode: Optional[str]):
    if mode is None:
        yield
        return
    from ..hip import ops
    before = ops.get_mma()
    ops.set_mma(mode)
    try:
        yield
    finally:
        ops.set_mma(before)


class UNetTrainer:
    """``train_step`` runs one micro-batch and optimizes once every
    ``config.gradient_accumulation_steps`` calls; ``validate`` is the mean L1 of a loader in eval
    mode; ``fit`` loops over epochs and writes latest.pth, best.pth and epoch_N.pth.

    ``mma``: the operand mode of the device step (modules/hip/ops.py); default 'f16' with
    ``config.use_mixed_precision``, else the process's mode."""

    def __init__(self, model, config, device="cuda", mma: Optional[str] = None):
        check_supported(model, config)
        self.config, self.device = config, torch.device(device)
        self.model = model.to(self.device)
        self.accum = int(config.gradient_accumulation_steps)
        self.clip = float(config.gradient_clip_value) if config.gradient_clip_value else None
        self.lr = float(config.learning_rate)
        self.calls, self.epoch, self.best_val_loss = 0, 0, float("inf")
        self.on_gpu = self.device.type == "cuda"
        if self.on_gpu:
            from ..hip.unet_train import TrainState
            self.mma = mma if mma is not None else ("f16" if config.use_mixed_precision else None)
            self.state = TrainState(self.model, self.device)
        else:
            self.mma, self.state = None, None
            self.optimizer = reference_optimizer(self.model, self.lr)

    # ---- one micro-batch -----------------------------------------------------------------
    def train_step(self, x: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        """x, target: [N,1,1,H,W].  Returns this micro-batch's loss term (already divided by the
        accumulation count) as a tensor on the device; no host synchronisation."""
        x, target = x.to(self.device), target.to(self.device)
        if x.dim() != 5 or x.shape[2] != 1:
            raise ValueError("the trainer covers depth-1 patches only: [N,1,1,H,W]")
        gscale = float(self.config.l1_weight) / self.accum
        self.calls += 1
        if self.on_gpu:
            self.model.train()
            with _operand_mode(self.mma):
                loss = self.state.accumulate(x.float(), target.float(), gscale).reshape(())
                if self.calls % self.accum == 0:
                    self.state.step(self.lr, self.clip)
            return loss
        loss = reference_step(self.model, x, target, self.accum, float(self.config.l1_weight))
        if self.calls % self.accum == 0:
            reference_update(self.model, self.optimizer, self.clip)
        return loss

    # ---- validation ----------------------------------------------------------------------
    @torch.no_grad()
    def _eval_loss(self, x: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if not self.on_gpu:
            return (self.model(x) - target).abs().mean()
        from ..hip import ops, unet as U
        from ..hip.unet_train import l1_out
        N, _, _, H, W = x.shape
        with torch.cuda.device(self.device), _operand_mode(self.mma):
            plan = U.plan_for(self.model, self.device)
            y, last = U.forward(plan, ops.pack_nhwc4(x.float().reshape(N, 1, H, W)))
            return l1_out(y, last.scale, last.shift, plan.out_weight, self.state.bout,
                          target.float().reshape(N, H, W).contiguous())[0].reshape(())

    def validate(self, loader) -> float:
        """Mean over the loader's batches of mean |model(x) - target| in eval mode."""
        self.model.eval()
        total, n = None, 0
        for batch in loader:
            loss = self._eval_loss(batch["input"].to(self.device), batch["target"].to(self.device))
            total = loss if total is None else total + loss
            n += 1
        return float(total) / n if n else float("nan")

    # ---- checkpoints ---------------------------------------------------------------------
    def _config_dict(self) -> dict:
        cfg = {k: (list(v) if isinstance(v, tuple) else v) for k, v in vars(self.config).items()}
        cfg.update(base_channels=int(self.model.base_channels), in_channels=int(self.model.n_channels),
                   out_channels=int(self.model.n_classes), model_type=self.config.model_type)
        return cfg

    def save(self, path: str) -> None:
        sd = {k: v.detach().cpu().clone() for k, v in self.model.state_dict().items()}
        opt = self.state.optimizer_state_dict() if self.on_gpu else self.optimizer.state_dict()
        torch.save({"model_state_dict": sd, "config": self._config_dict(), "optimizer_state_dict": opt,
                    "epoch": self.epoch, "best_val_loss": self.best_val_loss}, path)

    def load(self, path: str) -> None:
        """Resume: parameters, BatchNorm buffers, optimizer state, epoch and best validation loss."""
        ckpt = torch.load(path, map_location="cpu", weights_only=True)
        self.model.load_state_dict(ckpt["model_state_dict"])
        if self.on_gpu:
            from ..hip.unet_train import TrainState
            self.state = TrainState(self.model, self.device)
            self.state.load_optimizer_state_dict(ckpt["optimizer_state_dict"])
        else:
            self.optimizer.load_state_dict(ckpt["optimizer_state_dict"])
        self.epoch = int(ckpt.get("epoch", 0))
        self.best_val_loss = float(ckpt.get("best_val_loss", float("inf")))

    # ---- the loop ------------------------------------------------------------------------
    def fit(self, train_loader, val_loader=None, num_epochs: Optional[int] = None, checkpoint_dir: Optional[str] = None,
            log=print) -> dict:
        """Epochs ``self.epoch`` .. ``num_epochs`` - 1.  After each: latest.pth, best.pth when the
        validation loss improved, epoch_N.pth every ``save_interval`` epochs."""
        num_epochs = int(self.config.num_epochs if num_epochs is None else num_epochs)
        ckdir = checkpoint_dir or self.config.checkpoint_dir
        os.makedirs(ckdir, exist_ok=True)
        history = {"train": [], "val": []}
        for epoch in range(self.epoch, num_epochs):
            total, n = None, 0
            for batch in train_loader:
                loss = self.train_step(batch["input"], batch["target"])
                total = loss if total is None else total + loss
                n += 1
            train_loss = float(total) * self.accum / n if n else float("nan")
            val_loss = self.validate(val_loader) if val_loader is not None else train_loss
            self.epoch = epoch + 1
            history["train"].append(train_loss)
            history["val"].append(val_loss)
            log(f"epoch {self.epoch}/{num_epochs}: train L1 {train_loss:.6f}, val L1 {val_loss:.6f}")
            best = val_loss < self.best_val_loss
            if best:
                self.best_val_loss = val_loss
            self.save(os.path.join(ckdir, "latest.pth"))
            if best:
                self.save(os.path.join(ckdir, "best.pth"))
            if self.config.save_interval and self.epoch % int(self.config.save_interval) == 0:
                self.save(os.path.join(ckdir, f"epoch_{self.epoch}.pth"))
        return history
