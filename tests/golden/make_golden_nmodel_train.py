"""Golden training-step results of the reference's normal-map U-Net (modules/nmodel/model.py) for
tests/test_cpu_nmodel_train.py and tests/test_gpu_nmodel_train.py.

Run ONLY in the build container, where /root/reference exists:

    python tests/golden/make_golden_nmodel_train.py      # writes tests/golden/nmodel_train.npz

The reference module is imported from its file and run on the CPU in training mode on one
micro-batch [N,1,1,H,W] of depth-1 patches: loss = mean |model(x) - target|, backward, in float64
(model.double()) and in float32.  Weights come from make_golden_nmodel.seeded_state, inputs and
targets from oracle/prng.py streams, so the tests rebuild them; only results are written.

A ReLU, pool-argmax or sign decision that flips within rounding changes a deep layer's gradient at
the percent level, so a case's seed is advanced until its smallest |BatchNorm output|, its smallest
top-two gap of a pool window with a positive maximum and its smallest |output - target| are all at
least MARGIN.  The seed used and the three margins are written with the case.

Importing this file does not need the reference.
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
REF = os.environ.get("DUCOSY_REFERENCE", "/root/reference")
OUT = os.path.join(HERE, "nmodel_train.npz")
MARGIN = 1e-5
SAMPLES = 64          # entries per parameter a "sampled" case stores
PRESETS = ("Config", "LightConfig", "StandardConfig", "FastTrainConfig")

# case -> (class name, base channels, first seed, N, H, W, store full gradients)
CASES = {
    "t1": ("UNet3DLight", 8, 21, 2, 28, 20, True),
    "t2": ("UNet3D", 8, 31, 2, 48, 32, False),
}


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _load("make_golden_nmodel", os.path.join(HERE, "make_golden_nmodel.py"))


def _prng():
    return G._prng()


def case_batch(case: str, seed: int):
    """(x, target) [N,H,W] float32 in [-1, 1) of a case at ``seed``."""
    _, _, _, n, h, w, _ = CASES[case]
    p = _prng()
    return p.uniform(seed, f"x:{case}", (n, h, w), -1.0, 1.0), p.uniform(seed, f"t:{case}", (n, h, w), -1.0, 1.0)


def sample_index(case: str, seed: int, name: str, numel: int) -> np.ndarray:
    """The SAMPLES flat indices of parameter ``name`` a sampled case stores."""
    u = _prng().uniform(seed, f"idx:{case}:{name}", (SAMPLES,), 0.0, 1.0).astype(np.float64)
    return np.minimum((u * numel).astype(np.int64), numel - 1)


def trained_view(name: str, t):
    """The part of a parameter (or of its gradient) the depth-1 step trains: the centre depth tap of
    a 3x3x3 weight, everything else whole."""
    return t[:, :, 1] if t.dim() == 5 and t.shape[2] == 3 else t


def run_step(model, x, target, dtype, hooks=False):
    """One training-mode forward + backward of ``model`` (reference or mirror) in ``dtype``.  Returns
    (loss, {name: gradient}, {name: buffer after the step}, margins or None)."""
    import torch
    import torch.nn as nn
    model = model.to(dtype).train()
    model.zero_grad(set_to_none=True)
    margins = {"bn": float("inf"), "pool": float("inf"), "sign": float("inf")}
    handles = []
    if hooks:
        def bn_hook(_m, _inp, out):   # runs before the in-place ReLU
            margins["bn"] = min(margins["bn"], float(out.detach().abs().min()))

        def pool_hook(_m, inp):
            a = inp[0].detach()[:, :, 0]
            n, c, h, w = a.shape
            win = a[:, :, :h // 2 * 2, :w // 2 * 2].reshape(n, c, h // 2, 2, w // 2, 2).permute(0, 1, 2, 4, 3, 5)
            top = win.reshape(n, c, h // 2, w // 2, 4).sort(dim=-1, descending=True).values
            gap = (top[..., 0] - top[..., 1])[top[..., 0] > 0]
            if gap.numel():
                margins["pool"] = min(margins["pool"], float(gap.min()))

        for m in model.modules():
            if isinstance(m, nn.BatchNorm3d):
                handles.append(m.register_forward_hook(bn_hook))
            elif isinstance(m, nn.MaxPool3d):
                handles.append(m.register_forward_pre_hook(pool_hook))
    xt = torch.from_numpy(x).to(dtype)[:, None, None]
    tt = torch.from_numpy(target).to(dtype)[:, None, None]
    out = model(xt)
    loss = (out - tt).abs().mean()
    loss.backward()
    for h in handles:
        h.remove()
    margins["sign"] = float((out.detach() - tt).abs().min())
    grads = {k: p.grad.detach() for k, p in model.named_parameters()}
    bufs = {k: b.detach().clone() for k, b in model.named_buffers()}
    return float(loss.detach()), grads, bufs, margins if hooks else None


def main():
    import torch
    ref = _load("ref_nmodel_model", os.path.join(REF, "modules", "nmodel", "model.py"))
    out = {}
    for case, (cls, base, seed0, n, h, w, full) in CASES.items():
        shapes = {k: tuple(v.shape) for k, v in getattr(ref, cls)(base_channels=base).state_dict().items()}
        state = {k: torch.from_numpy(np.asarray(v)) for k, v in G.seeded_state(shapes, seed0).items()}

        def fresh():
            m = getattr(ref, cls)(base_channels=base)
            m.load_state_dict(state)
            return m

        seed = seed0
        while True:
            x, t = case_batch(case, seed)
            loss64, g64, b64, margins = run_step(fresh(), x, t, torch.float64, hooks=True)
            if min(margins.values()) >= MARGIN:
                break
            print(case, "seed", seed, "margins", margins, "-> next seed")
            seed += 1
        loss32, g32, _, _ = run_step(fresh(), x, t, torch.float32)
        out[f"{case}:seed"] = np.array(seed, dtype=np.int64)
        out[f"{case}:margins"] = np.array([margins["bn"], margins["pool"], margins["sign"]])
        out[f"{case}:loss"] = np.array(loss64)
        names = list(g64)
        out[f"{case}:names"] = np.array(names)
        norms, deltas = [], []
        for k in names:
            a = g64[k]
            if a.dim() == 5 and a.shape[2] == 3:   # the off-centre taps multiply zero padding
                assert float(a[:, :, 0].abs().max()) == 0.0 and float(a[:, :, 2].abs().max()) == 0.0, k
            a64 = trained_view(k, a).contiguous().reshape(-1)
            a32 = trained_view(k, g32[k]).contiguous().reshape(-1).double()
            norms.append(float(a64.norm()))
            deltas.append(float((a32 - a64).norm() / a64.norm()))
            if full:
                out[f"{case}:grad:{k}"] = a64.numpy().astype(np.float32)
            else:
                out[f"{case}:grad:{k}"] = a64.numpy()[sample_index(case, seed, k, a64.numel())].astype(np.float32)
        out[f"{case}:norms"] = np.array(norms)
        out[f"{case}:delta32"] = np.array(deltas)
        for k, b in b64.items():
            if not k.endswith("num_batches_tracked"):
                out[f"{case}:buf:{k}"] = b.numpy()
            else:
                assert int(b) == 101
        print(case, cls, base, "seed", seed, "loss", loss64, "| loss32 - loss64 |", abs(loss32 - loss64), "margins", margins,
              "delta32 min/max", min(deltas), max(deltas))
    # the recipe: the fields of the reference's Config presets (its constructor makes directories)
    import json
    import tempfile
    cfg = _load("ref_nmodel_config", os.path.join(REF, "modules", "nmodel", "config.py"))
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            for preset in PRESETS:
                d = {k: v for k, v in vars(getattr(cfg, preset)()).items() if k != "log_dir"}
                out[f"cfg:{preset}"] = np.array(json.dumps(d, sort_keys=True))
        finally:
            os.chdir(cwd)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
