"""Golden outputs of the reference's normal-map U-Net (modules/nmodel/model.py) for
tests/test_cpu_nmodel.py and tests/test_gpu_nmodel.py.

Run ONLY in the build container, where /root/reference exists:

    python tests/golden/make_golden_nmodel.py      # writes tests/golden/nmodel_unet.npz

The reference module needs only torch; it is imported from its file and run on the CPU, one
[1,1,1,H,W] slice at a time as its predict_volume does, in float64 (model.double()) and float32.
Weights and BatchNorm running statistics come from oracle/prng.py streams keyed by the state_dict
names (``seeded_state``), so the tests rebuild them; only key / shape lists, inputs and outputs are
written.  Importing this file does not need the reference.
"""
import importlib.util
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
REF = os.environ.get("DUCOSY_REFERENCE", "/root/reference")
OUT = os.path.join(HERE, "nmodel_unet.npz")

# case -> (class name, base channels, weight seed, slices, H, W)
CASES = {
    "a": ("UNet3DLight", 16, 11, 3, 28, 20),   # 28->14->7->3, 20->10->5->2: pad split on both axes, two levels
    "b": ("UNet3DLight", 16, 11, 2, 64, 64),   # no pad
    "c": ("UNet3D", 8, 12, 2, 48, 32),         # 4 downs; 48->..->3, 32->..->2, one pad
    "d": ("UNet3DLight", 16, 11, 1, 8, 8),     # reaches a 1-pixel axis: the align_corners corner case
}
LISTED = {"light16": ("UNet3DLight", 16), "full8": ("UNet3D", 8), "full32": ("UNet3D", 32)}


def _prng():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from oracle import prng
    return prng


def seeded_state(shapes: dict, seed: int) -> dict:
    """{name: float32 / int64 array} for a U-Net state_dict given {name: shape}: He-scaled conv
    weights, BatchNorm gamma in +-[0.5, 1.5) with about 3 in 10 negative, beta in [-0.3, 0.3), running
    mean ~ N(0, 0.3), running variance in [0.5, 1.5)."""
    prng = _prng()
    out = {}
    for name, shape in shapes.items():
        shape = tuple(int(s) for s in shape)
        leaf = name.rsplit(".", 1)[-1]
        if leaf == "num_batches_tracked":
            out[name] = np.array(100, dtype=np.int64)
        elif len(shape) == 5:
            fan_in = shape[1] * shape[3] * shape[4]   # the taps a one-slice forward sees
            out[name] = prng.normal(seed, name, shape, 0.0, math.sqrt(2.0 / fan_in))
        elif leaf == "running_mean":
            out[name] = prng.normal(seed, name, shape, 0.0, 0.3)
        elif leaf == "running_var":
            out[name] = prng.uniform(seed, name, shape, 0.5, 1.5)
        elif leaf == "weight":                         # BatchNorm gamma, both signs
            sign = 1.0 - 2.0 * prng.bernoulli(seed, name + "#sign", shape, 0.3)
            out[name] = (prng.uniform(seed, name, shape, 0.5, 1.5) * sign).astype(np.float32)
        elif name.startswith("outc."):                 # the 1x1 convolution's bias
            out[name] = prng.uniform(seed, name, shape, -0.1, 0.1)
        else:                                          # BatchNorm beta
            out[name] = prng.uniform(seed, name, shape, -0.3, 0.3)
    return out


def case_input(case: str) -> np.ndarray:
    """[slices, H, W] float32 in [-1, 1): the normalised slices of a case."""
    _, _, seed, n, h, w = CASES[case]
    return _prng().uniform(seed, f"x:{case}", (n, h, w), -1.0, 1.0)


def main():
    import torch
    spec = importlib.util.spec_from_file_location("ref_nmodel_model", os.path.join(REF, "modules", "nmodel", "model.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {}
    for tag, (cls, base) in LISTED.items():
        sd = getattr(ref, cls)(base_channels=base).state_dict()
        out[f"keys:{tag}"] = np.array(list(sd))
        out[f"shapes:{tag}"] = np.array([",".join(str(int(s)) for s in v.shape) for v in sd.values()])
    for case, (cls, base, seed, n, h, w) in CASES.items():
        model = getattr(ref, cls)(base_channels=base).eval()
        state = seeded_state({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed)
        model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
        x = case_input(case)
        ys = {}
        with torch.no_grad():
            for name, dt in (("y32", torch.float32), ("y64", torch.float64)):
                model = model.to(dt)
                ys[name] = np.stack([model(torch.from_numpy(x[i]).to(dt)[None, None, None])[0, 0, 0].numpy()
                                     for i in range(n)])
        out[f"x:{case}"] = x
        out[f"y32:{case}"] = ys["y32"]
        out[f"y64:{case}"] = ys["y64"]
        out[f"delta32:{case}"] = np.array(np.abs(ys["y32"].astype(np.float64) - ys["y64"]).max())
        print(case, cls, base, x.shape, "max|y64|", float(np.abs(ys["y64"]).max()), "delta32", float(out[f"delta32:{case}"]))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
