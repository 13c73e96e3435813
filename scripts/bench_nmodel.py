#!/usr/bin/env python
"""The difference-map U-Net over one HU volume: the HIP path against the mirror module's ATen forward.

    python scripts/bench_nmodel.py [--slices 128] [--size 512] [--reps 3] [--chunk N] [--models light16 full32]

One seeded [slices, size, size] HU volume already on the device goes through
  * hip: ``predict_volume_device`` (modules/nmodel, csrc/unet.hip, the rows pass), in the operand mode
    of modules/hip/ops.py;
  * aten_f32: the mirror nn.Module's own forward on the same GPU in float32, on [chunk,1,1,H,W]
    batches with the normalisation and denormalisation as torch ops (the reference feeds one slice
    at a time; whole chunks are the kinder baseline);
  * aten_autocast: the same under torch.autocast('cuda'), the way the reference runs it.
The ATen legs are the baseline, never the code under test.  All legs run in this process,
alternating, after one warm-up each; wall clock around a device synchronise, best of --reps.  A
per-kernel table of the HIP path (HIP events around every launch of one more run, summed per
label) follows, so a slow layer shape shows.  Prints the commit and one JSON line per model.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "ducosy-gan_amd"))

from modules.hip import ops  # noqa: E402
from modules.hip import unet as U  # noqa: E402
from modules.nmodel import UNet3D, UNet3DLight, predict_volume_device  # noqa: E402

MODELS = {"light16": (UNet3DLight, 16), "full32": (UNet3D, 32)}


def commit():
    """The checked-out commit; DUCOSY_COMMIT names it where the tree travels without its history."""
    try:
        out = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, timeout=10)
        if out.returncode == 0 and out.stdout.strip():
            dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain"], capture_output=True, text=True, timeout=30)
            return out.stdout.strip() + ("+dirty" if dirty.stdout.strip() else "")
    except (OSError, subprocess.SubprocessError):
        pass
    return os.environ.get("DUCOSY_COMMIT", "unknown")


def seeded(cls, base, dev):
    """Random weights with non-trivial BatchNorm statistics and scales of both signs."""
    torch.manual_seed(0)
    model = cls(base_channels=base).eval()
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm3d):
            m.running_mean.normal_(0, 0.3)
            m.running_var.uniform_(0.5, 1.5)
            m.weight.data.uniform_(0.5, 1.5).mul_(torch.where(torch.rand(m.weight.shape) < 0.3, -1.0, 1.0))
            m.bias.data.uniform_(-0.3, 0.3)
        elif isinstance(m, torch.nn.Conv3d) and m.kernel_size == (3, 3, 3):
            m.weight.data.normal_(0, (2.0 / (9 * m.in_channels)) ** 0.5)
    return model.to(dev)


@torch.no_grad()
def aten(model, hu, chunk, autocast):
    out = torch.empty_like(hu)
    for z in range(0, hu.shape[0], chunk):
        x = ((hu[z:z + chunk].clamp(-1024, 3071) + 1024) / 4095 * 2 - 1)[:, None, None]
        with torch.autocast("cuda", enabled=autocast):
            y = model(x)
        out[z:z + chunk] = (y[:, 0, 0].float() + 1) / 2 * 4000
    return out


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def kernel_table(model, hu, chunk):
    """ms per label over one more HIP run, HIP events around every launch."""
    U.TIMES = []
    try:
        predict_volume_device(model, hu, chunk=chunk)
        torch.cuda.synchronize()
        rows = {}
        for label, a, b in U.TIMES:
            n, ms = rows.get(label, (0, 0.0))
            rows[label] = (n + 1, ms + a.elapsed_time(b))
    finally:
        U.TIMES = None
    return {k: {"launches": n, "ms": round(ms, 3)} for k, (n, ms) in rows.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slices", type=int, default=128)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=None, help="slices per call of every leg (default: the HIP path's own)")
    ap.add_argument("--models", nargs="+", default=list(MODELS), choices=list(MODELS))
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_nmodel.py needs a GPU")
    dev = torch.device(a.device)
    print("commit:", commit())
    g = torch.Generator(device="cpu").manual_seed(1)
    hu = (torch.rand(a.slices, a.size, a.size, generator=g) * 2600 - 1100).to(dev)
    for tag in a.models:
        cls, base = MODELS[tag]
        model = seeded(cls, base, dev)
        chunk = a.chunk or U.default_chunk(U.plan_for(model, dev), a.slices, a.size, a.size)
        legs = {"hip": lambda: predict_volume_device(model, hu, chunk=chunk),
                "aten_f32": lambda: aten(model, hu, chunk, False),
                "aten_autocast": lambda: aten(model, hu, chunk, True)}
        times = {k: [] for k in legs}
        outs = {}
        for rep in range(a.reps + 1):            # rep 0 is the warm-up of every leg at the full shape
            for name, fn in legs.items():
                t, out = _wall(fn)
                if rep:
                    times[name].append(t)
                if rep == a.reps:
                    outs[name] = out
        res = {"metric": "nmodel_volume_seconds", "commit": commit(), "device": torch.cuda.get_device_name(dev),
               "model": f"{cls.__name__} base {base}", "shape": f"{a.slices}x{a.size}x{a.size}", "chunk": chunk,
               "mma": ops.get_mma()}
        for name in legs:
            res[f"{name}_s"] = round(min(times[name]), 4)
            res[f"{name}_all_s"] = [round(t, 4) for t in times[name]]
        res["aten_f32_over_hip"] = round(res["aten_f32_s"] / res["hip_s"], 3)
        scale = float(outs["aten_f32"].abs().max())
        for name in ("hip", "aten_autocast"):
            res[f"{name}_max_diff_vs_aten_f32_over_max"] = float((outs[name] - outs["aten_f32"]).abs().max()) / scale
        outs.clear()
        res["hip_kernels"] = kernel_table(model, hu, chunk)
        print(json.dumps(res))


if __name__ == "__main__":
    main()
