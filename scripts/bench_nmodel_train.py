#!/usr/bin/env python
"""One optimizer step of the normal-map U-Net: the HIP step against the mirror module's ATen step.

    python scripts/bench_nmodel_train.py [--size 512] [--accum 8] [--reps 5] [--models light16 full32]

One optimizer step is the reference's recipe (modules/nmodel/config.py): --accum micro-batches of
one size x size slice, L1 loss, the global-norm clip at 1.0, Adam at lr 5e-5.  Legs, on the same
module weights and the same seeded slices already on the device:
  * hip: modules/hip/unet_train.py (TrainState.accumulate x accum, then step) in the operand mode
    of modules/hip/ops.py;
  * hip_f16: the same in the 'f16' operand mode (what use_mixed_precision selects);
  * aten_f32: the mirror nn.Module in training mode, loss.backward(), clip_grad_norm_, Adam;
  * aten_autocast: the same under torch.autocast('cuda') with a GradScaler.
The ATen legs are the baseline, never the code under test.  All legs run in this process,
alternating, after one warm-up step each; every step is timed with HIP events on the stream and
the median of --reps is reported.  A per-kernel table of the hip leg (HIP events around every
launch of one more step, summed per label) follows.  Prints the commit and one JSON line per model.
"""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "ducosy-gan_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_nmodel import MODELS, commit, seeded  # noqa: E402
from modules.hip import ops  # noqa: E402
from modules.hip import unet as U  # noqa: E402
from modules.hip.unet_train import TrainState  # noqa: E402

LR, CLIP = 5e-5, 1.0


class HipLeg:
    def __init__(self, model, mode):
        self.state, self.mode = TrainState(copy.deepcopy(model).train()), mode

    def step(self, batches):
        before = ops.get_mma()
        ops.set_mma(self.mode)
        try:
            for x, t in batches:
                self.state.accumulate(x, t, 1.0 / len(batches))
            self.state.step(LR, CLIP)
        finally:
            ops.set_mma(before)


class AtenLeg:
    def __init__(self, model, autocast):
        self.model, self.autocast = copy.deepcopy(model).train(), autocast
        self.opt = torch.optim.Adam(self.model.parameters(), lr=LR)
        self.scaler = torch.amp.GradScaler("cuda", enabled=autocast)

    def step(self, batches):
        for x, t in batches:
            with torch.autocast("cuda", enabled=self.autocast):
                loss = (self.model(x) - t).abs().mean() / len(batches)
            self.scaler.scale(loss).backward()
        self.scaler.unscale_(self.opt)
        torch.nn.utils.clip_grad_norm_(self.model.parameters(), CLIP)
        self.scaler.step(self.opt)
        self.scaler.update()
        self.opt.zero_grad(set_to_none=True)


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def kernel_table(leg, batches):
    U.TIMES = []
    try:
        leg.step(batches)
        torch.cuda.synchronize()
        rows = {}
        for label, a, b in U.TIMES:
            n, ms = rows.get(label, (0, 0.0))
            rows[label] = (n + 1, ms + a.elapsed_time(b))
    finally:
        U.TIMES = None
    top = sorted(rows.items(), key=lambda kv: -kv[1][1])
    return {k: {"launches": n, "ms": round(ms, 3)} for k, (n, ms) in top}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--accum", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--models", nargs="+", default=list(MODELS), choices=list(MODELS))
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_nmodel_train.py needs a GPU")
    dev = torch.device(a.device)
    torch.cuda.set_device(dev)
    print("commit:", commit())
    g = torch.Generator(device="cpu").manual_seed(1)
    batches = [((torch.rand(1, 1, 1, a.size, a.size, generator=g) * 2 - 1).to(dev),
                (torch.rand(1, 1, 1, a.size, a.size, generator=g) * 2 - 1).to(dev)) for _ in range(a.accum)]
    for tag in a.models:
        cls, base = MODELS[tag]
        model = seeded(cls, base, dev)
        legs = {"hip": HipLeg(model, ops.get_mma()), "hip_f16": HipLeg(model, "f16"),
                "aten_f32": AtenLeg(model, False), "aten_autocast": AtenLeg(model, True)}
        times = {k: [] for k in legs}
        for rep in range(a.reps + 1):            # rep 0 is the warm-up of every leg at the full shape
            for name, leg in legs.items():
                ms = _timed(lambda: leg.step(batches))
                if rep:
                    times[name].append(ms)
        res = {"metric": "nmodel_train_step_ms", "commit": commit(), "device": torch.cuda.get_device_name(dev),
               "model": f"{cls.__name__} base {base}", "step": f"{a.accum} x 1x{a.size}x{a.size}", "mma": ops.get_mma()}
        for name in legs:
            res[f"{name}_ms"] = round(statistics.median(times[name]), 3)
            res[f"{name}_all_ms"] = [round(t, 3) for t in times[name]]
        res["aten_f32_over_hip"] = round(res["aten_f32_ms"] / res["hip_ms"], 3)
        res["aten_autocast_over_hip"] = round(res["aten_autocast_ms"] / res["hip_ms"], 3)
        res["aten_autocast_over_hip_f16"] = round(res["aten_autocast_ms"] / res["hip_f16_ms"], 3)
        table = kernel_table(legs["hip"], batches)
        res["hip_kernels_ms_total"] = round(sum(v["ms"] for v in table.values()), 3)
        res["hip_kernels"] = table
        print(json.dumps(res))
        del legs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
