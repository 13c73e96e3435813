#!/usr/bin/env python
"""Timing of the heart-mask clean-up, the organ mask and the apply pass on one patient.

    python scripts/bench_masking.py [--shape 128x512x512] [--reps 5] [--host_reps 1] [--skip_host]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/bench_masking.py --trace_run

One synthetic patient: a label volume [z, y, x] holding a heart ellipsoid (label 51) with an
outflow stalk that rises in +z across a two-voxel gap, 33 more organ blobs of the other target
labels, hollow so that every one has holes to fill, each over its own range of slices, and three
int16 series.

  * host against device for the three stages: modules/organ_masks.py (numpy / scipy.ndimage, wall
    clock, --host_reps runs) against modules/hip/organ_masks.py on resident tensors (HIP events
    around one call after a warm-up, median / min / max of --reps).  The device results are compared
    with the host's and the run fails when they differ in one byte.
  * a patient end to end on the device, wall clock around a synchronise: upload of the labels and
    the three series, heart clean-up, organ mask, apply, download of the three masked series and
    the modified labels.
  * --trace_run does one warm-up and one pass of the three device stages and exits: the process to
    put under a kernel trace for the per-kernel times.

Prints progress lines and, last, one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PKG = os.path.join(ROOT, "ducosy-gan_amd")
sys.path.insert(0, PKG)

from modules import organ_masks as OM  # noqa: E402
from modules.hip import organ_masks as G  # noqa: E402


def patient(shape, seed=0):
    """(labels uint8 [z, y, x], three int16 series)"""
    d, h, w = shape
    lab = np.zeros(shape, dtype=np.uint8)

    def ellipsoid(c, r, label, hollow):
        lo = [max(0, int(ci - ri)) for ci, ri in zip(c, r)]
        hi = [min(n, int(ci + ri) + 2) for ci, ri, n in zip(c, r, shape)]
        z, y, x = np.ogrid[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        q = ((z - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((x - c[2]) / r[2]) ** 2
        box = lab[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        box[(q <= 1.0) & (q >= hollow)] = label

    others = [v for v in OM.MASK_TARGET_LABELS if v != OM.HEART_LABEL]
    cols = 6
    for i, label in enumerate(others):                       # hollow ellipsoids on a 6 x 6 grid of the slice
        cy, cx = (i // cols + 0.5) * h / cols, (i % cols + 0.5) * w / cols
        cz = (0.15 + 0.7 * ((i * 7) % len(others)) / len(others)) * d
        ellipsoid((cz, cy, cx), (0.18 * d, 0.07 * h, 0.07 * w), label, 0.35)
    hz, hy, hx = 0.4 * d, 0.5 * h, 0.5 * w
    ellipsoid((hz, hy, hx), (0.23 * d, 0.1 * h, 0.12 * w), OM.HEART_LABEL, 0.0)
    top = int(hz + 0.23 * d)
    s = max(2, w // 64)
    lab[top - 2:, int(hy) - s:int(hy) + s, int(hx) - s:int(hx) + s] = OM.HEART_LABEL       # the stalk ...
    lab[top + 4:top + 6, int(hy) - s:int(hy) + s, int(hx) - s:int(hx) + s] = 0             # ... and its gap
    rng = np.random.default_rng(seed)
    series = [rng.integers(-1024, 3000, shape, dtype=np.int16) for _ in range(3)]
    return lab, series


def _events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def _spread(times, digits=3):
    return {"median": round(statistics.median(times), digits), "min": round(min(times), digits),
            "max": round(max(times), digits)}


def _wall(fn, reps):
    times, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return times, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="128x512x512")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host_reps", type=int, default=1)
    ap.add_argument("--skip_host", action="store_true")
    ap.add_argument("--trace_run", action="store_true")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_masking.py needs a GPU")
    dev = torch.device(a.device)
    shape = tuple(int(v) for v in a.shape.split("x"))
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    t0 = time.perf_counter()
    lab, series = patient(shape)
    print(f"phantom patient {shape} in {time.perf_counter() - t0:.1f} s: heart {int((lab == 51).sum())} voxels, "
          f"{len(np.unique(lab)) - 1} labels", flush=True)
    res = {"metric": "masking_patient", "device": torch.cuda.get_device_name(dev), "shape": a.shape}
    with torch.cuda.device(dev):
        dlab = torch.from_numpy(lab).to(dev)
        dser = [torch.from_numpy(s).to(dev) for s in series]
        stages = {"heart": lambda: G.modify_heart_label(dlab), "organ_mask": lambda: G.organ_mask(dlab)}
        outs = {k: fn() for k, fn in stages.items()}            # warm-up, and the results to compare
        stages["apply"] = lambda: G.apply_organ_mask(*dser, outs["organ_mask"])
        outs["apply"] = stages["apply"]()
        torch.cuda.synchronize()
        if a.trace_run:
            for fn in stages.values():
                fn()
            torch.cuda.synchronize()
            print(json.dumps({"metric": "masking_trace_run", "shape": a.shape}))
            return
        dev_ms = {k: _spread([_events(fn)[0] for _ in range(a.reps)]) for k, fn in stages.items()}
        res["device_ms"] = dev_ms
        res["workspace_MB"] = {
            "heart": round(G.heart_workspace_size(shape) / 2 ** 20, 1),
            "organ_mask": round(G.organ_mask_workspace_size(shape, len(OM.MASK_TARGET_LABELS),
                                                            G.default_chunk(shape, len(OM.MASK_TARGET_LABELS))) / 2 ** 20, 1)}
        print("device:", json.dumps(dev_ms), flush=True)

        def end_to_end():
            l, s = torch.from_numpy(lab).to(dev), [torch.from_numpy(v).to(dev) for v in series]
            heart = G.modify_heart_label(l)
            masked = G.apply_organ_mask(*s, G.organ_mask(heart))
            got = [heart.cpu()] + [m.cpu() for m in masked]
            torch.cuda.synchronize()
            return got
        end_to_end()
        res["patient_end_to_end_ms"] = _spread(_wall(end_to_end, a.reps)[0])
        print("end to end:", json.dumps(res["patient_end_to_end_ms"]), flush=True)
        if not a.skip_host:
            host = {}
            t, want_heart = _wall(lambda: OM.modify_heart_label(lab.T), a.host_reps)
            host["heart"] = _spread(t)
            print("host heart:", host["heart"], flush=True)
            t, want_mask = _wall(lambda: OM.organ_mask(lab), a.host_reps)
            host["organ_mask"] = _spread(t)
            print("host organ mask:", host["organ_mask"], flush=True)
            t, want_apply = _wall(lambda: [OM.apply_organ_mask(s, want_mask) for s in series], a.host_reps)
            host["apply"] = _spread(t)
            res["host_ms"] = host
            res["host_over_device"] = {k: round(host[k]["median"] / dev_ms[k]["median"], 1) for k in host}
            agree = {"heart": bool(np.array_equal(outs["heart"].cpu().numpy().T, want_heart)),
                     "organ_mask": bool(np.array_equal(outs["organ_mask"].cpu().numpy(), want_mask)),
                     "apply": all(np.array_equal(o.cpu().numpy(), w) for o, w in zip(outs["apply"], want_apply))}
            res["heart_voxels"] = {"before": int((lab == 51).sum()), "after": int((want_heart == 51).sum())}
            res["mask_share"] = round(float(want_mask.mean()), 4)
            res["agreement"] = agree
    print(json.dumps(res))
    if not a.skip_host and not all(res["agreement"].values()):
        sys.exit(1)


if __name__ == "__main__":
    main()
