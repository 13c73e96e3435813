#!/usr/bin/env python
"""Host against device timing of generate.py's volume smoothing (modules/inference.py::smooth_volume).

    python scripts/bench_postprocess.py [--shapes 128x512x512 512x512x512] [--reps 3] [--skip_host]

For every shape one seeded int16 volume goes through
  * the host path (scipy, as ``--postprocess_device cpu``), timed once with time.perf_counter;
  * the device path end to end: upload, kernels, download of the int16 result
    (``smooth_volume(v, device=...)``), best of --reps after a warm-up on a small volume;
  * the device kernels alone, volume resident, from HIP events, best of --reps after a warm-up at
    the full shape; --stages adds one event pair per stage (second of two runs).
The two results are compared with np.array_equal.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "ducosy-gan_amd"))

from modules.hip import volume as V  # noqa: E402
from modules.inference import SMOOTH_KW, smooth_volume, smooth_volume_device  # noqa: E402


def seeded_volume(shape, seed=0):
    """Stored values of a CT-like volume: soft tissue noise, a bone block above the threshold."""
    rng = np.random.default_rng(seed)
    v = rng.normal(40, 300, shape).astype(np.float32)
    d, h, w = shape
    v[:, h // 4:h // 3, w // 4:w // 2] += 900
    return np.round(v).astype(np.int16)


def _events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def stage_times(vol):
    """Event time of every stage of the device path, in ms (the chunked unsharp stage summed)."""
    t = {}
    t["gauss_z_0.8"], g = _events(lambda: V.gaussian_filter1d(vol, 0.8, 0))
    t["gauss_z_0.7"], sm = _events(lambda: V.gaussian_filter1d(g, SMOOTH_KW["sigma_z"], 0))
    # sigma_xy 0.05 has radius 0: the device path skips those two passes (postprocess_gpu.py)
    t["minmax"], mm = _events(lambda: V.minmax(g))
    r = SMOOTH_KW["sharpen_radius"]
    n = max(1, min(vol.shape[0], (64 << 20) // (vol.shape[1] * vol.shape[2] * 8)))
    s, o = sm[:n], g[:n]
    scale = vol.shape[0] / n
    ty, y = _events(lambda: V.gaussian_filter1d(s, r, 1, out_dtype=torch.float64))
    tx, bs = _events(lambda: V.gaussian_filter1d(y, r, 2))
    t["blur_y_f32_f64"], t["blur_x_f64"] = 2 * ty * scale, 2 * tx * scale   # two blurs per chunk
    bo = V.gaussian_filter1d(V.gaussian_filter1d(o, r, 1, out_dtype=torch.float64), r, 2)
    out = torch.empty(s.shape, dtype=torch.int16, device=vol.device)
    tf, _ = _events(lambda: V.unsharp_finish(s, bs, bo, o, mm, SMOOTH_KW["sharpen_amount"], 750, out))
    t["unsharp_finish"] = tf * scale
    return {k: round(x, 3) for k, x in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["128x512x512", "512x512x512"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--skip_host", action="store_true", help="device times only (no comparison)")
    ap.add_argument("--stages", action="store_true", help="add per-stage event times")
    a = ap.parse_args()
    dev = torch.device(a.device)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    smooth_volume(seeded_volume((8, 64, 64)), device=dev)  # library load, allocator, first launches
    res = {"metric": "smooth_volume_seconds", "device": torch.cuda.get_device_name(dev), "shapes": {}}
    for spec in a.shapes:
        shape = tuple(int(x) for x in spec.split("x"))
        v = seeded_volume(shape)
        r = {}
        e2e, got = [], None
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = smooth_volume(v, device=dev)
            e2e.append(time.perf_counter() - t0)
        r["device_end_to_end_s"] = round(min(e2e), 4)
        vol = torch.from_numpy(v.astype(np.float32)).to(dev)
        smooth_volume_device(vol)
        torch.cuda.synchronize()
        r["device_kernels_ms"] = round(min(_events(lambda: smooth_volume_device(vol))[0] for _ in range(a.reps)), 3)
        if a.stages:
            stage_times(vol)  # warm-up of every stage at this shape
            r["stage_ms"] = stage_times(vol)
        del vol
        if not a.skip_host:
            t0 = time.perf_counter()
            want = smooth_volume(v)
            r["host_s"] = round(time.perf_counter() - t0, 3)
            r["identical"] = bool(np.array_equal(got, want))
            r["speedup_end_to_end"] = round(r["host_s"] / r["device_end_to_end_s"], 1)
            r["speedup_kernels"] = round(r["host_s"] * 1e3 / r["device_kernels_ms"], 1)
        res["shapes"][spec] = r
    print(json.dumps(res))
    if not a.skip_host and not all(r["identical"] for r in res["shapes"].values()):
        sys.exit(1)


if __name__ == "__main__":
    main()
