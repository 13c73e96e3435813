#!/usr/bin/env python
"""Staged against resident timing of generate.py's per-patient work, in memory (no files).

    python scripts/bench_generate.py [--slices 128] [--size 512] [--img_size 512] [--slice_batch 16] [--reps 3]

One seeded phantom patient (modules/phantom, int16 stored values with per-slice rescale) and two
seeded Generators (cin 3 and cin 2, 9 residual blocks) go through
  * staged: what generate() + synthesis(--postprocess_device cuda) compute between the decoded
    NCCT slices and the int16 volume, without the DICOM files in between: hu_from_stored and
    normalise_hu on the host, per-slice ``_conditioning``, ``translate_slices``,
    ``stored_from_output``, ``synthesize_volume(device, keep_on_device=True)``,
    ``smooth_volume(device)``;
  * resident: ``translate_volume_device`` -> ``smooth_volume_device`` -> one download.
Both legs run in this process, alternating, after one warm-up each; wall clock around a device
synchronise, best of --reps.  The three kernels of csrc/slices.hip are also timed alone with HIP
events (20 calls per window, best of --reps after a warm-up) and reported with the bytes their
algorithm moves over that time; ``generators_only_s`` is the two Generators' forward over the same
chunks with inputs already on the device, the part both legs share.  The int16 results are compared with np.array_equal when --size equals --img_size (the
staged path's ATen resizes differ from the resize kernel in the last bits otherwise, which a
truncating cast can turn into off-by-one stored values).  Prints ``identical: true/false`` and one
JSON line.  --apply_diffmap adds a third leg, the resident path with the difference-map stage
(a seeded UNet3DLight base 16, or --nmodel full32 for UNet3D base 32; modules/nmodel), and reports it
as ``resident_diffmap_s`` next to ``resident_s``.  --synthesis enhancement runs every leg with the
enhancement-difference merge (sCECT v3) in place of the HU-range merge and adds ``translate_enhance``
to the kernel table, beside ``translate_merge``.
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

from modules import phantom  # noqa: E402
from modules.hip import slices as S  # noqa: E402
from modules.inference import (_conditioning, hu_from_stored, normalise_hu, smooth_volume,  # noqa: E402
                               smooth_volume_device, stored_from_output, synthesize_volume, translate_slices,
                               translate_volume_device)
from modules.model import Generator  # noqa: E402

SOFT, LUNG = (-150, 250), (-1000, -150)


def staged(models, raw, slopes, inters, img_size, batch, dev, mode="range"):
    hu = [hu_from_stored(r, a, b) for r, a, b in zip(raw, slopes, inters)]
    stored = []
    for kind, model, (lo, hi) in (("soft_tissue", models[0], SOFT), ("lung", models[1], LUNG)):
        ys = translate_slices(model, [normalise_hu(h, lo, hi) for h in hu], img_size, batch, dev,
                              _conditioning(model, kind, hu, dev))
        stored.append(np.stack([stored_from_output(y, lo, hi, a, b, raw.dtype)
                                for y, a, b in zip(ys, slopes, inters)]))
    on_dev = synthesize_volume(raw, slopes, inters, stored[0], stored[1], SOFT, LUNG, device=dev, keep_on_device=True,
                               mode=mode)
    return smooth_volume(on_dev, device=dev)


def resident(models, raw, slopes, inters, img_size, batch, dev, nmodel=None, mode="range"):
    merged = translate_volume_device(models[0], models[1], raw, slopes, inters, SOFT, LUNG, img_size, batch, dev,
                                     nmodel=nmodel, synthesis=mode)
    return smooth_volume_device(merged).cpu().numpy()


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def _event_ms(fn, reps, iters=20):
    """ms per call: ``iters`` back-to-back calls between two events, best of ``reps`` after a warm-up."""
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) / iters)
    return best


@torch.no_grad()
def generators_only(models, D, img_size, batch, dev):
    """Wall time of the two Generators alone over the series' chunks, inputs already on the device."""
    g = torch.Generator(device="cpu").manual_seed(2)
    x = (torch.rand(batch, 1, img_size, img_size, generator=g) * 2 - 1).to(dev)
    masks = [(torch.rand(batch, m.input_channels - 1, img_size, img_size, generator=g) < 0.3).float().to(dev)
             for m in models]

    def run():
        for model, m in zip(models, masks):
            for i in range(0, D, batch):
                n = min(batch, D - i)
                model(x[:n], m[:n])
    return _wall(run)[0]


def kernel_times(raw, slopes, inters, dev, reps, mode="range"):
    """Event time and achieved GB/s (algorithmic bytes: inputs read once, outputs written once) of the
    slices.hip kernels at the benchmark's series shape; mode "enhancement" adds translate_enhance."""
    D, H, W = raw.shape
    n = D * H * W
    res = {}
    g = torch.Generator(device="cpu").manual_seed(1)
    ys = (torch.rand(D, H, W, generator=g) * 2 - 1).to(dev)
    yl = (torch.rand(D, H, W, generator=g) * 2 - 1).to(dev)
    bits = torch.from_numpy(raw).to(dev)
    a, b = torch.from_numpy(slopes).to(dev), torch.from_numpy(inters).to(dev)
    ms = _event_ms(lambda: S.translate_merge(bits, a, b, ys, yl, SOFT, LUNG), reps)
    res["translate_merge_f32_only"] = {"ms": round(ms, 4), "GBps": round(14 * n / ms / 1e6, 1)}
    ms = _event_ms(lambda: S.translate_merge(bits, a, b, ys, yl, SOFT, LUNG, want_soft=True, want_lung=True,
                                             want_merged=True), reps)
    res["translate_merge_all_outputs"] = {"ms": round(ms, 4), "GBps": round(20 * n / ms / 1e6, 1)}
    if mode == "enhancement":
        ms = _event_ms(lambda: S.translate_enhance(bits, a, b, ys, yl, SOFT, LUNG), reps)
        res["translate_enhance_f32_only"] = {"ms": round(ms, 4), "GBps": round(14 * n / ms / 1e6, 1)}
        ms = _event_ms(lambda: S.translate_enhance(bits, a, b, ys, yl, SOFT, LUNG, want_stored=True), reps)
        res["translate_enhance_with_stored"] = {"ms": round(ms, 4), "GBps": round(18 * n / ms / 1e6, 1)}
    x = ys[:, None]
    hh, hw = max(1, H // 2), max(1, W // 2)
    small = S.resize_aa(x, (hh, hw))
    for name, fn, src, dst in (("resize_aa_down2", S.resize_aa, x, (hh, hw)), ("resize_aa_up2", S.resize_aa, small, (H, W)),
                               ("resize_nearest_down2", S.resize_nearest, x, (hh, hw)),
                               ("resize_nearest_up2", S.resize_nearest, small, (H, W))):
        ms = _event_ms(lambda: fn(src, dst), reps)
        moved = 4 * (src.numel() + D * dst[0] * dst[1])
        res[name] = {"ms": round(ms, 4), "GBps": round(moved / ms / 1e6, 1),
                     "shape": f"{D}x{src.shape[2]}x{src.shape[3]}->{dst[0]}x{dst[1]}"}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slices", type=int, default=128)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--img_size", type=int, default=None, help="network size (default: --size)")
    ap.add_argument("--slice_batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--apply_diffmap", action="store_true", help="also time the resident path with the difference-map stage")
    ap.add_argument("--nmodel", choices=["light16", "full32"], default="light16")
    ap.add_argument("--synthesis", choices=["range", "enhancement"], default="range",
                    help="the merge both legs run: the HU-range merge or the enhancement-difference merge")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_generate.py needs a GPU")
    dev = torch.device(a.device)
    img_size = a.img_size or a.size
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    raw, slopes, inters = phantom.ct_batch(0, a.slices, a.size)
    torch.manual_seed(0)
    models = (Generator(3, 9).to(dev).eval(), Generator(2, 9).to(dev).eval())
    legs = {"staged": lambda *args: staged(*args, mode=a.synthesis),
            "resident": lambda *args: resident(*args, mode=a.synthesis)}
    if a.apply_diffmap:
        from modules.nmodel import UNet3D, UNet3DLight
        nmodel = (UNet3DLight(base_channels=16) if a.nmodel == "light16" else UNet3D(base_channels=32)).to(dev).eval()
        legs["resident_diffmap"] = lambda *args: resident(*args, nmodel=nmodel, mode=a.synthesis)
    times = {k: [] for k in legs}
    outs = {}
    for rep in range(a.reps + 1):            # rep 0 is the warm-up of both legs at the full shape
        for name, fn in legs.items():
            t, out = _wall(lambda: fn(models, raw, slopes, inters, img_size, a.slice_batch, dev))
            if rep:
                times[name].append(t)
            outs[name] = out
    res = {"metric": "generate_patient_seconds", "device": torch.cuda.get_device_name(dev),
           "shape": f"{a.slices}x{a.size}x{a.size}", "img_size": img_size, "slice_batch": a.slice_batch,
           "synthesis": a.synthesis,
           "staged_s": round(min(times["staged"]), 4), "resident_s": round(min(times["resident"]), 4),
           "staged_all_s": [round(t, 4) for t in times["staged"]],
           "resident_all_s": [round(t, 4) for t in times["resident"]]}
    res["resident_median_s"] = round(float(np.median(times["resident"])), 4)
    res["staged_over_resident"] = round(res["staged_s"] / res["resident_s"], 3)
    if a.apply_diffmap:
        res["nmodel"] = a.nmodel
        res["resident_diffmap_s"] = round(min(times["resident_diffmap"]), 4)
        res["resident_diffmap_all_s"] = [round(t, 4) for t in times["resident_diffmap"]]
        res["diffmap_stage_s"] = round(res["resident_diffmap_s"] - res["resident_s"], 4)
    same = bool(np.array_equal(outs["staged"], outs["resident"]))
    res["identical"] = same
    if not same:
        d = np.abs(outs["staged"].astype(np.int64) - outs["resident"].astype(np.int64))
        res["differing_share"], res["largest_difference"] = float((d != 0).mean()), int(d.max())
    res["generators_only_s"] = round(min(generators_only(models, a.slices, img_size, a.slice_batch, dev)
                                         for _ in range(a.reps)), 4)
    res["kernels"] = kernel_times(raw, slopes, inters, dev, a.reps, a.synthesis)
    print("identical:", "true" if same else "false")
    print(json.dumps(res))
    if img_size == a.size and not same:
        sys.exit(1)


if __name__ == "__main__":
    main()
