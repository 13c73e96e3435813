"""The enhancement-difference synthesis ("sCECT v3", the reference's synthesis_test,
generate.py:302-477) on the host: modules/inference.py::synthesize_enhancement against hand-computed
voxels and an independent per-voxel restatement in np.float32 scalars, synthesize_volume's
enhancement mode, generate.py::synthesis_test on a working directory, and the new flags.  pydicom is
not installed here, so parity with files written by the reference's own script is unpinned."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT
from modules import dicom
from modules.inference import smooth_volume, synthesize_enhancement, synthesize_volume

SHAPES = [(3, 5, 7), (2, 8, 16), (3, 24, 20)]
PAIRS = [(1.0, -1024.0), (0.5, 0.0), (0.7, -1000.0)]
DTYPES = [np.int16, np.uint16]
# a = 1, b = -1024: (raw, soft, lung) -> merged
BOUNDARY = [((624, 674, 624), 624.0),      # HU -400 exactly: not valid (strict)
            ((625, 675, 625), 675.0),      # HU -399: valid
            ((1000, 1005, 1000), 1000.0),  # a gain of exactly 5 is not applied (strict)
            ((1000, 1006, 1000), 1006.0),  # 6 is
            ((1000, 1010, 1020), 1030.0),  # both models: (r + ds) + dl
            ((1000, 990, 1003), 1000.0),   # neither
            ((1000, 1000, 1007), 1007.0)]  # lung alone


def draw_series(shape, dtype, seed=0):
    """(raw, soft, lung, slopes, intercepts): stored values that fit ``dtype``, the translations raw
    plus an integer in [-20, 60], slice k with PAIRS[k % 3], the BOUNDARY voxels at the head of slice 0."""
    rng = np.random.default_rng(seed)
    info = np.iinfo(dtype)
    lo = 0 if dtype == np.uint16 else -1024
    raw = rng.integers(lo, 3001, size=shape)
    soft = np.clip(raw + rng.integers(-20, 61, size=shape), info.min, info.max)
    lung = np.clip(raw + rng.integers(-20, 61, size=shape), info.min, info.max)
    for k, ((r, s, g), _) in enumerate(BOUNDARY):
        raw.reshape(shape[0], -1)[0, k], soft.reshape(shape[0], -1)[0, k], lung.reshape(shape[0], -1)[0, k] = r, s, g
    pairs = [PAIRS[k % len(PAIRS)] for k in range(shape[0])]
    return (raw.astype(dtype), soft.astype(dtype), lung.astype(dtype), [a for a, _ in pairs], [b for _, b in pairs])


def per_voxel(raw, soft, lung, slope, intercept, thr=5.0, min_hu=-400.0, soft_pair=None, lung_pair=None):
    """The rule restated voxel by voxel with np.float32 scalars (one rounding per operation)."""
    f = np.float32
    a, b, thr, min_hu = f(slope), f(intercept), f(thr), f(min_hu)
    sa, sb = (a, b) if soft_pair is None else (f(soft_pair[0]), f(soft_pair[1]))
    la, lb = (a, b) if lung_pair is None else (f(lung_pair[0]), f(lung_pair[1]))
    out = np.empty(raw.shape, f)
    for idx in np.ndindex(raw.shape):
        r = f(raw[idx])
        hr = f(f(r * a) + b)
        es = f(f(f(f(soft[idx]) * sa) + sb) - hr)
        el = f(f(f(f(lung[idx]) * la) + lb) - hr)
        m = r
        if es > thr and hr > min_hu:
            m = f(m + f(es / a))
        if el > thr and hr > min_hu:
            m = f(m + f(el / a))
        out[idx] = m
    return out


def load_generate(name="dcs_gen_enh"):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "ducosy-gan_amd", "generate.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


@pytest.mark.parametrize("dtype", DTYPES)
def test_hand_computed_voxels(dtype):
    raw, soft, lung = (np.array([v[0][k] for v in BOUNDARY], dtype)[None] for k in range(3))
    got = synthesize_enhancement(raw, soft, lung, 1, -1024)
    assert got.dtype == np.float32 and got.tolist() == [[v[1] for v in BOUNDARY]]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_matches_the_per_voxel_restatement(shape, dtype):
    raw, soft, lung, slopes, inters = draw_series(shape, dtype)
    keep = [x.copy() for x in (raw, soft, lung)]
    seen = set()
    for k in range(shape[0]):
        got = synthesize_enhancement(raw[k], soft[k], lung[k], slopes[k], inters[k])
        want = per_voxel(raw[k], soft[k], lung[k], slopes[k], inters[k])
        assert got.dtype == np.float32 and got.shape == raw[k].shape
        assert np.array_equal(got, want)
        hr = raw[k].astype(np.float32) * np.float32(slopes[k]) + np.float32(inters[k])
        for s, g in zip((soft[k].astype(np.float32) * np.float32(slopes[k]) + np.float32(inters[k]) - hr > 5).ravel(),
                        (lung[k].astype(np.float32) * np.float32(slopes[k]) + np.float32(inters[k]) - hr > 5).ravel()):
            seen.add((bool(s), bool(g)))
    assert len(seen) == 4                                   # all four branch combinations occur
    for x, k in zip((raw, soft, lung), keep):
        assert np.array_equal(x, k)                         # inputs untouched
    # other settings, and the translated series' own rescale pairs
    got = synthesize_enhancement(raw[0], soft[0], lung[0], 1, -1024, 12.5, -300, (1.0, -1020.0), (0.99, -1024))
    want = per_voxel(raw[0], soft[0], lung[0], 1, -1024, 12.5, -300, (1.0, -1020.0), (0.99, -1024))
    assert np.array_equal(got, want)
    assert not np.array_equal(got, synthesize_enhancement(raw[0], soft[0], lung[0], 1, -1024, 12.5, -300))


def test_volume_mode_on_the_host_stacks_the_slices():
    raw, soft, lung, slopes, inters = draw_series((3, 5, 7), np.int16, seed=1)
    got = synthesize_volume(raw, slopes, inters, soft, lung, (-150, 250), (-1000, -150), mode="enhancement")
    want = np.stack([synthesize_enhancement(raw[k], soft[k], lung[k], slopes[k], inters[k]) for k in range(3)])
    assert got.dtype == np.float32 and np.array_equal(got, want)
    other = synthesize_volume(raw, slopes, inters, soft, lung, (-150, 250), (-1000, -150), mode="enhancement",
                              threshold=20, min_hu=0)
    want = np.stack([synthesize_enhancement(raw[k], soft[k], lung[k], slopes[k], inters[k], 20, 0) for k in range(3)])
    assert np.array_equal(other, want) and not np.array_equal(other, got)
    with pytest.raises(ValueError):
        synthesize_volume(raw, slopes, inters, soft, lung, (-150, 250), (-1000, -150), mode="v3")


def write_working(root, raw, soft, lung, slopes, inters, soft_inter_shift=0.0):
    """A working directory as generate() leaves it: raw / soft_tissue / lung under root/DS/P0."""
    for kind, vol, shift in (("raw", raw, 0.0), ("soft_tissue", soft, soft_inter_shift), ("lung", lung, 0.0)):
        folder = os.path.join(root, "DS", "P0", kind)
        os.makedirs(folder)
        for k in range(len(vol)):
            ds = dicom.new_ct_slice(vol[k], float(slopes[k]), float(inters[k]) + shift, instance=k + 1,
                                    uid_suffix=f"{kind}.{k}")
            ds.save_as(os.path.join(folder, f"IM{k:03d}.dcm"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_synthesis_test_on_the_host(tmp_path, dtype):
    gen = load_generate()
    raw, soft, lung, slopes, inters = draw_series((4, 16, 12), dtype, seed=2)
    write_working(str(tmp_path / "w"), raw, soft, lung, slopes, inters)
    args = gen.get_args(["--dataset_names", "DS", "--working_dir_root", str(tmp_path / "w"),
                         "--output_dir_root", str(tmp_path / "o"), "--synthesis", "enhancement"])
    gen.synthesis_test(args)
    merged = synthesize_volume(raw, slopes, inters, soft, lung, (-150, 250), (-1000, -150), mode="enhancement")
    assert (merged != raw).any() and (merged == raw).any()
    want = smooth_volume(merged)
    out = tmp_path / "o" / "DS" / "P0"
    assert sorted(os.listdir(out)) == [f"{k:04d}.dcm" for k in range(4)]
    for k in range(4):
        o = dicom.dcmread(str(out / f"{k:04d}.dcm"))
        px = o.pixel_array
        assert np.array_equal(px.view(np.int16), want[k])
        assert o.SeriesDescription == "DuCoSyGAN sCECT v3"
        assert (float(o.WindowWidth), float(o.WindowCenter)) == (1250.0, -375.0)
        assert int(o.SmallestImagePixelValue) == int(want[k].min())
        assert int(o.LargestImagePixelValue) == int(want[k].max())
    # synthesis() on the same directory still writes the v2 series
    gen.synthesis(gen.get_args(["--dataset_names", "DS", "--working_dir_root", str(tmp_path / "w"),
                                "--output_dir_root", str(tmp_path / "o2")]))
    assert dicom.dcmread(str(tmp_path / "o2" / "DS" / "P0" / "0000.dcm")).SeriesDescription == "DuCoSyGAN sCECT v2"


def test_get_args():
    gen = load_generate()
    a = gen.get_args([])
    assert a.synthesis == "range" and a.enhancement_threshold == 5.0 and a.enhancement_min_hu == -400.0
    b = gen.get_args(["--synthesis", "enhancement", "--enhancement_threshold", "7.5", "--enhancement_min_hu", "-250"])
    assert (b.synthesis, b.enhancement_threshold, b.enhancement_min_hu) == ("enhancement", 7.5, -250.0)
    with pytest.raises(SystemExit):
        gen.get_args(["--synthesis", "v3"])
