"""The training-set builder of the normal-map U-Net on the host: modules/nmodel/prepare.py
(residual_targets, pearson_from_sums) against a voxel-by-voxel restatement in float32 scalars and
hand-computed voxels, and prepare_nmodel_data.py::build_dataset on a DICOM tree: files, manifest,
the skips, --overwrite, --min_corr, a stand-in ``translate``, and that CTDiffDataset loads the result.

The fixture's CECT is the phantom plus 60 HU in the soft-tissue voxels, N(0, 6) noise and three
voxels per slice 4500 HU above the NCCT, so n_apply, n_neg and n_over are all positive."""
import csv
import functools
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT
from modules import dicom, phantom
from modules.inference import hu_from_stored
from modules.nmodel import prepare as P
from modules.nmodel.dataset import CTDiffDataset, get_dataloaders

F = np.float32


def cect_for(raw, sn, in_, seed, cect_unsigned=True):
    """(cect, sc, ic) of an NCCT series: its HU plus 60 where it lies in (0, 200), N(0, 6) noise and
    three voxels per slice at +4500 HU; uint16 with the pair (1, -1024), or int16 with slopes 1 / 0.5
    and intercept -1000."""
    n, size = raw.shape[0], raw.shape[1] * raw.shape[2]
    hu = raw.astype(np.float64) * sn[:, None, None] + in_[:, None, None]
    rng = np.random.default_rng([seed, 1234])
    c_hu = hu + np.where((hu > 0) & (hu < 200), 60.0, 0.0) + rng.normal(0, 6, hu.shape)
    for z in range(n):
        idx = rng.choice(size, 3, replace=False)
        c_hu.reshape(n, -1)[z, idx] = hu.reshape(n, -1)[z, idx] + 4500.0
    if cect_unsigned:
        sc, ic, dt = np.ones(n, F), np.full(n, -1024.0, F), np.uint16
    else:
        sc, ic, dt = np.where(np.arange(n) % 2, 0.5, 1.0).astype(F), np.full(n, -1000.0, F), np.int16
    info = np.iinfo(dt)
    cect = np.clip(np.round((c_hu - ic[:, None, None]) / sc[:, None, None]), info.min, info.max).astype(dt)
    return cect, sc, ic


def pair_volume(seed, n=5, size=64, cect_unsigned=True, kinds=None):
    """(ncct int16, sn, in, cect, sc, ic): phantom.ct_batch (slopes 1 and 0.5 in one volume) and its CECT."""
    raw, sn, in_ = phantom.ct_batch(seed, n, size, kinds)
    return (raw, sn, in_) + cect_for(raw, sn, in_, seed, cect_unsigned)


def stand_in_merged(raw, sn, in_):
    """A stand-in for the merged sCECT: the NCCT stored values plus 30.25 where the HU is in (0, 200)."""
    hu = raw.astype(F) * np.asarray(sn, F)[:, None, None] + np.asarray(in_, F)[:, None, None]
    return raw.astype(F) + np.where((hu > 0) & (hu < 200), F(30.25), F(0))


@functools.lru_cache(maxsize=None)
def case(seed, n, size, cect_unsigned, with_merged):
    """One volume pair and the host result, computed once and shared (read-only)."""
    pair = pair_volume(seed, n, size, cect_unsigned)
    merged = stand_in_merged(*pair[:3]) if with_merged else None
    out = P.residual_targets(*pair, merged=merged)
    for a in pair + out + ((merged,) if with_merged else ()):
        a.setflags(write=False)
    return pair, merged, out


def restated(pair, merged, threshold=8.0):
    """residual_targets voxel by voxel in numpy float32 scalars; sums by np.sum of float64 values."""
    ncct, sn, in_, cect, sc, ic = pair
    D, H, W = ncct.shape
    vue, diff = np.zeros((D, H, W), F), np.zeros((D, H, W), F)
    for z in range(D):
        a, b, c, d = F(sn[z]), F(in_[z]), F(sc[z]), F(ic[z])
        nz, cz = ncct[z].ravel(), cect[z].ravel()
        mz = None if merged is None else merged[z].ravel()
        vz, dz = vue[z].reshape(-1), diff[z].reshape(-1)
        for i in range(H * W):
            x = F(nz[i]) * a + b
            y = F(cz[i]) * c + d
            g = x if mz is None else F(mz[i]) * a + b
            vz[i], dz[i] = x, (y - g) / a
            assert type(x) is F and type(dz[i]) is F
    stats = np.zeros((D, 11))
    for z in range(D):
        dz = diff[z].ravel()
        x64 = vue[z].ravel().astype(np.float64)
        y64 = (cect[z].ravel().astype(F) * F(sc[z]) + F(ic[z])).astype(np.float64)
        stats[z] = [dz.size, int((dz >= F(threshold)).sum()), int((dz < 0).sum()), int((dz > 4000).sum()),
                    np.sum(np.clip(dz, 0, 4000).astype(np.float64)), np.sum(np.abs(dz).astype(np.float64)),
                    np.sum(x64), np.sum(y64), np.sum(x64 * x64), np.sum(y64 * y64), np.sum(x64 * y64)]
    return vue, diff, stats


def check_against(got, want, rtol):
    """vue and diff bit for bit, counts equal, float64 sums within rtol of the reference value."""
    assert got[0].dtype == got[1].dtype == F and got[2].dtype == np.float64
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    assert got[2].shape == want[2].shape == (want[0].shape[0], 11)
    assert np.array_equal(got[2][:, :4], want[2][:, :4])
    err = np.abs(got[2][:, 4:] - want[2][:, 4:])
    rel = err / np.maximum(np.abs(want[2][:, 4:]), 1e-300)
    print("max relative error of the sums", rel.max())
    assert np.all(err <= rtol * np.abs(want[2][:, 4:]))


@pytest.mark.parametrize("cect_unsigned,with_merged", [(True, False), (True, True), (False, True)])
def test_residual_targets_against_the_scalar_restatement(cect_unsigned, with_merged):
    pair, merged, got = case(7, 5, 64, cect_unsigned, with_merged)
    assert set(pair[1].tolist()) == {1.0, 0.5} and pair[3].dtype == (np.uint16 if cect_unsigned else np.int16)
    tot = got[2].sum(0)
    assert tot[P.N_APPLY] > 0 and tot[P.N_NEG] > 0 and tot[P.N_OVER] > 0, tot[:4]   # no branch is vacuous
    check_against(got, restated(pair, merged), 1e-12)
    if with_merged:
        assert not np.array_equal(got[1], case(7, 5, 64, cect_unsigned, False)[2][1])
        assert np.array_equal(got[0], case(7, 5, 64, cect_unsigned, False)[2][0])


def test_hand_computed_voxels():
    ncct = np.array([[[100, 200, -50, 300]]], np.int16)            # slope 0.5, intercept -1000
    cect = np.array([[[1100, 5200, 0, 100]]], np.uint16)           # slope 1, intercept -1024
    vue, diff, st = P.residual_targets(ncct, [0.5], [-1000], cect, [1], [-1024])
    assert vue.tolist() == [[[-950.0, -900.0, -1025.0, -850.0]]]
    assert diff.tolist() == [[[2052.0, 10152.0, 2.0, -148.0]]]     # (y - x) / 0.5, y = 76, 4176, -1024, -924
    assert st[0, :6].tolist() == [4, 2, 1, 1, 2052.0 + 4000.0 + 2.0, 2052.0 + 10152.0 + 2.0 + 148.0]
    x, y = np.array([-950.0, -900.0, -1025.0, -850.0]), np.array([76.0, 4176.0, -1024.0, -924.0])
    assert st[0, 6:].tolist() == [x.sum(), y.sum(), (x * x).sum(), (y * y).sum(), (x * y).sum()]
    merged = np.array([[[150.5, 200, -50, 300]]], F)               # g = -924.75, then x
    vue2, diff2, st2 = P.residual_targets(ncct, [0.5], [-1000], cect, [1], [-1024], merged, threshold=2001.5)
    assert np.array_equal(vue2, vue) and diff2.tolist() == [[[2001.5, 10152.0, 2.0, -148.0]]]
    assert st2[0, :6].tolist() == [4, 2, 1, 1, 6003.5, 12303.5]    # the threshold is met with equality
    assert merged.tolist() == [[[150.5, 200, -50, 300]]]


def test_bad_arguments_raise():
    pair, _, _ = case(7, 5, 64, True, False)
    ncct, sn, in_, cect, sc, ic = pair
    with pytest.raises(ValueError):
        P.residual_targets(ncct, sn, in_, cect[:4], sc[:4], ic[:4])
    with pytest.raises(ValueError):
        P.residual_targets(ncct, sn, in_, cect[:, :32], sc, ic)
    with pytest.raises(ValueError):
        P.residual_targets(ncct, sn, in_, cect, sc, ic, merged=np.zeros((5, 64, 32), F))
    with pytest.raises(ValueError):
        P.residual_targets(ncct, sn[:2], in_, cect, sc, ic)
    with pytest.raises(TypeError):
        P.residual_targets(ncct.astype(F), sn, in_, cect, sc, ic)


def test_pearson_from_sums_against_corrcoef():
    """1e-9 absolute.  The sums are float64 and the formula is the textbook one, whose cancellation
    costs mean^2 / variance ulps: about 1e5 x 1e-16 on the all-air slice (mean -1024, sigma 3),
    the worst of these."""
    pair, _, (vue, _, st) = case(7, 5, 64, True, False)
    y = pair[3].astype(F) * pair[4][:, None, None] + pair[5][:, None, None]
    got = P.pearson_from_sums(st)
    want = np.array([np.corrcoef(vue[z].ravel().astype(np.float64), y[z].ravel().astype(np.float64))[0, 1]
                     for z in range(5)])
    print("per-slice |error|", np.abs(got - want))
    assert got.shape == (5,) and np.all(np.abs(got - want) <= 1e-9)
    vol = P.pearson_from_sums(st.sum(0))
    assert abs(float(vol) - np.corrcoef(vue.ravel().astype(np.float64), y.ravel().astype(np.float64))[0, 1]) <= 1e-9
    assert P.volume_summary(st)["corr"] == float(vol)
    # a constant slice has no correlation
    ncct = pair[0].copy()
    ncct[2] = 17
    st2 = P.residual_targets(ncct, *pair[1:])[2]
    r = P.pearson_from_sums(st2)
    assert np.isnan(r[2]) and np.all(np.isfinite(np.delete(r, 2)))
    const = np.full((1, 8, 8), 3, np.int16)
    assert np.isnan(P.pearson_from_sums(P.residual_targets(const, [0.3], [0.1], const, [0.7], [-0.3])[2])[0])


# ---------------------------------------------------------------------------------------
# the entry point
# ---------------------------------------------------------------------------------------
def load_builder():
    spec = importlib.util.spec_from_file_location("dcs_prepare_nmodel_data",
                                                  os.path.join(ROOT, "ducosy-gan_amd", "prepare_nmodel_data.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def write_series(folder, stored, slopes, inters, tag, keep=None):
    """One series as DICOM files whose file order is the reverse of their InstanceNumber order."""
    os.makedirs(folder, exist_ok=True)
    D = len(stored)
    for s in range(D):
        z = D - 1 - s                                  # file s holds slice z; instance z + 1
        if keep is not None and z not in keep:
            continue
        ds = dicom.new_ct_slice(stored[z], float(slopes[z]), float(inters[z]), instance=z + 1, uid_suffix=f"{tag}.{z}")
        ds.save_as(os.path.join(folder, f"IM{s:03d}.dcm"))


def write_patients(root, names, size=64, slices=5):
    """Good patients under ``root`` (a dataset directory); {name: pair}."""
    pairs = {}
    for k, name in enumerate(names):
        pair = pair_volume(20 + k, slices, size, cect_unsigned=bool(k % 2))
        write_series(os.path.join(root, name, "POST VUE"), pair[0], pair[1], pair[2], f"{k}.0")
        write_series(os.path.join(root, name, "POST STD"), pair[3], pair[4], pair[5], f"{k}.1")
        pairs[name] = pair
    return pairs


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """DS: three good patients (A, B, C), one whose CECT lacks a slice, one with one smaller CECT slice,
    one whose CECT has a slice of the other stored dtype, one without a CECT folder, and one whose CECT series is another anatomy's (air and one-lung slices
    against a chest)."""
    root = tmp_path_factory.mktemp("nmodel_data")
    ds = str(root / "in" / "DS")
    pairs = write_patients(ds, ["A", "B", "C"])
    a = pairs["A"]
    write_series(os.path.join(ds, "X_counts", "POST VUE"), a[0], a[1], a[2], "x.0")
    write_series(os.path.join(ds, "X_counts", "POST STD"), a[3], a[4], a[5], "x.1", keep={0, 1, 2, 4})
    write_series(os.path.join(ds, "Y_sizes", "POST VUE"), a[0], a[1], a[2], "y.0")
    small = [s if z != 3 else np.ascontiguousarray(s[:32, :32]) for z, s in enumerate(a[3])]
    write_series(os.path.join(ds, "Y_sizes", "POST STD"), small, a[4], a[5], "y.1")
    write_series(os.path.join(ds, "V_dtypes", "POST VUE"), a[0], a[1], a[2], "v.0")
    mixed = [s if z != 1 else s.astype(np.uint16 if s.dtype == np.int16 else np.int16) for z, s in enumerate(a[3])]
    write_series(os.path.join(ds, "V_dtypes", "POST STD"), mixed, a[4], a[5], "v.1")
    write_series(os.path.join(ds, "W_missing", "POST VUE"), a[0], a[1], a[2], "w.0")
    chest = pair_volume(31, 5, 64, kinds=["chest"])
    other = pair_volume(32, 5, 64, kinds=["air", "one_lung"])
    write_series(os.path.join(ds, "Z_foreign", "POST VUE"), chest[0], chest[1], chest[2], "z.0")
    write_series(os.path.join(ds, "Z_foreign", "POST STD"), other[3], other[4], other[5], "z.1")
    pairs["Z_foreign"] = chest[:3] + other[3:]
    return root, pairs


def run(builder, root, data_dir, extra=(), translate=None):
    args = builder.get_args(["--input_dir_root", str(root / "in"), "--dataset_names", "DS", "--data_dir", str(data_dir)]
                            + list(extra))
    return builder.build_dataset(args, translate=translate)


def manifest(data_dir):
    with open(os.path.join(data_dir, "manifest.csv"), newline="") as f:
        return {r["id"]: r for r in csv.DictReader(f)}


def test_builder_against_ncct_on_the_host(tree, tmp_path):
    root, pairs = tree
    builder, data = load_builder(), tmp_path / "data"
    rows = run(builder, root, data, ["--against", "ncct", "--device", "cpu"])
    man = manifest(data)
    assert [r["id"] for r in rows] == sorted(man) == ["DS_" + n for n in ("A", "B", "C", "V_dtypes", "W_missing", "X_counts", "Y_sizes", "Z_foreign")]
    assert list(next(iter(man.values()))) == list(builder.MANIFEST_COLUMNS)
    for name in ("A", "B", "C", "Z_foreign"):
        pid = f"DS_{name}"
        vue, diff = np.load(data / "vue_files" / f"{pid}_vue.npy"), np.load(data / "diff_map" / f"{pid}_diff.npy")
        want = P.residual_targets(*pairs[name])
        assert vue.dtype == diff.dtype == F and vue.shape == (5, 64, 64)
        assert np.array_equal(vue.view(np.uint32), want[0].view(np.uint32))
        assert np.array_equal(diff.view(np.uint32), want[1].view(np.uint32))
        r, tot = man[pid], P.volume_summary(want[2])
        assert r["status"] == "written" and (r["D"], r["H"], r["W"]) == ("5", "64", "64")
        assert (r["against"], r["synthesis"]) == ("ncct", "")
        assert [int(r[k]) for k in ("n", "n_apply", "n_neg", "n_over")] == [tot[k] for k in ("n", "n_apply", "n_neg", "n_over")]
        assert min(tot["n_apply"], tot["n_neg"], tot["n_over"]) > 0
        assert float(r["mean_clipped"]) == tot["mean_clipped"] and float(r["share_apply"]) == tot["share_apply"]
        assert float(r["corr"]) == tot["corr"]
        with open(data / "stats" / f"{pid}_slices.csv", newline="") as f:
            sl = list(csv.DictReader(f))
        assert len(sl) == 5 and list(sl[0]) == list(builder.SLICE_COLUMNS)
        assert np.array_equal(np.array([[float(s[k]) for k in P.STAT_NAMES] for s in sl]), want[2])
        corr = P.pearson_from_sums(want[2])
        assert [s["corr"] for s in sl] == ["" if np.isnan(c) else repr(float(c)) for c in corr]
        # the file is what CTDiffDataset.normalize_hu expects: the NCCT in HU
        hu = np.stack([hu_from_stored(pairs[name][0][z], pairs[name][1][z], pairs[name][2][z]) for z in range(5)])
        assert np.array_equal(CTDiffDataset.normalize_hu(vue), CTDiffDataset.normalize_hu(hu))
    assert man["DS_X_counts"]["status"] == "skipped: slice counts differ: 5 NCCT, 4 CECT"
    assert man["DS_Y_sizes"]["status"] == "skipped: slices differ in shape: 32x32, 64x64"
    assert man["DS_W_missing"]["status"] == "skipped: CECT series missing or empty"
    assert man["DS_V_dtypes"]["status"] == "skipped: CECT series mixes stored dtypes: int16, uint16"
    assert sorted(os.listdir(data / "diff_map")) == [f"DS_{n}_diff.npy" for n in ("A", "B", "C", "Z_foreign")]
    # the true pairs correlate (see test_min_corr_skips_a_foreign_series), the foreign one does not
    assert all(float(man[f"DS_{n}"]["corr"]) > 0.95 for n in "ABC") and float(man["DS_Z_foreign"]["corr"]) < 0.9

    # the training side loads it
    sizes = {}
    for mode in ("train", "val"):
        ds = CTDiffDataset(str(data), mode, patch_size=(1, 32, 32), patches_per_volume=2)
        item = ds[0]
        assert item["input"].shape == item["target"].shape == (1, 1, 32, 32)
        assert float(item["input"].abs().max()) <= 1 and float(item["target"].abs().max()) <= 1
        sizes[mode] = len(ds.patient_ids)
    assert sizes == {"train": 3, "val": 1}
    tl, vl = get_dataloaders(str(data), batch_size=1, num_workers=0, patch_size=(1, 32, 32), patches_per_volume=2)
    assert next(iter(tl))["input"].shape == (1, 1, 1, 32, 32) and len(vl) == 2

    # a second run leaves the files alone, and says so; --overwrite rewrites them
    vue_a = data / "vue_files" / "DS_A_vue.npy"
    original = vue_a.read_bytes()
    np.save(vue_a, np.zeros(3, F))
    marker = vue_a.read_bytes()
    rows = run(builder, root, data, ["--against", "ncct", "--device", "cpu"])
    assert vue_a.read_bytes() == marker
    man = manifest(data)
    assert all(man[f"DS_{n}"]["status"].startswith("kept: files exist") for n in ("A", "B", "C", "Z_foreign"))
    assert man["DS_X_counts"]["status"].startswith("skipped: slice counts differ")
    run(builder, root, data, ["--against", "ncct", "--device", "cpu", "--overwrite"])
    assert vue_a.read_bytes() == original and manifest(data)["DS_A"]["status"] == "written"


def test_min_corr_skips_a_foreign_series(tree, tmp_path):
    """The gate 0.9 lies between the two kinds of pair.  A true pair differs by 60 HU of enhancement,
    sigma 6 noise and three voxels per slice at +4500 HU, which add 3 x 4500^2 / 4096 = 1.5e4 to a
    variance of about 2.5e5 (air at -1024 against tissue around 0): a correlation near 0.97.  Air and
    one-lung slices against chest slices share the air around the body and little else: far below 0.9."""
    root, _ = tree
    builder, data = load_builder(), tmp_path / "data"
    run(builder, root, data, ["--against", "ncct", "--device", "cpu", "--min_corr", "0.9"])
    man = manifest(data)
    assert [man[f"DS_{n}"]["status"] for n in "ABC"] == ["written"] * 3
    st = man["DS_Z_foreign"]["status"]
    assert st.startswith("skipped: correlation ") and st.endswith("below --min_corr 0.9")
    assert float(man["DS_Z_foreign"]["corr"]) < 0.9 and man["DS_Z_foreign"]["n"] != ""
    assert not os.path.exists(data / "diff_map" / "DS_Z_foreign_diff.npy")
    assert not os.path.exists(data / "vue_files" / "DS_Z_foreign_vue.npy")


def test_builder_with_a_stand_in_translate(tree, tmp_path):
    root, pairs = tree
    builder, data = load_builder(), tmp_path / "data"
    seen = []

    def translate(raw, slopes, intercepts):
        seen.append(raw.shape)
        return stand_in_merged(raw, slopes, intercepts)

    run(builder, root, data, ["--against", "scect", "--device", "cpu", "--synthesis", "enhancement"], translate)
    man = manifest(data)
    assert len(seen) == 4
    for name in ("A", "B", "C"):
        want = P.residual_targets(*pairs[name], merged=stand_in_merged(*pairs[name][:3]))
        plain = P.residual_targets(*pairs[name])
        diff = np.load(data / "diff_map" / f"DS_{name}_diff.npy")
        assert np.array_equal(diff.view(np.uint32), want[1].view(np.uint32)) and not np.array_equal(diff, plain[1])
        assert np.array_equal(np.load(data / "vue_files" / f"DS_{name}_vue.npy"), want[0])
        assert (man[f"DS_{name}"]["against"], man[f"DS_{name}"]["synthesis"]) == ("scect", "enhancement")
        assert int(man[f"DS_{name}"]["n_apply"]) == int(want[2][:, P.N_APPLY].sum())


def test_against_scect_on_the_host_exits_with_the_message(tree, tmp_path):
    root, _ = tree
    builder = load_builder()
    with pytest.raises(SystemExit) as e:
        run(builder, root, tmp_path / "data", ["--against", "scect", "--device", "cpu"])
    assert "--against scect needs the GPU and both Generator checkpoints" in str(e.value)
    assert not os.path.exists(tmp_path / "data" / "manifest.csv")
