"""The training-set builder of the normal-map U-Net on the GPU: the kernel (csrc/nmodel_data.hip,
modules/hip/nmodel_data.py) against the host function modules/nmodel/prepare.py, the entry point
prepare_nmodel_data.py with the resident pipeline behind it, and the way from a built data directory
through train_nmodel.py to inference.

Bars.  vue and diff: bit for bit (the same float32 operations, one rounding each).  Counts: equal.
Sums: 1e-10 relative, the bar of tests/test_gpu_regions.py for the same reduction scheme (two orders
of N <= 1e5 float64 terms differ by at most N * 2^-53 of the sum of their magnitudes; the volumes
are drawn so that no sum cancels below a hundredth of that)."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from modules.hip import lib
from modules.hip import nmodel_data as ND
from modules.inference import translate_volume_device
from modules.model import Generator
from modules.nmodel import UNet3DLight, load_model, predict_volume
from modules.nmodel import prepare as P
from test_cpu_nmodel_data import F, cect_for, load_builder, manifest, pair_volume, run, stand_in_merged, write_patients

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SOFT, LUNG = (-150, 250), (-1000, -150)
RTOL = 1e-10
# (3,7,9): 63 voxels per slice, the scalar instance, one chunk; (2,70,300): 21000 voxels per slice, above
# DCS_MET_PAIR_CHUNK, so three partial records are folded; (1,64,64): one slice, the vector instance;
# (5,64,64): the phantom with slopes 1 and 0.5 and a uint16 CECT
assert lib.MET_PAIR_CHUNK == 8192 and lib.NMODEL_NSTATS == P.NSTATS == 11
SHAPES = [(3, 7, 9), (2, 70, 300), (1, 64, 64), (5, 64, 64)]


@functools.lru_cache(maxsize=None)
def volume(shape):
    """(pair, merged, host result without merged, host result with merged), computed once."""
    D, H, W = shape
    if shape == (5, 64, 64):
        pair = pair_volume(7, 5, 64, cect_unsigned=True)
    else:
        rng = np.random.default_rng([D, H, W])
        # HU -1024 .. 476, and -1000.3 .. 49 at slope 0.7: products, sums and quotients that round
        raw = rng.integers(0, 1500, shape).astype(np.int16)
        sn = np.where(np.arange(D) % 2, 1.0, 0.7).astype(F)
        in_ = np.where(np.arange(D) % 2, -1024.0, -1000.3).astype(F)
        pair = (raw, sn, in_) + cect_for(raw, sn, in_, D + H + W, cect_unsigned=shape != (1, 64, 64))
    merged = stand_in_merged(*pair[:3])
    plain, against = P.residual_targets(*pair), P.residual_targets(*pair, merged=merged)
    for a in pair + (merged,) + plain + against:
        a.setflags(write=False)
    for st in (plain[2], against[2]):       # no branch is vacuous
        assert st[:, P.N_APPLY].sum() > 0 and st[:, P.N_NEG].sum() > 0 and st[:, P.N_OVER].sum() > 0
    return pair, merged, plain, against


def up(a):
    return torch.from_numpy(np.array(a).view(np.int16)).to(DEV)


def device_targets(pair, merged):
    ncct, sn, in_, cect, sc, ic = pair
    m = None if merged is None else torch.from_numpy(np.array(merged)).to(DEV)
    keep = None if m is None else m.clone()
    run_ = lambda: ND.residual_targets(up(ncct), sn, in_, up(cect), sc, ic, m, 8.0, ncct_unsigned=ncct.dtype == np.uint16,
                                       cect_unsigned=cect.dtype == np.uint16)
    first, second = run_(), run_()
    assert all(torch.equal(a, b) for a, b in zip(first, second))          # bit-identical from run to run
    assert m is None or torch.equal(m, keep)                              # merged is only read
    assert first[0].is_cuda and first[2].dtype == torch.float64
    return tuple(t.cpu().numpy() for t in first)


@pytest.mark.parametrize("with_merged", [False, True], ids=["ncct", "merged"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_against_the_host_function(shape, with_merged):
    pair, merged, plain, against = volume(shape)
    want = against if with_merged else plain
    got = device_targets(pair, merged if with_merged else None)
    assert got[0].dtype == got[1].dtype == F and got[2].shape == (shape[0], 11)
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    assert np.array_equal(got[2][:, :4], want[2][:, :4])
    err = np.abs(got[2][:, 4:] - want[2][:, 4:])
    print(f"{shape} merged={with_merged}: worst relative error of the sums "
          f"{(err / np.maximum(np.abs(want[2][:, 4:]), 1e-300)).max():.3e}")
    assert np.all(err <= RTOL * np.abs(want[2][:, 4:]))


def test_a_uint16_tensor_sets_its_own_flag():
    pair, _, plain, _ = volume((5, 64, 64))
    ncct, sn, in_, cect, sc, ic = pair
    got = ND.residual_targets(up(ncct), sn, in_, up(cect).view(torch.uint16), sc, ic)
    assert np.array_equal(got[1].cpu().numpy(), plain[1])


def test_bad_arguments_raise_before_any_launch():
    pair, merged, _, _ = volume((3, 7, 9))
    ncct, sn, in_, cect, sc, ic = pair
    with pytest.raises(RuntimeError, match="device tensor required"):
        ND.residual_targets(torch.from_numpy(np.array(ncct)), sn, in_, up(cect), sc, ic)
    with pytest.raises(RuntimeError, match="device tensor required"):
        ND.residual_targets(up(ncct), sn, in_, up(cect), sc, ic, torch.from_numpy(np.array(merged)))
    with pytest.raises(RuntimeError):
        ND.residual_targets(up(ncct).float(), sn, in_, up(cect), sc, ic)
    with pytest.raises(ValueError):
        ND.residual_targets(up(ncct), sn, in_, up(cect)[:2], sc[:2], ic[:2])
    with pytest.raises(ValueError):
        ND.residual_targets(up(ncct), sn[:2], in_, up(cect), sc, ic)
    with pytest.raises(ValueError):
        ND.residual_targets(up(ncct), sn, in_, up(cect), sc, ic, torch.zeros(3, 7, 8, device=DEV))
    # the C entry point refuses an output that aliases an input and a short workspace
    v = torch.empty(3, 7, 9, device=DEV)
    st, ws = torch.empty(3, 11, dtype=torch.float64, device=DEV), torch.empty(3 * 11, dtype=torch.float64, device=DEV)
    f = lambda a: torch.from_numpy(np.array(a, F)).to(DEV)
    p = lambda t: None if t is None else t.data_ptr()
    held = [up(ncct), f(sn), f(in_), up(cect), f(sc), f(ic)]
    call = lambda m, d, nbytes: lib.call("dcs_nmodel_targets", p(held[0]), 0, p(held[1]), p(held[2]), p(held[3]), 1,
                                         p(held[4]), p(held[5]), p(m), 3, 7, 9, 8.0, p(v), p(d), p(st), p(ws), nbytes, None)
    with pytest.raises(lib.HipLibraryError, match="aliases"):
        call(v, torch.empty_like(v), ws.numel() * 8)
    with pytest.raises(lib.HipLibraryError, match="alias"):
        call(None, v, ws.numel() * 8)
    with pytest.raises(lib.HipLibraryError, match="workspace too small"):
        call(None, torch.empty_like(v), ws.numel() * 8 - 8)
    assert lib.query("dcs_nmodel_targets_workspace_size", 3, 7, 9) == ws.numel() * 8
    assert lib.query("dcs_nmodel_targets_workspace_size", 2, 70, 300) == 2 * 3 * 11 * 8
    assert lib.query("dcs_nmodel_targets_workspace_size", 0, 7, 9) == 0


# ---------------------------------------------------------------------------------------
# the entry point
# ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """DS: two patients of 5 slices at 64x64; DS3: three; the two Generator checkpoints; the base command line."""
    root = tmp_path_factory.mktemp("nmodel_data_gpu")
    pairs = write_patients(str(root / "in" / "DS"), ["A", "B"])
    write_patients(str(root / "in" / "DS3"), ["A", "B", "C"])
    torch.manual_seed(0)
    models = Generator(3, 1).to(DEV).eval(), Generator(2, 1).to(DEV).eval()
    base = ["--img_size", "64", "--slice_batch", "2"]
    for name, g in zip(("soft", "lung"), models):
        torch.save(g.state_dict(), str(root / f"{name}.pth"))
        base += [f"--model_path_{name}", str(root / f"{name}.pth")]
    return root, pairs, models, base


@pytest.mark.parametrize("mode", ["range", "enhancement"])
def test_entry_point_against_the_scect(tree, tmp_path, mode):
    root, pairs, models, base = tree
    builder, data = load_builder(), tmp_path / "data"
    run(builder, root, data, base + ["--synthesis", mode])
    man = manifest(data)
    assert sorted(man) == ["DS_A", "DS_B"]
    for name in ("A", "B"):
        ncct, sn, in_ = pairs[name][:3]
        merged = translate_volume_device(*models, ncct, [float(v) for v in sn], [float(v) for v in in_], SOFT, LUNG, 64, 2,
                                         DEV, synthesis=mode).cpu().numpy()
        assert (merged != ncct).any()
        want = P.residual_targets(*pairs[name], merged=merged)
        diff, vue = np.load(data / "diff_map" / f"DS_{name}_diff.npy"), np.load(data / "vue_files" / f"DS_{name}_vue.npy")
        assert np.array_equal(diff.view(np.uint32), want[1].view(np.uint32))
        assert np.array_equal(vue.view(np.uint32), want[0].view(np.uint32))
        r = man[f"DS_{name}"]
        assert (r["status"], r["against"], r["synthesis"]) == ("written", "scect", mode)
        assert [int(r[k]) for k in ("n_apply", "n_neg", "n_over")] == [int(want[2][:, k].sum()) for k in (1, 2, 3)]


def test_entry_point_against_the_ncct_writes_the_same_bytes_on_both_devices(tree, tmp_path):
    root, pairs, _, _ = tree
    builder = load_builder()
    run(builder, root, tmp_path / "gpu", ["--against", "ncct", "--device", "cuda"])
    run(builder, root, tmp_path / "cpu", ["--against", "ncct", "--device", "cpu"])
    for name in ("A", "B"):
        for sub, end in (("vue_files", "vue"), ("diff_map", "diff")):
            a, b = (tmp_path / d / sub / f"DS_{name}_{end}.npy" for d in ("gpu", "cpu"))
            assert a.read_bytes() == b.read_bytes()
    g, c = manifest(tmp_path / "gpu"), manifest(tmp_path / "cpu")
    for pid in g:
        assert [g[pid][k] for k in ("status", "n", "n_apply", "n_neg", "n_over")] == \
               [c[pid][k] for k in ("status", "n", "n_apply", "n_neg", "n_over")]
        assert abs(float(g[pid]["corr"]) - float(c[pid]["corr"])) <= 1e-9


def _load_train_nmodel():
    spec = importlib.util.spec_from_file_location("dcs_train_nmodel_data", os.path.join(ROOT, "ducosy-gan_amd", "train_nmodel.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_a_built_data_directory_trains(tree, tmp_path):
    """Closing the loop: builder -> train_nmodel.py (one epoch) -> checkpoint -> predict_volume."""
    root, _, _, _ = tree
    data = tmp_path / "data"
    run(load_builder(), root, data, ["--against", "ncct", "--device", "cuda", "--dataset_names", "DS3"])
    assert sorted(os.listdir(data / "diff_map")) == [f"DS3_{n}_diff.npy" for n in "ABC"]
    tn = _load_train_nmodel()
    hist = tn.main(["--model_type", "light", "--base_channels", "8", "--data_dir", str(data), "--output_dir",
                    str(tmp_path / "out"), "--patch_size", "1", "32", "32", "--patches_per_volume", "2", "--num_workers", "0",
                    "--gradient_accumulation_steps", "2", "--num_epochs", "1", "--save_interval", "1"])
    assert len(hist["train"]) == 1 and all(np.isfinite(hist["train"] + hist["val"]))
    model, cfg = load_model(str(tmp_path / "out" / "checkpoints" / "latest.pth"), DEV)
    assert type(model) is UNet3DLight and cfg.base_channels == 8
    vue = np.load(data / "vue_files" / "DS3_A_vue.npy")
    pred = predict_volume(model, vue, DEV)
    assert pred.shape == vue.shape and np.isfinite(pred).all()
