"""The normal-map U-Net mirrors (modules/nmodel) without a GPU: state_dict layout and float64
forward against the reference's own (tests/golden/nmodel_unet.npz, written by
tests/golden/make_golden_nmodel.py), the folded 2-D form the device path is built from, load_model's
checkpoint rules, the host tail, and the new flag's default."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
from modules import nmodel
from modules.nmodel import UNet3D, UNet3DLight, fold, forward_folded, load_model
from modules.postprocess import apply_diffmap

CLASSES = {"UNet3D": UNet3D, "UNet3DLight": UNet3DLight}


def load_golden_script():
    spec = importlib.util.spec_from_file_location("make_golden_nmodel",
                                                  os.path.join(GOLDEN, "make_golden_nmodel.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = load_golden_script()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "nmodel_unet.npz"))


def seeded_model(cls_name, base, seed):
    """The mirror class with the fixture's prng weights and BatchNorm statistics, eval mode."""
    model = CLASSES[cls_name](base_channels=base).eval()
    state = G.seeded_state({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    return model


@pytest.mark.parametrize("tag", sorted(G.LISTED))
def test_state_dict_layout_is_the_references(golden, tag):
    cls, base = G.LISTED[tag]
    sd = CLASSES[cls](base_channels=base).state_dict()
    assert list(sd) == [str(k) for k in golden[f"keys:{tag}"]]
    assert [",".join(str(int(s)) for s in v.shape) for v in sd.values()] == [str(s) for s in golden[f"shapes:{tag}"]]


@pytest.mark.parametrize("case", sorted(G.CASES))
def test_float64_forward_and_folded_form_equal_the_reference(golden, case):
    cls, base, seed, n, h, w = G.CASES[case]
    model = seeded_model(cls, base, seed).double()
    x = torch.from_numpy(golden[f"x:{case}"]).double()
    assert np.array_equal(golden[f"x:{case}"], G.case_input(case))
    want = golden[f"y64:{case}"]
    ref = np.abs(want).max()
    gamma = torch.cat([v for k, v in model.state_dict().items() if k.endswith(".1.weight") or k.endswith(".4.weight")])
    assert (gamma < 0).any() and (gamma > 0).any()          # the folded scale has both signs
    with torch.no_grad():
        slicewise = torch.stack([model(x[i][None, None, None])[0, 0, 0] for i in range(n)]).numpy()
        folded = forward_folded(fold(model, torch.float64), x[:, None])[:, 0].numpy()
    assert np.abs(slicewise - want).max() <= 1e-12 * ref
    assert np.abs(folded - want).max() <= 1e-12 * ref
    # the fixture's own float32 spread, the device tests' bar, is what it says
    assert float(golden[f"delta32:{case}"]) == np.abs(golden[f"y32:{case}"].astype(np.float64) - want).max() > 0


def test_folded_form_refuses_what_it_does_not_cover():
    with pytest.raises(ValueError):
        fold(UNet3DLight(trilinear=False))
    f = fold(UNet3DLight(base_channels=4).eval(), torch.float64)
    with pytest.raises(ValueError):
        forward_folded(f, torch.zeros(1, 1, 7, 16, dtype=torch.float64))   # 7 >> 3 == 0


def _checkpoint(tmp_path, name, model, config=None, drop_counters=False):
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    if drop_counters:
        sd = {k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")}
    ckpt = {"model_state_dict": sd, "epoch": 3}
    if config is not None:
        ckpt["config"] = config
    path = str(tmp_path / name)
    torch.save(ckpt, path)
    return path


def test_load_model_rules(tmp_path):
    torch.manual_seed(0)
    light, full = UNet3DLight(base_channels=8), UNet3D(base_channels=4)
    # class by down4, channels from the first convolution when there is no config
    m, cfg = load_model(_checkpoint(tmp_path, "light.pth", light), "cpu")
    assert type(m) is UNet3DLight and not m.training
    assert (cfg.base_channels, cfg.in_channels, cfg.out_channels) == (8, 1, 1)
    m, cfg = load_model(_checkpoint(tmp_path, "full.pth", full), "cpu")
    assert type(m) is UNet3D and (cfg.base_channels, cfg.in_channels, cfg.out_channels) == (4, 1, 1)
    for k, v in full.state_dict().items():
        assert torch.equal(m.state_dict()[k], v), k
    # channels from config when it is there (its defaults: 16, 1, 1)
    m, cfg = load_model(_checkpoint(tmp_path, "cfg.pth", UNet3DLight(base_channels=16), config={}), "cpu")
    assert type(m) is UNet3DLight and (cfg.base_channels, cfg.in_channels, cfg.out_channels) == (16, 1, 1)
    two = UNet3D(n_channels=2, n_classes=3, base_channels=4)
    m, cfg = load_model(_checkpoint(tmp_path, "cfg2.pth", two,
                                    config={"base_channels": 4, "in_channels": 2, "out_channels": 3}), "cpu")
    assert (cfg.base_channels, cfg.in_channels, cfg.out_channels) == (4, 2, 3)
    assert m.inc.double_conv[0].in_channels == 2 and m.outc.conv.out_channels == 3
    # BatchNorm's step counter is ignored, present or not; any other mismatch is an error
    m, _ = load_model(_checkpoint(tmp_path, "nocount.pth", light, drop_counters=True), "cpu")
    assert torch.equal(m.inc.double_conv[1].running_var, light.inc.double_conv[1].running_var)
    with pytest.raises(RuntimeError):
        load_model(_checkpoint(tmp_path, "wrong.pth", light, config={"base_channels": 16}), "cpu")
    torch.save({"weights": 1}, str(tmp_path / "bad.pth"))
    with pytest.raises(ValueError):
        load_model(str(tmp_path / "bad.pth"), "cpu")


def test_host_tail_is_apply_diffmap_of_the_denormalised_output():
    thr = 8
    # difference-map values just below / at / above the threshold, at and above 256, negative, zero
    d = np.array([7.9990234, 8.0, 8.0009766, 0.0, -3.5, 255.0, 255.99, 256.0, 257.5, 300.0, 511.9, 512.0, 3999.0,
                  4000.0, 4321.0, -4000.0], dtype=np.float32)
    y = (d / np.float32(2000) - np.float32(1)).astype(np.float32)
    vol = np.round(np.linspace(-1000, 2000, d.size)).astype(np.float32)   # whole numbers: the sum is exact
    denorm = nmodel.denormalize_diff(y)
    assert denorm.dtype == np.float32 and np.array_equal(denorm, (y + 1) / 2 * 4000)
    assert (denorm < thr).any() and (denorm >= 256).any() and (denorm < 0).any()
    got = nmodel.diffmap_tail(vol, y, thr)
    assert got.dtype == np.float32 and np.array_equal(got, apply_diffmap(vol.copy(), denorm.copy(), thr))
    kept = np.where(denorm < thr, 0, denorm)
    assert np.array_equal(got - vol, (kept.astype(np.int64) % 256).astype(np.float32))   # wraps modulo 256


def test_normalize_hu_host_form():
    hu = np.array([-5000, -1024, -1023.5, 0, 40.25, 3070.9, 3071, 9000], dtype=np.float32)
    got = nmodel.normalize_hu(hu)
    assert got.dtype == np.float32 and got[0] == got[1] == -1 and got[-1] == got[-2] == 1
    want = (np.clip(hu.astype(np.float64), -1024, 3071) + 1024) / 4095 * 2 - 1
    assert np.abs(got - want).max() < 3e-7
    assert np.array_equal(nmodel.normalize_hu(hu.astype(np.int16)), nmodel.normalize_hu(hu.astype(np.int16).astype(np.float32)))


def test_apply_diffmap_flag_defaults():
    spec = importlib.util.spec_from_file_location("dcs_gen_nmodel", os.path.join(ROOT, "ducosy-gan_amd", "generate.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    a = gen.get_args([])
    assert a.apply_diffmap is False and a.save_diff is False and a.diffmap_threshold == 8
    assert a.nmodel_path.endswith("Normal_Map_Unet.pth")
    b = gen.get_args(["--apply_diffmap", "--nmodel_path", "x.pth", "--diffmap_threshold", "12", "--save_diff"])
    assert b.apply_diffmap and b.save_diff and b.nmodel_path == "x.pth" and b.diffmap_threshold == 12
