"""Training the normal-map U-Net without a GPU (modules/nmodel config / dataset / trainer): the ATen
recipe against the reference's own float64 step (tests/golden/nmodel_train.npz, written by
tests/golden/make_golden_nmodel_train.py), the optimizer loop against torch's, the dataset's rules,
the checkpoint layout, and the configurations that must raise."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from modules import nmodel
from modules.nmodel import (Config, CTDiffDataset, FastTrainConfig, LightConfig, StandardConfig, UNet3D, UNet3DLight,
                            UNetTrainer, get_dataloaders, load_model, reference_step, split_ids)
from modules.nmodel import config as config_mod

CLASSES = {"UNet3D": UNet3D, "UNet3DLight": UNet3DLight}


def _load_maker():
    spec = importlib.util.spec_from_file_location("make_golden_nmodel_train",
                                                  os.path.join(GOLDEN, "make_golden_nmodel_train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


T = _load_maker()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "nmodel_train.npz"))


def seeded_train_model(case):
    """The mirror class of a case with the fixture's prng state (as the maker loads the reference's)."""
    cls, base, seed0 = T.CASES[case][:3]
    model = CLASSES[cls](base_channels=base)
    state = T.G.seeded_state({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed0)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    return model


def case_tensors(golden, case):
    x, t = T.case_batch(case, int(golden[f"{case}:seed"]))
    return torch.from_numpy(x)[:, None, None], torch.from_numpy(t)[:, None, None]


def golden_gradient(golden, case, name, got_flat):
    """(want, got) of one parameter: whole for a full case, the sampled entries for a sampled one."""
    want = golden[f"{case}:grad:{name}"].astype(np.float64)
    if T.CASES[case][6]:
        return want, got_flat
    return want, got_flat[T.sample_index(case, int(golden[f"{case}:seed"]), name, got_flat.size)]


def rel_l2(got, want):
    return float(np.linalg.norm(np.asarray(got, np.float64) - want) / np.linalg.norm(want))


@pytest.mark.parametrize("case", sorted(T.CASES))
def test_reference_step_float64_equals_the_reference(golden, case):
    """1e-6 relative: the fixture stores float32 gradients, so that is its storage floor."""
    print(f"case {case}: seed {int(golden[f'{case}:seed'])}, margins (|BN out|, pool gap, |o - t|) "
          f"{golden[f'{case}:margins'].tolist()}")
    assert float(golden[f"{case}:margins"].min()) >= T.MARGIN
    model = seeded_train_model(case).double()
    x, t = case_tensors(golden, case)
    loss = reference_step(model, x.double(), t.double())
    assert abs(float(loss) - float(golden[f"{case}:loss"])) <= 1e-6 * float(golden[f"{case}:loss"])
    names = [str(k) for k in golden[f"{case}:names"]]
    params = dict(model.named_parameters())
    assert names == list(params)
    for i, k in enumerate(names):
        g = params[k].grad
        if g.dim() == 5 and g.shape[2] == 3:
            assert float(g[:, :, 0].abs().max()) == 0.0 and float(g[:, :, 2].abs().max()) == 0.0, k
        flat = T.trained_view(k, g).contiguous().reshape(-1).numpy()
        assert abs(np.linalg.norm(flat) - golden[f"{case}:norms"][i]) <= 1e-6 * golden[f"{case}:norms"][i], k
        want, got = golden_gradient(golden, case, k, flat)
        assert rel_l2(got, want) <= 1e-6, (k, rel_l2(got, want))
    for k, b in model.named_buffers():
        if k.endswith("num_batches_tracked"):
            assert int(b) == 101
        else:
            want = golden[f"{case}:buf:{k}"]
            assert np.abs(b.numpy() - want).max() <= 1e-6 * np.abs(want).max(), k


def _tiny_batches(n, seed=0, hw=(16, 16), N=2):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand((N, 1, 1) + hw, generator=g, dtype=torch.float64) * 2 - 1,
             torch.rand((N, 1, 1) + hw, generator=g, dtype=torch.float64) * 2 - 1) for _ in range(n)]


def _config(tmp_path, monkeypatch, cls=FastTrainConfig, **kw):
    monkeypatch.chdir(tmp_path)
    cfg = cls(make_dirs=False)
    cfg.set_output_dir(str(tmp_path / "out"))
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_two_optimizer_steps_equal_torch_adam_and_clip(tmp_path, monkeypatch):
    """Accumulation 2, a clip that engages: UNetTrainer on the CPU against a loop written out with
    torch.optim.Adam and clip_grad_norm_."""
    cfg = _config(tmp_path, monkeypatch, gradient_accumulation_steps=2, gradient_clip_value=0.05, learning_rate=1e-3)
    torch.manual_seed(1)
    a = UNet3DLight(base_channels=8).double()
    b = UNet3DLight(base_channels=8).double()
    b.load_state_dict(a.state_dict())
    batches = _tiny_batches(4)
    trainer = UNetTrainer(a, cfg, device="cpu")
    got_losses = [float(trainer.train_step(x, t)) for x, t in batches]
    opt = torch.optim.Adam(b.parameters(), lr=1e-3)
    want_losses, norms = [], []
    b.train()
    for i, (x, t) in enumerate(batches):
        loss = torch.nn.functional.l1_loss(b(x), t) / 2
        loss.backward()
        want_losses.append(float(loss.detach()))
        if i % 2 == 1:
            norms.append(float(torch.nn.utils.clip_grad_norm_(b.parameters(), 0.05)))
            opt.step()
            opt.zero_grad()
    assert min(norms) > 0.05                                          # the clip engaged both times
    assert np.allclose(got_losses, want_losses, rtol=1e-12, atol=0)
    for (k, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.allclose(p, q, rtol=1e-12, atol=1e-15), k
    for (k, p), q in zip(a.named_buffers(), b.buffers()):
        assert torch.equal(p, q), k


# ---------------------------------------------------------------------------------------
# configuration and dataset
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset", T.PRESETS)
def test_config_fields_and_defaults_are_the_references(golden, preset, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    want = json.loads(str(golden[f"cfg:{preset}"]))
    cfg = getattr(config_mod, preset)()
    got = json.loads(json.dumps({k: v for k, v in vars(cfg).items() if k != "log_dir"}))
    assert got == want
    assert list(vars(cfg)) == list(vars(Config(make_dirs=False)))
    assert os.path.isdir(cfg.checkpoint_dir) and os.path.isdir(cfg.log_dir)      # the constructor makes them
    cfg.save(str(tmp_path / "c.json"))
    back = getattr(config_mod, preset).load(str(tmp_path / "c.json"))
    assert back.learning_rate == cfg.learning_rate and list(back.patch_size) == [1, 512, 512]


def _write_patients(root, n, shape=(4, 16, 16), seed=0):
    rng = np.random.default_rng(seed)
    os.makedirs(root / "vue_files"), os.makedirs(root / "diff_map")
    for i in range(n):
        np.save(root / "vue_files" / f"P{i}_vue.npy", rng.uniform(-1500, 3500, shape).astype(np.float32))
        np.save(root / "diff_map" / f"P{i}_diff.npy", rng.uniform(-100, 4500, shape).astype(np.float32))


def test_dataset_normalisations_are_the_inference_ones():
    hu = np.array([-5000, -1024, -1023.5, 0, 40.25, 3070.9, 3071, 9000], dtype=np.float32)
    assert np.abs(CTDiffDataset.normalize_hu(hu).astype(np.float32) - nmodel.normalize_hu(hu)).max() <= 2.0 ** -23
    y = np.linspace(-1, 1, 41, dtype=np.float32)
    assert np.abs(CTDiffDataset.denormalize_diff(y) - nmodel.denormalize_diff(y)).max() <= 4000 * 2.0 ** -23
    d = np.array([-3, 0, 8, 2000, 4000, 5000], dtype=np.float32)
    n = CTDiffDataset.normalize_diff(d)
    assert n[0] == n[1] == -1 and n[-1] == n[-2] == 1 and n[3] == 0
    assert np.allclose(CTDiffDataset.denormalize_diff(n), np.clip(d, 0, 4000))
    assert np.allclose(CTDiffDataset.denormalize_hu(CTDiffDataset.normalize_hu(hu)), np.clip(hu, -1024, 3071), atol=1e-3)


def test_dataset_patches(tmp_path):
    _write_patients(tmp_path, 4, shape=(3, 12, 10))
    ds = CTDiffDataset(str(tmp_path), mode="train", patch_size=(1, 16, 16), patches_per_volume=5)
    assert len(ds) == len(ds.patient_ids) * 5
    vol = np.arange(3 * 12 * 10, dtype=np.float32).reshape(3, 12, 10)
    # a slice index past the volume takes the last slice; a patch larger than the slice is zero-padded
    p = ds.extract_slice_patch(vol, 4, (1, 16, 16))
    assert p.shape == (1, 16, 16) and np.array_equal(p[0, :12, :10], vol[2]) and not p[0, 12:].any() and not p[0, :, 10:].any()
    assert np.array_equal(ds.extract_slice_patch(vol, 1, (1, 12, 10))[0], vol[1])
    np.random.seed(0)
    q = ds.extract_slice_patch(vol, 0, (1, 4, 4))                       # a crop from inside slice 0
    y, x = np.argwhere(vol[0] == q[0, 0, 0])[0]
    assert np.array_equal(q[0], vol[0, y:y + 4, x:x + 4])
    item = ds[len(ds) - 1]                                             # slice 4 of a 3-slice volume
    assert item["input"].shape == item["target"].shape == (1, 1, 16, 16) and item["input"].dtype == torch.float32
    pid = item["patient_id"]
    assert pid == ds.patient_ids[-1]
    want = CTDiffDataset.normalize_hu(np.load(tmp_path / "vue_files" / f"{pid}_vue.npy"))[2]
    assert np.allclose(item["input"][0, 0, :12, :10].numpy(), want, atol=1e-6)
    pad = item["input"][0, 0, 12:].numpy()                              # zeros (0 HU) added BEFORE the normalisation
    assert np.allclose(pad, CTDiffDataset.normalize_hu(np.zeros(1)), atol=1e-7)
    with pytest.raises(ValueError):
        CTDiffDataset(str(tmp_path), mode="test")


@pytest.mark.parametrize("n,val_size", [(3, 0.15), (7, 0.15), (20, 0.15), (20, 0.3)])
def test_split_is_sklearns(n, val_size):
    ids = [f"P{i}" for i in range(n)]
    train, val = split_ids(ids, val_size, 42)
    assert len(val) == int(np.ceil(val_size * n)) and len(train) == n - len(val)
    assert sorted(train + val) == sorted(ids)
    sk = pytest.importorskip("sklearn.model_selection")
    want_train, want_val = sk.train_test_split(ids, test_size=val_size, random_state=42)
    assert train == want_train and val == want_val


# ---------------------------------------------------------------------------------------
# the trainer on the CPU
# ---------------------------------------------------------------------------------------
def test_fit_writes_checkpoints_load_model_reads(tmp_path, monkeypatch):
    _write_patients(tmp_path / "data", 3)
    cfg = _config(tmp_path, monkeypatch, patch_size=(1, 16, 16), patches_per_volume=2, num_epochs=2, save_interval=2,
                  gradient_accumulation_steps=2, num_workers=0, use_mixed_precision=False)
    torch.manual_seed(0)
    trainer = UNetTrainer(nmodel.build_model(cfg), cfg, device="cpu")
    train_loader, val_loader = get_dataloaders(str(tmp_path / "data"), 1, 0, cfg.val_size, True, cfg.patch_size, 2)
    hist = trainer.fit(train_loader, val_loader)
    assert len(hist["train"]) == 2 and all(np.isfinite(hist["train"] + hist["val"]))
    for name in ("latest.pth", "best.pth", "epoch_2.pth"):
        assert os.path.isfile(os.path.join(cfg.checkpoint_dir, name)), name
    ckpt = torch.load(os.path.join(cfg.checkpoint_dir, "latest.pth"), weights_only=True)
    assert {"model_state_dict", "config", "optimizer_state_dict", "epoch", "best_val_loss"} <= set(ckpt)
    assert ckpt["epoch"] == 2 and ckpt["best_val_loss"] == min(hist["val"])
    assert {"base_channels", "in_channels", "out_channels", "model_type"} <= set(ckpt["config"])
    model, c = load_model(os.path.join(cfg.checkpoint_dir, "best.pth"), "cpu")
    assert type(model) is UNet3DLight and (c.base_channels, c.in_channels, c.out_channels) == (8, 1, 1)
    latest, _ = load_model(os.path.join(cfg.checkpoint_dir, "latest.pth"), "cpu")
    for k, v in trainer.model.state_dict().items():
        assert torch.equal(latest.state_dict()[k], v), k
    # resume: the epoch, the best loss and Adam's state come back
    again = UNetTrainer(nmodel.build_model(cfg), cfg, device="cpu")
    again.load(os.path.join(cfg.checkpoint_dir, "latest.pth"))
    assert again.epoch == 2 and again.best_val_loss == trainer.best_val_loss
    assert again.optimizer.state_dict()["state"][0]["step"] == trainer.optimizer.state_dict()["state"][0]["step"]


def test_one_value_per_channel_raises():
    """One 8x8 slice through UNet3DLight leaves a 1x1 map at the bottom: torch's own error."""
    model = UNet3DLight(base_channels=8)
    x = torch.zeros(1, 1, 1, 8, 8)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        reference_step(model, x, x)
    reference_step(model, torch.zeros(2, 1, 1, 8, 8), torch.zeros(2, 1, 1, 8, 8))   # two slices: fine


def test_unsupported_configurations_raise(tmp_path, monkeypatch):
    ok = _config(tmp_path, monkeypatch)
    UNetTrainer(UNet3DLight(base_channels=8), ok, device="cpu")
    for kw in ({"patch_size": (4, 16, 16)}, {"ssim_weight": 0.1}):
        with pytest.raises(ValueError):
            UNetTrainer(UNet3DLight(base_channels=8), _config(tmp_path, monkeypatch, **kw), device="cpu")
    for bad in (UNet3DLight(trilinear=False, base_channels=8), UNet3DLight(n_channels=2, base_channels=8),
                UNet3DLight(n_classes=2, base_channels=8)):
        with pytest.raises(ValueError):
            UNetTrainer(bad, ok, device="cpu")
    t = UNetTrainer(UNet3DLight(base_channels=8), ok, device="cpu")
    with pytest.raises(ValueError):
        t.train_step(torch.zeros(1, 1, 2, 16, 16), torch.zeros(1, 1, 2, 16, 16))   # a depth-2 patch
