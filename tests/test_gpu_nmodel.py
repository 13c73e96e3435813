"""The difference-map stage on the GPU (csrc/unet.hip, modules/hip/unet.py, modules/nmodel): each new
kernel alone against ATen / numpy on the CPU, the whole forward against the reference's float64
output (tests/golden/nmodel_unet.npz), chunk invariance, predict_volume, and both generate.py
pipelines with --apply_diffmap."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN
from modules import nmodel
from modules.hip import ops
from modules.hip import unet as U
from modules.model import Generator
from modules.nmodel import UNet3D, UNet3DLight, predict_volume, predict_volume_device
from modules.postprocess import apply_diffmap
from modules.postprocess_gpu import apply_diffmap_device
from test_cpu_dicom import _write_tree
from test_cpu_nmodel import G, seeded_model
from test_gpu_resident import _load_generate, _series

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _rand(seed, shape, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * (hi - lo) + lo


def _affine(seed, C):
    """A folded BatchNorm with scales of both signs."""
    scale = _rand(seed, (C,), 0.5, 1.5) * torch.where(torch.arange(C) % 3 == 1, -1.0, 1.0)
    return scale, _rand(seed + 1, (C,), -0.3, 0.3)


# ---------------------------------------------------------------------------------------
# each kernel alone
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(7, 5), (8, 8)])
def test_affine_relu_pool_is_exact(H, W):
    N, C = 2, 8
    y, (scale, shift) = _rand(1, (N, H, W, C), -2, 2), _affine(2, C)
    a = F.relu(y * scale + shift)                                   # float32, one rounding per step
    want_pool = F.max_pool2d(a.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    skip, pooled = U.affine_relu_pool(y.to(DEV), scale.to(DEV), shift.to(DEV))
    assert pooled.shape == (N, H // 2, W // 2, C)
    assert torch.equal(skip.cpu(), a) and torch.equal(pooled.cpu(), want_pool)
    # the skip as the leading channels of a wider tensor: the other channels stay as they were
    cat = torch.full((N, H, W, C + 4), 7.0, device=DEV)
    _, pooled2 = U.affine_relu_pool(y.to(DEV), scale.to(DEV), shift.to(DEV), skip=cat)
    assert torch.equal(cat[..., :C].cpu(), a) and bool((cat[..., C:] == 7.0).all()) and torch.equal(pooled2, pooled)


@pytest.mark.parametrize("h,w,Ho,Wo", [(3, 2, 7, 5), (2, 3, 5, 7), (1, 4, 2, 8), (4, 1, 8, 2), (1, 1, 3, 3)])
def test_upsample2_pad_matches_aten(h, w, Ho, Wo):
    N, C = 2, 8
    x, (scale, shift) = _rand(3, (N, h, w, C)), _affine(4, C)

    def want(src):
        up = F.interpolate(src.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True)
        dh, dw = Ho - up.shape[2], Wo - up.shape[3]
        return F.pad(up, [dw // 2, dw - dw // 2, dh // 2, dh - dh // 2]).permute(0, 2, 3, 1)

    got = U.upsample2_pad(x.to(DEV), (Ho, Wo)).cpu()
    assert got.shape == (N, Ho, Wo, C)
    err = float((got - want(x)).abs().max())
    assert err <= 1e-6, err
    if h == 1 and w == 1:   # every output inside the 2x2 map is that pixel
        assert torch.equal(got[:, 0:2, 0:2], x.expand(N, 2, 2, C)) and bool((got[:, 2] == 0).all())
    # with the source's affine + ReLU, into the channels behind a skip
    cat = torch.full((N, Ho, Wo, 4 + C), 7.0, device=DEV)
    U.upsample2_pad(x.to(DEV), (Ho, Wo), scale.to(DEV), shift.to(DEV), out=cat, channel_offset=4)
    err = float((cat[..., 4:].cpu() - want(F.relu(x * scale + shift))).abs().max())
    assert err <= 1e-6 * 2, err                      # data in [-1, 1] mapped into [0, 1.8]: the bound scales with it
    assert bool((cat[..., :4] == 7.0).all())


def test_output_kernel_equals_the_host_tail():
    thr = 8
    d = np.concatenate([np.array([7.9990234, 8.0, 8.0009766, 0.0, -3.5, 255.0, 255.99, 256.0, 257.5, 300.0, 511.9,
                                  512.0, 3999.0, 4000.0, 4321.0, -4000.0, 7.5, 8.5], dtype=np.float32),
                        np.random.default_rng(5).uniform(-50, 600, 1003).astype(np.float32)])
    t = (d / np.float32(2000) - np.float32(1)).astype(np.float32)       # the logits
    # o = relu(t) * 1 + relu(-t) * -1 is t exactly: the projection adds no rounding of its own
    y = np.zeros((t.size, 4), np.float32)
    y[:, 0], y[:, 1], y[:, 2] = t, -t, 3.0
    one, zero = torch.ones(4, device=DEV), torch.zeros(4, device=DEV)
    w = torch.tensor([1.0, -1.0, 0.0, 0.0], device=DEV)
    vol = np.round(np.random.default_rng(6).uniform(-1000, 3000, t.size)).astype(np.float32) + np.float32(0.25)
    denorm = nmodel.denormalize_diff(t)
    assert (denorm < thr).any() and (denorm >= 256).any() and (denorm < 0).any()
    want = nmodel.diffmap_tail(vol, t, thr)
    merged = torch.from_numpy(vol.copy()).to(DEV)
    diff = U.out_diffmap(torch.from_numpy(y).to(DEV), one, zero, w, 0.0, thr, volume=merged, want_diff=True)
    assert np.array_equal(diff.cpu().numpy(), denorm)                # un-thresholded, as predict_volume returns it
    assert np.array_equal(merged.cpu().numpy(), want)
    only = torch.from_numpy(vol.copy()).to(DEV)
    assert U.out_diffmap(torch.from_numpy(y).to(DEV), one, zero, w, 0.0, thr, volume=only) is None
    assert torch.equal(only, merged)
    # apply_diffmap_device: the same tail for a map that already exists
    dd = torch.from_numpy(denorm).to(DEV)
    got = apply_diffmap_device(torch.from_numpy(vol).to(DEV), dd, thr)
    assert np.array_equal(got.cpu().numpy(), apply_diffmap(vol.copy(), denorm.copy(), thr))
    assert np.array_equal(dd.cpu().numpy(), denorm)                  # the device map is left as it was
    for other in (0, 100.5):
        got = apply_diffmap_device(torch.from_numpy(vol).to(DEV), dd, other)
        assert np.array_equal(got.cpu().numpy(), apply_diffmap(vol.copy(), denorm.copy(), other))


@pytest.mark.parametrize("C", [8, 16, 32, 64, 256])   # one lane per pixel up to 16 channels, then C / 16 lanes
def test_output_kernel_projection(C):
    """affine + ReLU + 1x1 projection with bias against float64: C float32 products and sums."""
    P = 777
    y, (scale, shift), w = _rand(7, (P, C), -2, 2), _affine(8, C), _rand(9, (C,))
    a = F.relu(y.double() * scale.double() + shift.double())
    o = a @ w.double() + 0.125
    got = U.out_diffmap(y.to(DEV), scale.to(DEV), shift.to(DEV), w.to(DEV), 0.125, want_diff=True).cpu().double()
    # every product and sum rounds once, 2^-24 relative to a running magnitude of at most sum |a||w| + |bias|; so
    # do the two steps of the affine map and the three of the tail, the latter on o + 1
    bound = (C + 6) * 2.0 ** -24 * float((a.abs() @ w.abs().double() + 0.125 + 1.0).max())
    assert float((got / 2000 - 1 - o).abs().max()) <= bound


@pytest.mark.parametrize("n", [4096, 1001])
def test_normalize_hu_equals_the_host_form(n):
    hu = np.random.default_rng(n).uniform(-2000, 4000, n).astype(np.float32)
    hu[:6] = [-1024, 3071, -1024.0001, 3071.0005, 0, -5000]
    want = nmodel.normalize_hu(hu)
    dev = torch.from_numpy(hu).to(DEV)
    assert np.array_equal(U.normalize_hu(dev).cpu().numpy(), want)
    x4 = U.normalize_hu(dev.view(1, n), pad4=True).cpu().numpy()
    assert x4.shape == (1, n, 4) and np.array_equal(x4[0, :, 0], want) and not x4[..., 1:].any()


# ---------------------------------------------------------------------------------------
# the whole forward
# ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "nmodel_unet.npz"))


_MODELS = {}


def _model(case):
    cls, base, seed = G.CASES[case][:3]
    if (cls, base, seed) not in _MODELS:
        _MODELS[(cls, base, seed)] = seeded_model(cls, base, seed).to(DEV)
    return _MODELS[(cls, base, seed)]


def _logits_error(model, x, want64):
    """max |device logits - want64| of normalised slices x [N,H,W] (numpy), the logits recovered
    from the difference map the output kernel writes (an exact affine map of them up to its
    float32 rounding, which only adds to the error reported)."""
    plan = U.plan_for(model, DEV)
    x4 = torch.zeros(x.shape + (4,), device=DEV)
    x4[..., 0] = torch.from_numpy(x).to(DEV)
    y, last = U.forward(plan, x4)
    d = U.out_diffmap(y, last.scale, last.shift, plan.out_weight, plan.out_bias, want_diff=True)
    return float(np.abs(d.cpu().numpy().astype(np.float64) / 2000.0 - 1.0 - want64).max())


@pytest.mark.parametrize("case", sorted(G.CASES))
def test_forward_against_the_reference_float64(golden, case):
    """Bar: 4 x delta32, the reference's own float32-against-float64 spread of the case.
    Measured (default mode f16x3 -> bf16x6 passes; f16 -> bf16 passes, no bar): see DESIGN.md §3."""
    assert ops.get_mma() == "f16x3"
    model, x, want = _model(case), golden[f"x:{case}"], golden[f"y64:{case}"]
    bar = 4.0 * float(golden[f"delta32:{case}"])
    err = _logits_error(model, x, want)
    try:
        ops.set_mma("f16")
        err16 = _logits_error(model, x, want)
    finally:
        ops.set_mma("f16x3")
    print(f"nmodel case {case}: max error vs float64 {err:.3e} (bar {bar:.3e}, delta32 {bar / 4:.3e}); "
          f"f16 operand mode {err16:.3e} (no bar)")
    assert err <= bar, f"case {case}: max error {err:.3e} above 4 x delta32 = {bar:.3e}"


def test_full_model_at_its_default_width():
    """UNet3D base 32 reaches 256 -> 256 convolutions, which the Generator's residual blocks run in
    another K order: here they take the plain rows pass.  Against the mirror's float64 CPU forward,
    bar 4 x the mirror's own float32 spread."""
    torch.manual_seed(3)
    model = UNet3D().eval()
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm3d):
            m.running_mean.normal_(0, 0.3)
            m.running_var.uniform_(0.5, 1.5)
            m.weight.data.uniform_(0.5, 1.5).mul_(torch.where(torch.rand(m.weight.shape) < 0.3, -1.0, 1.0))
            m.bias.data.uniform_(-0.3, 0.3)
        elif isinstance(m, torch.nn.Conv3d) and m.kernel_size == (3, 3, 3):
            m.weight.data.normal_(0, (2.0 / (9 * m.in_channels)) ** 0.5)
    x = _rand(10, (1, 16, 16)).numpy()
    with torch.no_grad():
        t = torch.from_numpy(x)[:, None, None]
        y32 = model(t)[:, 0, 0].numpy().astype(np.float64)
        y64 = model.double()(t.double())[:, 0, 0].numpy()
    bar = 4.0 * float(np.abs(y32 - y64).max())
    err = _logits_error(model.float().to(DEV), x, y64)
    print(f"UNet3D base 32, 16x16: max error vs float64 {err:.3e} (bar {bar:.3e})")
    assert err <= bar, (err, bar)


@pytest.fixture(scope="module")
def hu_volume():
    hu = np.random.default_rng(12).uniform(-1100, 1500, (5, 28, 20)).astype(np.float32)
    hu[0, :4] = 3500
    return hu


def test_chunk_size_changes_nothing(hu_volume):
    model, hu = _model("a"), torch.from_numpy(hu_volume).to(DEV)
    ref = predict_volume_device(model, hu, chunk=5)
    assert ref.shape == hu.shape and ref.dtype == torch.float32 and bool(torch.isfinite(ref).all())
    assert float(ref.std()) > 0
    for chunk in (1, 2):
        assert torch.equal(predict_volume_device(model, hu, chunk=chunk), ref), chunk
    assert torch.equal(predict_volume_device(model, hu), ref)


def test_predict_volume_is_the_device_function_plus_transfers(hu_volume):
    model = _model("a")
    got = predict_volume(model, hu_volume, device=DEV, use_amp=True)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32
    assert np.array_equal(got, predict_volume_device(model, torch.from_numpy(hu_volume).to(DEV)).cpu().numpy())
    # the fused stage adds what apply_diffmap adds
    merged = np.round(np.random.default_rng(13).uniform(-1000, 2000, hu_volume.shape)).astype(np.float32)
    on_dev = torch.from_numpy(merged).to(DEV)
    diff = nmodel.apply_predicted_diffmap_device(model, torch.from_numpy(hu_volume).to(DEV), on_dev, 8, want_diff=True)
    assert np.array_equal(diff.cpu().numpy(), got)
    assert np.array_equal(on_dev.cpu().numpy(), apply_diffmap(merged.copy(), got.copy(), 8))


def test_unsupported_models_and_inputs_raise(hu_volume):
    hu = torch.from_numpy(hu_volume).to(DEV)
    with pytest.raises(ValueError):
        predict_volume_device(UNet3DLight(trilinear=False).to(DEV).eval(), hu)
    with pytest.raises(ValueError):
        predict_volume_device(UNet3DLight(n_classes=2).to(DEV).eval(), hu)
    with pytest.raises(ValueError):
        predict_volume_device(UNet3DLight(n_channels=2).to(DEV).eval(), hu)
    with pytest.raises(ValueError):
        predict_volume_device(_model("a"), hu[:, :7])               # 7 rows do not survive three pools
    with pytest.raises(RuntimeError):
        predict_volume_device(_model("a"), hu.cpu())                 # no CPU fallback
    with pytest.raises(ValueError):
        predict_volume_device(_model("a"), hu[0])


# ---------------------------------------------------------------------------------------
# generate.py
# ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """One patient of 5 slices at 64x64, the two Generator checkpoints, a seeded U-Net checkpoint."""
    root = tmp_path_factory.mktemp("nmodel")
    _write_tree(str(root / "in" / "DS"), patients=1, slices=5, size=64)
    torch.manual_seed(0)
    paths = {}
    for name, g in (("soft", Generator(3, 9)), ("lung", Generator(2, 9))):
        paths[name] = str(root / f"{name}.pth")
        torch.save(g.state_dict(), paths[name])
    unet = seeded_model("UNet3DLight", 16, 11)
    paths["unet"] = str(root / "unet.pth")
    torch.save({"model_state_dict": unet.state_dict(),
                "config": {"base_channels": 16, "in_channels": 1, "out_channels": 1}}, paths["unet"])
    base = ["--dataset_names", "DS", "--img_size", "64", "--slice_batch", "2", "--model_path_soft", paths["soft"],
            "--model_path_lung", paths["lung"], "--input_dir_root", str(root / "in")]
    return root, base, paths["unet"]


def _run(gen, root, base, tag, extra, resident, work=None):
    """One run of generate.py's functions; ``work``: synthesis() alone on that run's working series."""
    args = gen.get_args(base + ["--working_dir_root", str(root / f"w_{work or tag}"),
                                "--output_dir_root", str(root / f"o_{tag}"),
                                *(["--pipeline", "resident"] if resident else []), *extra])
    if resident:
        gen.generate_synthesis(args)
    else:
        if work is None:
            gen.generate(args)
        gen.synthesis(args)
    return root / f"o_{tag}" / "DS" / "P0", root / f"w_{work or tag}" / "DS" / "P0"


def test_pipelines_agree_with_the_stage(tree):
    root, base, unet = tree
    gen = _load_generate()
    flags = ["--apply_diffmap", "--nmodel_path", unet, "--save_diff"]
    out_s, work_s = _run(gen, root, base, "staged", flags, False)
    out_d, _ = _run(gen, root, base, "staged_dev", flags + ["--postprocess_device", "cuda"], False, work="staged")
    out_r, work_r = _run(gen, root, base, "res", flags, True)
    names, want = _series(out_s)
    assert names == [f"{i:04d}.dcm" for i in range(5)]
    for other in (out_d, out_r):
        got_names, got = _series(other)
        assert got_names == names
        for w, g in zip(want, got):
            assert g.pixel_array.dtype == w.pixel_array.dtype and np.array_equal(g.pixel_array, w.pixel_array)
    ds, dr = np.load(work_s / "diff.npy"), np.load(work_r / "diff.npy")
    assert ds.shape == (5, 64, 64) and ds.dtype == np.float32 and np.array_equal(ds, dr)
    assert (ds >= 8).any()                                           # the stage adds something
    # a threshold above every value: nothing is added, the files are the plain run's
    top = ["--apply_diffmap", "--nmodel_path", unet, "--diffmap_threshold", str(float(ds.max()) + 1)]
    out_t, _ = _run(gen, root, base, "res_top", top, True)
    out_p, work_p = _run(gen, root, base, "res_plain", [], True)
    assert not os.path.exists(work_p)
    _, plain = _series(out_p)
    for p, t in zip(plain, _series(out_t)[1]):
        assert np.array_equal(p.pixel_array, t.pixel_array)
    assert any(not np.array_equal(p.pixel_array, w.pixel_array) for p, w in zip(plain, want))


def test_without_the_flag_nothing_changes(tree):
    """No --apply_diffmap: the checkpoint is not read (its path may not even exist) and the resident
    result is the one without the stage."""
    root, base, unet = tree
    gen = _load_generate()
    out_a, _ = _run(gen, root, base, "off_present", ["--nmodel_path", unet], True)
    out_b, _ = _run(gen, root, base, "off_absent", ["--nmodel_path", str(root / "missing.pth")], True)
    na, a = _series(out_a)
    nb, b = _series(out_b)
    assert na == nb and len(na) == 5
    for x, y in zip(a, b):
        assert np.array_equal(x.pixel_array, y.pixel_array)
    with pytest.raises(FileNotFoundError):
        _run(gen, root, base, "on_absent", ["--apply_diffmap", "--nmodel_path", str(root / "missing.pth")], True)
