"""The enhancement-difference synthesis ("sCECT v3") on the GPU, everything bit-exact against the host
function modules/inference.py::synthesize_enhancement: the staged kernel (csrc/volume.hip,
merge_enhancement), the resident kernel behind the Generators (csrc/slices.hip, translate_enhance),
translate_volume_device(synthesis="enhancement"), and generate.py's three paths."""
import numpy as np
import pytest
import torch

from modules import dicom
from modules.hip import slices as S
from modules.hip import volume as V
from modules.inference import (stored_from_output, synthesize_enhancement, synthesize_volume,
                               translate_volume_device)
from modules.model import Generator
from test_cpu_dicom import _write_tree
from test_cpu_enhance import BOUNDARY, DTYPES, PAIRS, SHAPES, draw_series, load_generate, write_working
from test_cpu_nmodel import seeded_model
from test_gpu_resident import HEADER, _series, _staged, _uint16_series

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SOFT, LUNG = (-150, 250), (-1000, -150)
# (0.5, 0) maps the lung range to negative stored values, which a uint16 series cannot hold (numpy's
# cast is undefined there); the unsigned translate cases shift that slice's intercept instead
PAIRS_U16 = [(1.0, -1024.0), (0.5, -1024.0), (0.7, -1000.0)]


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(DEV)


def _f32(v):
    return torch.from_numpy(np.asarray(v, np.float32)).to(DEV)


def _host(raw, soft, lung, slopes, inters, *rule):
    return np.stack([synthesize_enhancement(raw[k], soft[k], lung[k], slopes[k], inters[k], *rule)
                     for k in range(len(raw))])


@pytest.mark.parametrize("dtype", DTYPES, ids=["int16", "uint16"])
@pytest.mark.parametrize("shape", SHAPES, ids=["scalar-odd", "vector", "two-blocks-tail"])
def test_merge_enhancement_matches_host(shape, dtype):
    raw, soft, lung, slopes, inters = draw_series(shape, dtype)
    want = _host(raw, soft, lung, slopes, inters)
    assert want[0].ravel()[:len(BOUNDARY)].tolist() == [v[1] for v in BOUNDARY]
    got = V.merge_enhancement(_up(raw), _up(soft), _up(lung), _f32(slopes), _f32(inters),
                              unsigned=dtype == np.uint16)
    assert got.dtype == torch.float32 and got.shape == raw.shape
    assert np.array_equal(got.cpu().numpy(), want)
    # other settings reach the kernel, and synthesize_volume's device route is this kernel
    got = V.merge_enhancement(_up(raw), _up(soft), _up(lung), _f32(slopes), _f32(inters), 12.5, -300.0,
                              unsigned=dtype == np.uint16)
    other = _host(raw, soft, lung, slopes, inters, 12.5, -300.0)
    assert np.array_equal(got.cpu().numpy(), other) and not np.array_equal(other, want)
    vol = synthesize_volume(raw, slopes, inters, soft, lung, SOFT, LUNG, device=DEV, mode="enhancement")
    assert isinstance(vol, np.ndarray) and vol.dtype == np.float32 and np.array_equal(vol, want)
    kept = synthesize_volume(raw, slopes, inters, soft, lung, SOFT, LUNG, device=DEV, keep_on_device=True,
                             mode="enhancement")
    assert kept.is_cuda and np.array_equal(kept.cpu().numpy(), want)


def _translate_case(shape, dtype, seed=3):
    """Raw values whose HU lies in [-600, 400] (around both thresholds and both models' ranges), model
    outputs in [-1, 1] with exact +-1 among them, slice k with pair k % 3."""
    rng = np.random.default_rng(seed)
    pairs = [(PAIRS_U16 if dtype == np.uint16 else PAIRS)[k % 3] for k in range(shape[0])]
    hu = rng.integers(-600, 401, size=shape)
    raw = np.stack([np.round((hu[k] - b) / a) for k, (a, b) in enumerate(pairs)]).astype(dtype)
    ys, yl = (rng.uniform(-1, 1, size=shape).astype(np.float32) for _ in range(2))
    for y in (ys, yl):
        y.reshape(-1)[:4] = (1.0, -1.0, -1.0, 1.0)
        y.reshape(-1)[-2:] = (-1.0, 1.0)
    return raw, [a for a, _ in pairs], [b for _, b in pairs], ys, yl


@pytest.mark.parametrize("dtype", DTYPES, ids=["int16", "uint16"])
@pytest.mark.parametrize("shape", SHAPES, ids=["scalar-odd", "vector", "two-blocks-tail"])
def test_translate_enhance_matches_host(shape, dtype):
    raw, slopes, inters, ys, yl = _translate_case(shape, dtype)
    D = shape[0]
    so = np.stack([stored_from_output(ys[k], *SOFT, slopes[k], inters[k], dtype) for k in range(D)])
    lo = np.stack([stored_from_output(yl[k], *LUNG, slopes[k], inters[k], dtype) for k in range(D)])
    if dtype == np.uint16:   # nothing negative to wrap
        assert min(((LUNG[0] - b) / a) for a, b in zip(slopes, inters)) >= 0
    want = _host(raw, so, lo, slopes, inters)
    assert (want != raw).any() and (want == raw).any() and (want != np.trunc(want)).any() == (0.7 in slopes)
    unsigned = dtype == np.uint16
    args = (_up(raw), _f32(slopes), _f32(inters), torch.from_numpy(ys).to(DEV), torch.from_numpy(yl).to(DEV))
    gs, gl, gm = S.translate_enhance(*args, SOFT, LUNG, unsigned=unsigned, want_stored=True)
    assert np.array_equal(gs.cpu().numpy().view(dtype), so)
    assert np.array_equal(gl.cpu().numpy().view(dtype), lo)
    assert gm.dtype == torch.float32 and np.array_equal(gm.cpu().numpy(), want)
    ns, nl, only = S.translate_enhance(*args, SOFT, LUNG, unsigned=unsigned)
    assert ns is None and nl is None and torch.equal(only, gm)
    # the staged kernel on the stored series gives the same tensor
    assert torch.equal(V.merge_enhancement(args[0], gs, gl, args[1], args[2], unsigned=unsigned), gm)
    _, _, other = S.translate_enhance(*args, SOFT, LUNG, 40.0, -200.0, unsigned=unsigned)
    assert np.array_equal(other.cpu().numpy(), _host(raw, so, lo, slopes, inters, 40.0, -200.0))
    assert not torch.equal(other, gm)


def test_bad_input_raises():
    raw, soft, lung, slopes, inters = draw_series((2, 8, 16), np.int16)
    r, s, g, a, b = _up(raw), _up(soft), _up(lung), _f32(slopes), _f32(inters)
    ys = torch.zeros(raw.shape, dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError):   # host tensors: no CPU fallback
        V.merge_enhancement(r.cpu(), s, g, a, b)
    with pytest.raises(RuntimeError):
        V.merge_enhancement(r, s, g.cpu(), a, b)
    with pytest.raises(RuntimeError):
        S.translate_enhance(r.cpu(), a, b, ys, ys.clone(), SOFT, LUNG)
    with pytest.raises(RuntimeError):
        S.translate_enhance(r, a, b, ys.cpu(), ys, SOFT, LUNG)
    with pytest.raises(RuntimeError):   # wrong dtype
        V.merge_enhancement(r.float(), s, g, a, b)
    with pytest.raises(RuntimeError):
        S.translate_enhance(r, a, b, ys.double(), ys, SOFT, LUNG)
    with pytest.raises(ValueError):     # mismatched shapes
        V.merge_enhancement(r, s[:1], g, a, b)
    with pytest.raises(ValueError):
        S.translate_enhance(r, a, b, ys[:1], ys, SOFT, LUNG)
    with pytest.raises(ValueError):     # a wrong number of slopes
        V.merge_enhancement(r, s, g, a[:1], b)
    with pytest.raises(ValueError):
        S.translate_enhance(r, a, b[:1], ys, ys.clone(), SOFT, LUNG)
    with pytest.raises(ValueError):
        translate_volume_device(None, None, raw, slopes, inters, SOFT, LUNG, 64, 2, DEV, synthesis="v3")
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def models():
    torch.manual_seed(0)
    return Generator(3, 9).to(DEV).eval(), Generator(2, 9).to(DEV).eval()


@pytest.mark.parametrize("unsigned", [False, True], ids=["int16", "uint16"])
def test_resident_volume_equals_the_staged_functions(models, unsigned):
    """3 slices of 64x64 at the network's own size, batch 2."""
    from modules import phantom
    raw, slopes, inters = _uint16_series() if unsigned else phantom.ct_batch(3, 3, 64)
    so, lo, _ = _staged(*models, raw, slopes, inters, 64, 2)
    want = _host(raw, so, lo, slopes, inters)
    assert (want != raw).any() and (want == raw).any()
    merged, gs, gl = translate_volume_device(*models, raw, slopes, inters, SOFT, LUNG, 64, 2, DEV, want_stored=True,
                                             synthesis="enhancement")
    assert merged.is_cuda and merged.dtype == torch.float32 and merged.shape == raw.shape
    assert np.array_equal(gs.cpu().numpy().view(raw.dtype), so)
    assert np.array_equal(gl.cpu().numpy().view(raw.dtype), lo)
    assert np.array_equal(merged.cpu().numpy(), want)
    only = translate_volume_device(*models, raw, slopes, inters, SOFT, LUNG, 64, 2, DEV, synthesis="enhancement")
    assert torch.equal(only, merged)
    other = translate_volume_device(*models, raw, slopes, inters, SOFT, LUNG, 64, 2, DEV, synthesis="enhancement",
                                    enhancement_threshold=30.0, enhancement_min_hu=-100.0)
    assert np.array_equal(other.cpu().numpy(), _host(raw, so, lo, slopes, inters, 30.0, -100.0))


# ---------------------------------------------------------------------------------------
# generate.py
# ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tree(tmp_path_factory, models):
    """One patient of 5 slices at 64x64, the two Generator checkpoints, a seeded U-Net checkpoint."""
    root = tmp_path_factory.mktemp("enhance")
    _write_tree(str(root / "in" / "DS"), patients=1, slices=5, size=64)
    paths = {}
    for name, g in zip(("soft", "lung"), models):
        paths[name] = str(root / f"{name}.pth")
        torch.save(g.state_dict(), paths[name])
    paths["unet"] = str(root / "unet.pth")
    torch.save({"model_state_dict": seeded_model("UNet3DLight", 16, 11).state_dict(),
                "config": {"base_channels": 16, "in_channels": 1, "out_channels": 1}}, paths["unet"])
    base = ["--dataset_names", "DS", "--img_size", "64", "--slice_batch", "2", "--model_path_soft", paths["soft"],
            "--model_path_lung", paths["lung"], "--input_dir_root", str(root / "in")]
    return root, base, paths["unet"]


def _args(gen, root, base, tag, extra, work=None):
    return gen.get_args(base + ["--working_dir_root", str(root / f"w_{work or tag}"),
                                "--output_dir_root", str(root / f"o_{tag}"), *extra])


def _same_files(want_dir, got_dir, n=5):
    names, want = _series(want_dir)
    got_names, got = _series(got_dir)
    assert got_names == names == [f"{i:04d}.dcm" for i in range(n)]
    for w, g in zip(want, got):
        assert g.pixel_array.dtype == w.pixel_array.dtype and np.array_equal(g.pixel_array, w.pixel_array)
        for key in HEADER:
            assert w.get(key) is not None and g.get(key) == w.get(key), key
    return want, got


def test_entry_point_three_paths_write_the_same_files(tree):
    root, base, unet = tree
    gen = load_generate("dcs_gen_enh_gpu")
    flag = ["--synthesis", "enhancement"]
    host = _args(gen, root, base, "host", flag, work="staged")
    gen.generate(host)
    gen.synthesis_test(host)
    gen.synthesis_test(_args(gen, root, base, "cuda", flag + ["--postprocess_device", "cuda"], work="staged"))
    gen.generate_synthesis(_args(gen, root, base, "res", flag + ["--pipeline", "resident"]))
    out = lambda tag: root / f"o_{tag}" / "DS" / "P0"
    want, _ = _same_files(out("host"), out("cuda"))
    _same_files(out("host"), out("res"))
    assert all(w.SeriesDescription == "DuCoSyGAN sCECT v3" for w in want)
    # not the v2 series: the range mode on the same working directory writes other pixels
    gen.synthesis(_args(gen, root, base, "v2", [], work="staged"))
    _, v2 = _series(out("v2"))
    assert all(v.SeriesDescription == "DuCoSyGAN sCECT v2" for v in v2)
    assert any(not np.array_equal(v.pixel_array, w.pixel_array) for v, w in zip(v2, want))
    # the difference-map stage in enhancement mode: staged on the device against resident
    dm = flag + ["--apply_diffmap", "--nmodel_path", unet]
    gen.synthesis_test(_args(gen, root, base, "cuda_dm", dm + ["--postprocess_device", "cuda"], work="staged"))
    gen.generate_synthesis(_args(gen, root, base, "res_dm", dm + ["--pipeline", "resident"]))
    with_dm, _ = _same_files(out("cuda_dm"), out("res_dm"))
    assert any(not np.array_equal(d.pixel_array, w.pixel_array) for d, w in zip(with_dm, want))
    # --synthesis range is the run without the flag
    gen.generate_synthesis(_args(gen, root, base, "res_plain", ["--pipeline", "resident"]))
    gen.generate_synthesis(_args(gen, root, base, "res_range", ["--pipeline", "resident", "--synthesis", "range"]))
    _same_files(out("res_plain"), out("res_range"))
    _same_files(out("v2"), out("res_plain"))


def test_series_with_their_own_rescale_pairs_merge_on_the_host(tmp_path, capsys):
    gen = load_generate("dcs_gen_enh_gpu2")
    raw, soft, lung, slopes, inters = draw_series((3, 8, 16), np.int16, seed=4)
    write_working(str(tmp_path / "w"), raw, soft, lung, slopes, inters, soft_inter_shift=3.0)
    common = ["--dataset_names", "DS", "--working_dir_root", str(tmp_path / "w"), "--synthesis", "enhancement"]
    gen.synthesis_test(gen.get_args(common + ["--output_dir_root", str(tmp_path / "host")]))
    capsys.readouterr()
    gen.synthesis_test(gen.get_args(common + ["--output_dir_root", str(tmp_path / "cuda"),
                                              "--postprocess_device", "cuda"]))
    assert "merging on the host" in capsys.readouterr().out
    want, _ = _same_files(tmp_path / "host" / "DS" / "P0", tmp_path / "cuda" / "DS" / "P0", n=3)
    from modules.inference import smooth_volume
    merged = np.stack([synthesize_enhancement(raw[k], soft[k], lung[k], slopes[k], inters[k],
                                              soft_rescale=(slopes[k], inters[k] + 3.0)) for k in range(3)])
    assert np.array_equal(np.stack([w.pixel_array for w in want]), smooth_volume(merged))
    assert not np.array_equal(merged, _host(raw, soft, lung, slopes, inters))
