"""Host side of the GPU volume post-processing (modules/postprocess_gpu.py,
modules/hip/volume.py, generate.py --postprocess_device): the Gaussian weights handed to the
kernel, the table of what runs on the device, the new flag, and the unchanged host defaults.
No GPU needed."""
import importlib.util
import os

import numpy as np
import pytest
from scipy.ndimage import gaussian_filter1d

from conftest import GOLDEN, ROOT


@pytest.mark.parametrize("sigma", [0.05, 0.3, 0.5, 0.7, 0.8, 1.0, 1.2, 1.5, 2.0, 3.0, 4.0])
def test_weights_equal_scipy_impulse_response(sigma):
    """gaussian_filter1d of a unit impulse returns the kernel itself: every other term of the
    correlation is a product with zero, so the comparison is exact."""
    from modules.hip.volume import gaussian_radius, gaussian_weights
    w = gaussian_weights(sigma)
    r = gaussian_radius(sigma)
    assert w.dtype == np.float64 and w.size == 2 * r + 1
    x = np.zeros(2 * r + 1 + 8, np.float64)
    x[r + 4] = 1.0
    got = gaussian_filter1d(x, sigma=sigma)[4:4 + 2 * r + 1]
    assert np.array_equal(got, w)
    assert np.array_equal(w, w[::-1])  # the kernel passes only w[0..r]


def test_kalman_gains_match_host_filter():
    from modules.hip.volume import kalman_gains
    from modules.postprocess import kalman_filter_1d
    z = np.random.default_rng(0).normal(0, 1, 12)
    for q, r in ((1e-5, 1e-2), (1e-3, 1e-1)):
        g = kalman_gains(z.size, q, r)
        x, want = z[0], []
        for k in range(z.size):
            x = x + g[k] * (z[k] - x)
            want.append(x)
        assert np.array_equal(np.array(want), kalman_filter_1d(z, q, r))


def test_gpu_supported_table():
    import torch
    from modules.postprocess_gpu import gpu_supported
    f32 = np.float32
    for m in ("gaussian", "gaussian3d", "adaptive", "median", "kalman"):
        assert gpu_supported(m, f32)
        assert gpu_supported(m, torch.float32)
        assert gpu_supported(m, f32, enhance_sharpness=False)
        for dt in (np.float64, np.int16, np.uint16, torch.float64):
            assert not gpu_supported(m, dt)
    assert not gpu_supported("interpolation", f32)
    assert not gpu_supported("bilateral", f32)
    # radius = int(4*sigma + 0.5) <= 16
    assert gpu_supported("gaussian", f32, sigma=4.1) and not gpu_supported("gaussian", f32, sigma=4.2)
    assert gpu_supported("gaussian3d", f32, sigma_z=0.7, sigma_xy=0.05, sharpen_amount=1.7, sharpen_radius=1.2)
    assert gpu_supported("gaussian3d", f32, sigma_z=0.0, sigma_xy=0.5)      # skipped axis
    assert not gpu_supported("gaussian3d", f32, sigma_z=5.0)
    assert not gpu_supported("gaussian3d", f32, sigma_xy=4.2)
    assert not gpu_supported("adaptive", f32, max_sigma=4.5)
    assert not gpu_supported("gaussian", f32, sharpen_radius=4.2)
    assert gpu_supported("gaussian", f32, sharpen_radius=4.2, enhance_sharpness=False)
    for k, ok in ((1, True), (3, True), (5, True), (7, True), (9, True), (4, False), (11, False), (0, False)):
        assert gpu_supported("median", f32, kernel_size=k) is ok, k


def _generate_module(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "ducosy-gan_amd", "generate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_postprocess_device_flag():
    gen = _generate_module("dcs_gen_pp")
    assert gen.get_args([]).postprocess_device == "cpu"
    assert gen.get_args(["--postprocess_device", "cuda"]).postprocess_device == "cuda"
    with pytest.raises(SystemExit):
        gen.get_args(["--postprocess_device", "tpu"])


def test_host_defaults_unchanged():
    from modules.inference import hu_from_stored, smooth_volume, synthesize, synthesize_volume
    z = np.load(os.path.join(GOLDEN, "postprocess.npz"))
    assert np.array_equal(smooth_volume(z["volume"]), z["synth"])
    assert np.array_equal(smooth_volume(z["volume"], device=None), z["synth"])
    rng = np.random.default_rng(3)
    raw, soft, lung = (rng.integers(0, 2000, (3, 5, 7)).astype(np.int16) for _ in range(3))
    slopes, inters = [1.0, 0.5, 2.0], [-1024.0, -1000.0, -1024.0]
    got = synthesize_volume(raw, slopes, inters, soft, lung, (-150, 250), (-1000, -150))
    for k in range(3):
        want = synthesize(raw[k], hu_from_stored(raw[k], slopes[k], inters[k]), soft[k], lung[k], (-150, 250),
                          (-1000, -150))
        assert np.array_equal(got[k], want)
    assert got.dtype == np.int16


def test_unknown_method_raises_without_device():
    from modules.postprocess_gpu import postprocess_ct_volume_gpu
    with pytest.raises(ValueError):
        postprocess_ct_volume_gpu(np.zeros((2, 3, 3), np.float32), method="bilateral")
