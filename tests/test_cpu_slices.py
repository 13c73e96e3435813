"""Host side of the resident inference path that needs no GPU: the antialiased-resize weight
tables (modules/hip/slices.py::aa_tables) against ATen's CPU resize, and generate.py's
--pipeline / --write_working arguments."""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT
from modules.hip.slices import MAX_TAPS, aa_tables

SHAPES = [((96, 96), (64, 64)), ((64, 64), (96, 96)), ((80, 48), (37, 53)), ((37, 53), (80, 48))]
IDS = ["96to64", "64to96", "80x48to37x53", "37x53to80x48"]


def apply_tables(x, out_size, axis):
    """The kernels' arithmetic in numpy: acc = acc + x * w from zero in tap order, float32."""
    start, count, w = aa_tables(x.shape[axis], out_size)
    x = np.moveaxis(x, axis, -1)
    acc = np.zeros(x.shape[:-1] + (out_size,), np.float32)
    for j in range(w.shape[1]):
        idx = np.minimum(start + j, x.shape[-1] - 1)   # padded taps have weight 0
        acc = acc + x[..., idx] * w[:, j]
    return np.moveaxis(acc, -1, axis)


def resize_by_tables(x, size):
    """Horizontal pass, then vertical pass, on [N,C,H,W]."""
    if x.shape[3] != size[1]:
        x = apply_tables(x, size[1], 3)
    if x.shape[2] != size[0]:
        x = apply_tables(x, size[0], 2)
    return x


@pytest.mark.parametrize("src,dst", SHAPES, ids=IDS)
def test_tables_reproduce_the_cpu_antialiased_resize(src, dst):
    x = np.random.default_rng(11).uniform(-1, 1, (2, 1) + src).astype(np.float32)
    want = F.interpolate(torch.from_numpy(x), size=dst, mode="bilinear", align_corners=False,
                         antialias=True).numpy()
    got = resize_by_tables(x, dst)
    assert got.dtype == np.float32 and got.shape == want.shape
    print("max abs difference", float(np.abs(got - want).max()))
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-6)


@pytest.mark.parametrize("n_in,n_out", [(96, 64), (64, 96), (80, 37), (48, 53), (37, 80), (53, 48), (512, 256),
                                        (512, 64), (7, 7), (1, 5), (5, 1)])
def test_tables_stay_inside_the_input_and_sum_to_one(n_in, n_out):
    start, count, w = aa_tables(n_in, n_out)
    assert start.dtype == np.int32 and count.dtype == np.int32 and w.dtype == np.float32
    assert start.shape == count.shape == (n_out,) and w.shape == (n_out, count.max())
    assert (start >= 0).all() and (count >= 1).all() and (count <= MAX_TAPS).all()
    assert (start + count <= n_in).all()
    np.testing.assert_allclose(w.astype(np.float64).sum(1), 1.0, rtol=0, atol=1e-6)
    assert (w >= 0).all()
    for i in range(n_out):
        assert not w[i, count[i]:].any()


def test_equal_sizes_are_the_identity():
    x = np.random.default_rng(3).uniform(-1, 1, (1, 2, 9, 13)).astype(np.float32)
    np.testing.assert_array_equal(apply_tables(apply_tables(x, 13, 3), 9, 2), x)


def test_ratio_above_eight_is_refused():
    aa_tables(64, 8)
    with pytest.raises(ValueError):
        aa_tables(64, 7)
    with pytest.raises(ValueError):
        aa_tables(0, 4)


def test_generate_pipeline_arguments():
    spec = importlib.util.spec_from_file_location("dcs_gen_args", os.path.join(ROOT, "ducosy-gan_amd", "generate.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    a = gen.get_args([])
    assert a.pipeline == "staged" and a.write_working is False
    a = gen.get_args(["--pipeline", "resident", "--write_working"])
    assert a.pipeline == "resident" and a.write_working is True
    assert callable(gen.generate_synthesis)
    with pytest.raises(SystemExit):
        gen.get_args(["--pipeline", "other"])
