"""Kernels of csrc/slices.hip through modules/hip/slices.py: the antialiased and nearest resizes
against ATen on the host, and the fused output -> stored value -> HU-range merge against
inference.stored_from_output + inference.synthesize per slice."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from modules.hip import lib
from modules.hip import slices as S
from modules.inference import hu_from_stored, stored_from_output, synthesize

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

SHAPES = [((96, 96), (64, 64)), ((64, 64), (96, 96)), ((80, 48), (37, 53)), ((37, 53), (80, 48))]
IDS = ["96to64", "64to96", "80x48to37x53", "37x53to80x48"]
SOFT, LUNG = (-150, 250), (-1000, -150)


def _uniform(shape, seed=11):
    return np.random.default_rng(seed).uniform(-1, 1, shape).astype(np.float32)


@pytest.mark.parametrize("nc", [(2, 1), (1, 2)], ids=["2x1", "1x2"])
@pytest.mark.parametrize("src,dst", SHAPES, ids=IDS)
def test_resize_aa_matches_cpu_interpolate(src, dst, nc):
    x = _uniform(nc + src)
    want = F.interpolate(torch.from_numpy(x), size=dst, mode="bilinear", align_corners=False, antialias=True).numpy()
    got = S.resize_aa(torch.from_numpy(x).to(DEV), dst).cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float32
    print("max abs difference", float(np.abs(got - want).max()))
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-6)


def test_resize_aa_one_axis_and_equal_sizes():
    x = torch.from_numpy(_uniform((2, 1, 40, 52), 5)).to(DEV)
    assert S.resize_aa(x, (40, 52)) is x
    assert S.resize_nearest(x, (40, 52)) is x
    for dst in ((40, 33), (25, 52)):   # one pass only, no intermediate buffer
        want = F.interpolate(x.cpu(), size=dst, mode="bilinear", align_corners=False, antialias=True).numpy()
        np.testing.assert_allclose(S.resize_aa(x, dst).cpu().numpy(), want, rtol=0, atol=1e-6)


def test_resize_aa_refuses_a_ratio_above_eight():
    x = torch.zeros(1, 1, 64, 64, device=DEV)
    assert S.resize_aa(x, 8).shape == (1, 1, 8, 8)
    with pytest.raises(ValueError):
        S.resize_aa(x, 7)
    # the entry point itself refuses it before any launch
    o, t = torch.zeros(1, 1, 7, 7, device=DEV), torch.zeros(1, 1, 64, 7, device=DEV)
    i32, w = torch.zeros(7, dtype=torch.int32, device=DEV), torch.zeros(7, 18, device=DEV)
    with pytest.raises(lib.HipLibraryError):
        lib.call("dcs_resize_aa", S._p(x), S._p(o), S._p(t), 1, 64, 64, 7, 7, S._p(i32), S._p(i32), S._p(w), 18,
                 S._p(i32), S._p(i32), S._p(w), 18, S._stream())
    with pytest.raises(lib.HipLibraryError):   # both sizes equal: nothing to resize
        lib.call("dcs_resize_aa", S._p(x), S._p(o), None, 1, 64, 64, 64, 64, None, None, None, 0, None, None, None,
                 0, S._stream())
    torch.cuda.synchronize()


@pytest.mark.parametrize("nc", [(2, 1), (1, 2)], ids=["2x1", "1x2"])
@pytest.mark.parametrize("src,dst", SHAPES + [((100, 100), (128, 128))], ids=IDS + ["100to128"])
def test_resize_nearest_is_exact(src, dst, nc):
    x = _uniform(nc + src, 7)
    want = F.interpolate(torch.from_numpy(x), size=dst, mode="nearest").numpy()
    got = S.resize_nearest(torch.from_numpy(x).to(DEV), dst).cpu().numpy()
    np.testing.assert_array_equal(got, want)


def _merge_case(dtype, size):
    """(raw, slopes, intercepts, y_soft, y_lung): D = 3 slices with raw HU on every range bound and
    on -150 where the ranges touch, and outputs with exact -1, 0, +1."""
    rng = np.random.default_rng(17)
    D = 3
    if dtype == np.int16:
        slopes, inters = [1.0, 0.5, 1.0], [0.0, -1024.0, -1024.0]
        raw = rng.integers(-1100, 1500, (D, size, size)).astype(np.int16)
        raw[1] = rng.integers(0, 4000, (size, size))
        raw[2] = rng.integers(0, 3000, (size, size))
    else:
        slopes, inters = [1.0, 1.0, 1.0], [-1024.0, -1024.0, -1024.0]
        raw = rng.integers(0, 3000, (D, size, size)).astype(np.uint16)
    for k in range(D):
        stored = [(hu - inters[k]) / slopes[k] for hu in (-1000, -150, 250)]
        vals = [int(s) + o for s in stored for o in (-1, 0, 1) if int(s) + o >= (0 if dtype == np.uint16 else -32768)]
        raw[k].reshape(-1)[5:5 + len(vals)] = vals
    ys, yl = _uniform((D, size, size), 23), _uniform((D, size, size), 29)
    for y in (ys, yl):
        for k in range(D):
            y[k].reshape(-1)[:3] = (-1.0, 0.0, 1.0)
            y[k].reshape(-1)[-3:] = (1.0, 0.0, -1.0)
    return raw, slopes, inters, ys, yl


def _host(raw, slopes, inters, ys, yl):
    so = np.stack([stored_from_output(ys[k], SOFT[0], SOFT[1], slopes[k], inters[k], raw.dtype) for k in range(len(raw))])
    lo = np.stack([stored_from_output(yl[k], LUNG[0], LUNG[1], slopes[k], inters[k], raw.dtype) for k in range(len(raw))])
    me = np.stack([synthesize(raw[k], hu_from_stored(raw[k], slopes[k], inters[k]), so[k], lo[k], SOFT, LUNG)
                   for k in range(len(raw))])
    return so, lo, me


# 41: H*W and W are no multiples of 4, the element kernel; 40 and 64: one 16-byte vector per thread
@pytest.fixture(scope="module", params=[(np.int16, 41), (np.int16, 40), (np.int16, 64), (np.uint16, 41),
                                        (np.uint16, 40), (np.uint16, 64)],
                ids=["int16-41", "int16-40", "int16-64", "uint16-41", "uint16-40", "uint16-64"])
def merge_case(request):
    dtype, size = request.param
    case = _merge_case(dtype, size)
    return case + _host(*case)


def _device_args(raw, slopes, inters, ys, yl):
    up = lambda a: torch.from_numpy(a).to(DEV)
    return (up(np.ascontiguousarray(raw).view(np.int16)), up(np.array(slopes, np.float32)),
            up(np.array(inters, np.float32)), up(ys), up(yl))


def test_translate_merge_matches_host(merge_case):
    raw, slopes, inters, ys, yl, so, lo, me = merge_case
    # the case holds what it is meant to: bounds, the touching point, truncation != floor
    hu0 = hu_from_stored(raw[0], slopes[0], inters[0])
    for b in (-1000, -150, 250):
        assert (hu0 == b).any()
    touch = np.stack([hu_from_stored(raw[k], slopes[k], inters[k]) for k in range(3)]) == -150
    assert touch.any() and np.array_equal(me[touch], lo[touch])
    assert (me == raw).any() and (me == so).any() and (me == lo).any()
    if raw.dtype == np.int16:
        px = (((yl[0] + np.float32(1)) / np.float32(2)) * np.float32(850) + np.float32(-1000))
        assert ((px < 0) & (px != np.floor(px))).any()      # slope 1, intercept 0: px = hu
        assert (np.trunc(px) != np.floor(px)).any()
    else:
        assert so.min() >= 24 and lo.min() >= 24            # intercept -1024: no negative px to wrap
    args = _device_args(raw, slopes, inters, ys, yl)
    unsigned = raw.dtype == np.uint16
    got = S.translate_merge(*args, SOFT, LUNG, unsigned=unsigned, want_soft=True, want_lung=True,
                            want_merged=True, want_f32=True)
    host = lambda t: t.cpu().numpy().view(raw.dtype)
    assert np.array_equal(host(got[0]), so)
    assert np.array_equal(host(got[1]), lo)
    assert np.array_equal(host(got[2]), me)
    assert got[3].dtype == torch.float32 and np.array_equal(got[3].cpu().numpy(), me.astype(np.float32))


@pytest.mark.parametrize("which", [0, 1, 2, 3], ids=["soft", "lung", "merged", "f32"])
def test_translate_merge_single_outputs(merge_case, which):
    raw, slopes, inters, ys, yl, so, lo, me = merge_case
    flags = dict(want_soft=which == 0, want_lung=which == 1, want_merged=which == 2, want_f32=which == 3)
    got = S.translate_merge(*_device_args(raw, slopes, inters, ys, yl), SOFT, LUNG, unsigned=raw.dtype == np.uint16,
                            **flags)
    assert [g is not None for g in got] == [which == k for k in range(4)]
    if which == 3:
        assert np.array_equal(got[3].cpu().numpy(), me.astype(np.float32))
    else:
        assert np.array_equal(got[which].cpu().numpy().view(raw.dtype), (so, lo, me)[which])


def test_translate_merge_bad_calls():
    raw, slopes, inters, ys, yl = _merge_case(np.int16, 40)
    r, a, b, s, g = _device_args(raw, slopes, inters, ys, yl)
    with pytest.raises(ValueError):     # nothing requested
        S.translate_merge(r, a, b, s, g, SOFT, LUNG, want_f32=False)
    with pytest.raises(RuntimeError):   # host tensor
        S.translate_merge(r.cpu(), a, b, s, g, SOFT, LUNG)
    with pytest.raises(RuntimeError):
        S.translate_merge(r, a, b, s.cpu(), g, SOFT, LUNG)
    with pytest.raises(RuntimeError):   # wrong dtype
        S.translate_merge(r.float(), a, b, s, g, SOFT, LUNG)
    with pytest.raises(RuntimeError):
        S.translate_merge(r, a, b, s.double(), g, SOFT, LUNG)
    with pytest.raises(ValueError):     # shapes
        S.translate_merge(r, a, b, s[:2], g, SOFT, LUNG)
    with pytest.raises(ValueError):
        S.translate_merge(r, a[:2], b, s, g, SOFT, LUNG)
    with pytest.raises(lib.HipLibraryError):   # the entry point refuses a call with no output
        lib.call("dcs_vol_translate_merge", S._p(r), lib.VOL_I16, S._p(a), S._p(b), S._p(s), S._p(g), 3, 40, 40,
                 -150.0, 250.0, 400.0, -1000.0, -150.0, 850.0, None, None, None, None, S._stream())
    torch.cuda.synchronize()


@pytest.mark.parametrize("fn", [S.resize_aa, S.resize_nearest], ids=["aa", "nearest"])
def test_resize_bad_calls(fn):
    x = torch.zeros(1, 1, 8, 8)
    with pytest.raises(RuntimeError):   # host tensor
        fn(x, (4, 4))
    with pytest.raises(RuntimeError):   # wrong dtype
        fn(x.to(DEV).double(), (4, 4))
    with pytest.raises(ValueError):     # not [N,C,H,W]
        fn(x.to(DEV)[0], (4, 4))
    with pytest.raises(ValueError):
        fn(x.to(DEV), (0, 4))
