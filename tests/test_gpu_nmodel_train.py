"""Training the normal-map U-Net on the GPU (csrc/unet_train.hip, modules/hip/unet_train.py,
modules/nmodel/trainer.py, train_nmodel.py): each new kernel alone against float64 on the CPU, the
whole step's gradients against the reference's float64 step (tests/golden/nmodel_train.npz) and
against the ATen recipe, running statistics, the optimizer plumbing, determinism, the way from a
step to inference, a falling loss, and the entry point end to end."""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, ROOT
from modules import nmodel
from modules.hip import ops
from modules.hip import unet as U
from modules.hip import unet_train as UT
from modules.nmodel import (FastTrainConfig, UNet3D, UNet3DLight, UNetTrainer, fold, forward_folded, load_model,
                            predict_volume_device, reference_step)
from test_cpu_nmodel_train import T, _write_patients, case_tensors, golden_gradient, rel_l2, seeded_train_model
from test_gpu_nmodel import _run, tree  # noqa: F401  (the generate.py tree of the inference tests)
from test_gpu_resident import _load_generate

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
E = 2.0 ** -24           # one float32 rounding, relative
BN_EPS = 1e-5


def _rand(seed, shape, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * (hi - lo) + lo


def _gamma_beta(seed, C):
    gamma = _rand(seed, (C,), 0.5, 1.5) * torch.where(torch.arange(C) % 3 == 1, -1.0, 1.0)
    return gamma, _rand(seed + 1, (C,), -0.3, 0.3)


def _stats64(y, gamma, beta):
    """(mean, var, invstd, scale, shift) of an NHWC tensor in float64."""
    y = y.double().reshape(-1, y.shape[-1])
    mean, var = y.mean(0), y.var(0, unbiased=False)
    invstd = 1.0 / torch.sqrt(var + BN_EPS)
    scale = gamma.double() * invstd
    return mean, var, invstd, scale, beta.double() - mean * scale


def _d(*ts):
    return [None if t is None else t.to(DEV).contiguous() for t in ts]


# ---------------------------------------------------------------------------------------
# each kernel alone
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(7, 5), (8, 8)])
def test_bn_stats(H, W):
    """Every output is a float64 result rounded once (2^-24); the bar is twice that, which also covers
    the float64 arithmetic.  Channel 3 has mean 1e3 and spread 1e-2: E[x^2] - mean^2 in float32
    would lose its variance entirely."""
    N, C = 2, 8
    y = _rand(1, (N, H, W, C), -2, 2)
    y[..., 3] = 1000.0 + _rand(2, (N, H, W), -0.01, 0.01)
    gamma, beta = _gamma_beta(3, C)
    rm, rv = _rand(4, (C,), -0.3, 0.3), _rand(5, (C,), 0.5, 1.5)
    mean, var, invstd, scale, shift = _stats64(y, gamma, beta)
    M = N * H * W
    want_rm = 0.9 * rm.double() + 0.1 * mean
    want_rv = 0.9 * rv.double() + 0.1 * var * M / (M - 1)
    drm, drv = _d(rm, rv)
    got = UT.bn_stats(*_d(y, gamma, beta), BN_EPS, 0.1, drm, drv, nrep=3)
    sc, sh, mu, istd = [t.cpu().double() for t in got]
    assert sc.shape == sh.shape == (3, C) and torch.equal(sc[0], sc[2]) and torch.equal(sh[0], sh[1])
    assert bool(((mu - mean).abs() <= 2 * E * mean.abs()).all())
    assert bool(((istd - invstd).abs() <= 2 * E * invstd).all()), ((istd - invstd).abs() / invstd).max()
    assert bool(((sc[0] - scale).abs() <= 2 * E * scale.abs()).all())
    assert bool(((sh[0] - shift).abs() <= 2 * E * (beta.abs().double() + (mean * scale).abs())).all())
    assert bool(((drm.cpu().double() - want_rm).abs() <= 2 * E * (rm.abs().double() + mean.abs())).all())
    assert bool(((drv.cpu().double() - want_rv).abs() <= 2 * E * want_rv).all())
    # a larger map: more than one block per reduction
    y2 = _rand(6, (2, 40, 36, 16), -2, 2)
    g2, b2 = _gamma_beta(7, 16)
    m2, _, i2, _, _ = _stats64(y2, g2, b2)
    _, _, mu2, is2 = UT.bn_stats(*_d(y2, g2, b2))
    assert bool(((mu2.cpu().double() - m2).abs() <= 2 * E * m2.abs() + 1e-12).all())
    assert bool(((is2.cpu().double() - i2).abs() <= 2 * E * i2).all())
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        UT.bn_stats(torch.zeros(1, 1, 1, 8, device=DEV), *_d(gamma, beta))


def _bn_case(seed, N, H, W, C, margin=1e-4):
    """y, gamma, beta and the float32 statistics the forward would hand the backward, with every
    pre-activation at least ``margin`` from 0 (a ReLU decision must not hang on a rounding)."""
    for s in range(seed, seed + 50):
        y = _rand(s, (N, H, W, C), -2, 2)
        gamma, beta = _gamma_beta(s + 100, C)
        mean, var, invstd, scale, shift = _stats64(y, gamma, beta)
        if float((y.double() * scale + shift).abs().min()) >= margin:
            return y, gamma, beta, [t.float() for t in (scale, shift, mean, invstd)]
    raise AssertionError("no seed with a margin")


def _bn_relu64(y, gamma, beta):
    """(a, leaves) of a = relu(BatchNorm_train(y)) in float64 with autograd, NHWC."""
    y64, g64, b64 = (t.double().clone().requires_grad_(True) for t in (y, gamma, beta))
    flat = y64.reshape(-1, y.shape[-1])
    xhat = (y64 - flat.mean(0)) / torch.sqrt(flat.var(0, unbiased=False) + BN_EPS)
    return F.relu(xhat * g64 + b64), (y64, g64, b64), xhat.detach()


def _check_bn_backward(got, leaves, xhat, g_abs, scale, M, label):
    """dbeta and dgamma are float64 sums of float32 terms rounded once: g is exact, xhat carries 2
    roundings and those of mean and invstd (4 E of (|y| + |mean|) invstd, bounded here by 4 E (|xhat| +
    2 |mean| invstd)).  dy = scale * (g - dbeta / M - xhat * dgamma / M) is 8 roundings on the sum of
    its terms' magnitudes, and inherits the errors of dbeta, dgamma and xhat: 16 E of that sum."""
    dy, dgamma, dbeta = got[:3]
    y64, g64, b64 = leaves
    want_dy, want_dg, want_db = y64.grad, g64.grad, b64.grad
    db_bound = 2 * E * g_abs.sum((0, 1, 2)) + 1e-30
    xh_mag = xhat.abs() + 2.0
    dg_bound = 6 * E * (g_abs * xh_mag).sum((0, 1, 2)) + 1e-30
    err_db = (dbeta.cpu().double() - want_db).abs()
    err_dg = (dgamma.cpu().double() - want_dg).abs()
    assert bool((err_db <= db_bound).all()), (label, "dbeta", float((err_db / db_bound).max()))
    assert bool((err_dg <= dg_bound).all()), (label, "dgamma", float((err_dg / dg_bound).max()))
    mag = scale.abs().double() * (g_abs + want_db.abs() / M + xh_mag * want_dg.abs() / M)
    err = (dy.cpu().double() - want_dy).abs()
    assert bool((err <= 16 * E * mag + 1e-30).all()), (label, "dy", float((err / (16 * E * mag + 1e-30)).max()))


def test_bn_relu_backward_form_a_channel_slice():
    N, H, W, C = 2, 7, 5, 8
    y, gamma, beta, st = _bn_case(10, N, H, W, C)
    wide = _rand(11, (N, H, W, 16))
    da = wide[..., 4:4 + C]
    a, leaves, xhat = _bn_relu64(y, gamma, beta)
    (a * da.double()).sum().backward()
    got = UT.bn_relu_backward(*_d(y, *st), da=wide.to(DEV), channel_offset=4)
    g_abs = (da.double() * (a > 0)).abs()
    _check_bn_backward(got, leaves, xhat, g_abs, st[0], N * H * W, "form A")
    # a dense da is the slice at offset 0 of itself: same bits
    dense = UT.bn_relu_backward(*_d(y, *st), da=da.contiguous().to(DEV))
    assert all(torch.equal(p, q) for p, q in zip(got, dense))


def test_bn_relu_backward_form_b_pool_routing():
    """Odd H and W; window (0,0) holds two equal positive maxima per channel (the first takes the
    pooled gradient), window (0,1) is all zero after the ReLU (nothing passes)."""
    N, H, W, C = 2, 7, 5, 8
    for seed in range(20, 70):
        y = _rand(seed, (N, H, W, C), -2, 2)
        gamma, beta = _gamma_beta(seed + 100, C)
        sg = torch.sign(gamma)
        y[0, 0, 0] = y[0, 0, 1] = 5.0 * sg          # equal maxima at window positions 0 and 1
        y[0, 1, 0], y[0, 1, 1] = 1.0 * sg, -1.0 * sg
        y[0, 0:2, 2:4] = -5.0 * sg                   # pre-activation < 0 at all four
        mean, var, invstd, scale, shift = _stats64(y, gamma, beta)
        if float((y.double() * scale + shift).abs().min()) >= 1e-4:
            break
    st = [t.float() for t in (scale, shift, mean, invstd)]
    wide, dpool = _rand(12, (N, H, W, 12)), _rand(13, (N, H // 2, W // 2, C))
    da = wide[..., 4:]
    a, leaves, xhat = _bn_relu64(y, gamma, beta)
    ad = a.detach()
    assert bool((ad[0, 0, 0] == ad[0, 0, 1]).all()) and bool((ad[0, 0, 0] > ad[0, 1, 0]).all()) and float(ad[0, 0:2, 2:4].max()) == 0
    pooled = F.max_pool2d(a.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    ((a * da.double()).sum() + (pooled * dpool.double()).sum()).backward()
    got = UT.bn_relu_backward(*_d(y, *st), da=wide.to(DEV), channel_offset=4, dpool=dpool.to(DEV))
    # the gradient reaching a, as torch routes it (first maximum on ties): for the bound's magnitudes
    a2 = a.detach().clone().requires_grad_(True)
    (F.max_pool2d(a2.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1) * dpool.double()).sum().backward()
    routed = a2.grad
    assert bool((routed[0, 0, 0] == dpool[0, 0, 0].double()).all()) and float(routed[0, 0, 1].abs().max()) == 0
    g_abs = ((da.double() + routed) * (a.detach() > 0)).abs()
    _check_bn_backward(got, leaves, xhat, g_abs, st[0], N * H * W, "form B")
    # exactly: form B is form A of da + the routed gradient wherever that sum is exact; make it so
    # with a da of zeros, so that form A's da is the routed gradient itself
    zero = torch.zeros(N, H, W, C)
    b = UT.bn_relu_backward(*_d(y, *st), da=zero.to(DEV), dpool=dpool.to(DEV))
    a_ = UT.bn_relu_backward(*_d(y, *st), da=routed.float().to(DEV))
    assert all(torch.equal(p, q) for p, q in zip(a_, b))
    # the odd last row and column are in no window: with a zero da they get only the mean terms
    M = N * H * W
    xh32 = (y - st[2]) * st[3]
    mean_terms = (st[0] * (-(b[2].cpu() / M) - xh32 * (b[1].cpu() / M)))
    assert float((b[0].cpu()[:, 6] - mean_terms[:, 6]).abs().max()) <= 8 * E * float(mean_terms.abs().max())
    assert float((b[0].cpu()[:, :, 4] - mean_terms[:, :, 4]).abs().max()) <= 8 * E * float(mean_terms.abs().max())


@pytest.mark.parametrize("C", [8, 16, 32])
def test_bn_relu_backward_form_c_output_projection(C):
    N, H, W = 2, 7, 5
    y, gamma, beta, st = _bn_case(30 + C, N, H, W, C)
    wout, dout = _rand(31, (C,)), _rand(32, (N, H, W), -1e-2, 1e-2)
    a, leaves, xhat = _bn_relu64(y, gamma, beta)
    w64 = wout.double().clone().requires_grad_(True)
    b64 = torch.zeros(1, dtype=torch.float64, requires_grad=True)
    ((a @ w64 + b64) * dout.double()).sum().backward()
    got = UT.bn_relu_backward(*_d(y, *st), dout=dout.to(DEV), wout=wout.to(DEV))
    da = dout.double()[..., None] * wout.double()
    # da = dout * wout is one more rounding on g: within the 16 E of dy and the sums' slack
    _check_bn_backward(got, leaves, xhat, (da * (a.detach() > 0)).abs() * (1 + 1e-6), st[0], N * H * W, f"form C {C}")
    dwout, dbias = got[3].cpu().double(), got[4].cpu().double()
    # a in float32: 2 roundings on |y scale| + |shift| and those of scale and shift; one final rounding
    a_mag = (y.double() * st[0].double()).abs() + st[1].abs().double()
    bound = 4 * E * (dout.abs().double()[..., None] * a_mag).sum((0, 1, 2)) + E * w64.grad.abs()
    assert bool(((dwout - w64.grad).abs() <= bound).all()), float(((dwout - w64.grad).abs() / bound).max())
    assert abs(float(dbias) - float(b64.grad)) <= 2 * E * float(dout.abs().sum())


@pytest.mark.parametrize("C", [8, 32])
def test_l1_out(C):
    P = 777
    y, gamma, beta, st = _bn_case(40 + C, 1, 1, P, C)
    scale, shift = st[0], st[1]
    wout, bias, target = _rand(41, (C,)), torch.tensor([0.125]), _rand(42, (P,))
    a = F.relu(y.reshape(P, C).double() * scale.double() + shift.double())
    o64 = a @ wout.double() + 0.125
    # C products and sums, the affine map's two steps, the bias: each 2^-24 of the running magnitude
    bound = (C + 4) * E * (a.abs() @ wout.abs().double() + 0.125)
    dy, ds, dsh, dw, db, dt = _d(y.reshape(P, C), scale, shift, wout, bias, target)
    loss, dout, o = UT.l1_out(dy, ds, dsh, dw, db, dt, gscale=0.5, want_o=True)
    assert bool(((o.cpu().double() - o64).abs() <= bound).all())
    want_loss = 0.5 * float((o64 - target.double()).abs().mean())
    assert abs(float(loss) - want_loss) <= 0.5 * float(bound.mean()) + 2 * E * want_loss
    k = np.float32(0.5 / P)
    sure = (o64 - target.double()).abs() > bound + E
    assert int(sure.sum()) > P // 2
    assert torch.equal(dout.cpu()[sure], (torch.sign(o64 - target.double())[sure] * float(k)).float())
    assert set(np.unique(dout.cpu().numpy())) <= {-k, np.float32(0), k}
    # a pixel where the output IS the target: sign(0) = 0, as torch
    dt2 = dt.clone()
    dt2[5] = o[5]
    loss2, dout2, _ = UT.l1_out(dy, ds, dsh, dw, db, dt2, gscale=0.5)
    assert float(dout2[5]) == 0.0 and torch.equal(torch.cat([dout2[:5], dout2[6:]]), torch.cat([dout[:5], dout[6:]]))
    assert float(loss2) <= float(loss)


@pytest.mark.parametrize("h,w,Ho,Wo", [(3, 2, 7, 5), (2, 3, 5, 7), (1, 4, 2, 8), (4, 1, 8, 2), (1, 1, 3, 3)])
def test_upsample2_pad_backward(h, w, Ho, Wo):
    N, C = 2, 8
    wide = _rand(50, (N, Ho, Wo, 4 + C))
    g = wide[..., 4:]

    def up(x):   # NHWC in, NHWC out, ATen
        u = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True)
        dh, dw = Ho - u.shape[2], Wo - u.shape[3]
        return F.pad(u, [dw // 2, dw - dw // 2, dh // 2, dh - dh // 2]).permute(0, 2, 3, 1)

    x = _rand(51, (N, h, w, C)).double().requires_grad_(True)
    (up(x) * g.double()).sum().backward()
    xa = torch.zeros(N, h, w, C, dtype=torch.float64, requires_grad=True)
    (up(xa) * g.double().abs()).sum().backward()
    got = UT.upsample2_pad_backward(wide.to(DEV), (h, w), C, channel_offset=4)
    assert got.shape == (N, h, w, C)
    # at most 16 outputs reach a source pixel.  Each term: the weights' product, the product with g and
    # the addition, 3 E on the adjoint of |g|; and each 1-D weight is off by up to 2 E of its source
    # coordinate (the float32 ratio and its product with the index, both below max(h, w)), an absolute
    # error that weighs on |g| whatever the weight: 16 taps x 2 axes x 2 E max(h, w) max |g|
    bound = 3 * E * xa.grad + 64 * E * max(h, w) * float(g.abs().max())
    err = (got.cpu().double() - x.grad).abs()
    assert bool((err <= bound).all()), float((err / bound).max())
    # the adjoint of the device's own forward
    x32 = _rand(52, (N, h, w, C))
    fwd = U.upsample2_pad(x32.to(DEV), (Ho, Wo)).cpu().double()
    lhs, rhs = float((fwd * g.double()).sum()), float((x32.double() * got.cpu().double()).sum())
    scale = float((fwd.abs() * g.double().abs()).sum())
    assert abs(lhs - rhs) <= 1e-5 * scale, (lhs, rhs)
    if h == 1 and w == 1:   # both outputs per axis are that pixel: the gradient is the 2x2 sum
        want = g[:, 0:2, 0:2].double().sum((1, 2))
        assert float((got.cpu().double()[:, 0, 0] - want).abs().max()) <= 4 * E * float(g.abs().sum((1, 2)).max())


@pytest.mark.parametrize("n,amp,clip", [(1001, 1e-3, 1.0), (1001, 1.0, 1.0), (300001, 1.0, 1.0), (5000, 1.0, 0.0)])
def test_sumsq_and_clip_coefficient(n, amp, clip):
    g = _rand(60, (n,), -amp, amp)
    norm = float(g.double().norm())
    out = UT.sumsq_clip(g.to(DEV), clip).cpu().double()
    # float64 sum of exact squares, one square root, one rounding; the coefficient: 3 more
    assert abs(float(out[0]) - norm) <= 2 * E * norm
    want = min(1.0, clip / (norm + 1e-6)) if clip > 0 else 1.0
    assert (want < 1.0) == (clip > 0 and norm > clip)
    assert abs(float(out[1]) - want) <= 5 * E * want
    if want == 1.0:
        assert float(out[1]) == 1.0


# ---------------------------------------------------------------------------------------
# the whole step
# ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "nmodel_train.npz"))


def _device_gradients(model, x, t, mode=None):
    """{name: numpy gradient (trained view)} and the loss of one micro-batch on a fresh device copy."""
    import copy
    m = copy.deepcopy(model).float().to(DEV)
    state = UT.TrainState(m)
    before = ops.get_mma()
    try:
        if mode:
            ops.set_mma(mode)
        loss = state.accumulate(x.float().to(DEV), t.float().to(DEV))
    finally:
        ops.set_mma(before)
    return {k: v.cpu().numpy().astype(np.float64).reshape(-1) for k, v in state.named_gradients().items()}, \
        float(loss), m, state


def _ratios(got, want_of, delta32, names):
    out = {}
    for i, k in enumerate(names):
        want, g = want_of(k, got[k])
        err = rel_l2(g, want)   # (a sum of +-2^-k terms can be exact in float32 too: delta32 == 0 asks for 0)
        out[k] = 0.0 if err == 0.0 else (err / float(delta32[i]) if delta32[i] > 0 else float("inf"))
    return out


def _group(name):
    return "bn" if (".1." in name or ".4." in name) else ("out" if name.startswith("outc") else "conv")


# Bars per parameter group, in units of the case's own delta32 (the reference's float32 step against
# its float64 step, per parameter).  The issue's bar is 4.
BAR = {"conv": 4.0, "bn": 4.0, "out": 4.0}


def _report_and_check(label, ratios, ratios16=None):
    worst = {}
    for k, r in ratios.items():
        g = _group(k)
        if r > worst.get(g, (0, ""))[0]:
            worst[g] = (r, k)
    print(f"{label}: worst gradient error / delta32 per group: "
          + ", ".join(f"{g} {r:.2f} ({k})" for g, (r, k) in sorted(worst.items()))
          + (f"; f16 operand mode worst {max(ratios16.values()):.1f} (no bar)" if ratios16 else ""))
    bad = {k: round(r, 2) for k, r in ratios.items() if r > BAR[_group(k)]}
    assert not bad, f"{label}: above the bar {BAR}: {bad}"


@pytest.mark.parametrize("case", sorted(T.CASES))
def test_step_gradients_against_the_reference_float64(golden, case):
    """Per parameter: relative L2 error <= 4 x that parameter's delta32.  Measured: DESIGN.md §3."""
    assert ops.get_mma() == "f16x3"
    print(f"case {case}: margins (|BN out|, pool gap, |o - t|) {golden[f'{case}:margins'].tolist()}")
    model = seeded_train_model(case)
    x, t = case_tensors(golden, case)
    names = [str(k) for k in golden[f"{case}:names"]]
    want_of = lambda k, g: golden_gradient(golden, case, k, g)
    got, loss, m, _ = _device_gradients(model, x, t)
    assert abs(loss - float(golden[f"{case}:loss"])) <= 1e-5 * float(golden[f"{case}:loss"])
    got16, _, _, _ = _device_gradients(model, x, t, "f16")
    _report_and_check(f"case {case}", _ratios(got, want_of, golden[f"{case}:delta32"], names),
                      _ratios(got16, want_of, golden[f"{case}:delta32"], names))
    # running statistics after the step, and the step counter
    for k, b in m.named_buffers():
        if k.endswith("num_batches_tracked"):
            assert int(b) == 101
        else:
            want = golden[f"{case}:buf:{k}"]
            assert np.abs(b.cpu().numpy() - want).max() <= 1e-5 * np.abs(want).max(), k


def _random_model(cls, base, seed):
    torch.manual_seed(seed)
    model = cls(base_channels=base)
    for mod in model.modules():
        if isinstance(mod, torch.nn.BatchNorm3d):
            mod.weight.data.uniform_(0.5, 1.5).mul_(torch.where(torch.rand(mod.weight.shape) < 0.3, -1.0, 1.0))
            mod.bias.data.uniform_(-0.3, 0.3)
        elif isinstance(mod, torch.nn.Conv3d) and mod.kernel_size == (3, 3, 3):
            mod.weight.data.normal_(0, (2.0 / (9 * mod.in_channels)) ** 0.5)
    return model


# UNet3D at 32x32: one 16x16 slice leaves ONE value per channel below four pools, which BatchNorm
# refuses in training mode (test_unsupported_configurations_raise); 32x32 leaves 2x2, as 16x16 does
# below UNet3DLight's three.
@pytest.mark.parametrize("cls,base,hw", [(UNet3DLight, 16, 16), (UNet3D, 32, 32)])
def test_step_gradients_at_the_default_widths(cls, base, hw):
    """UNet3DLight base 16 and UNet3D base 32 (reaching the 256 -> 256 convolutions), one slice, against
    the ATen recipe in float64; delta32 is the same recipe in float32 on the CPU.  The input's seed
    advances until no ReLU, pool or sign decision lies within 1e-5 of a tie, as the fixture's does."""
    import copy
    assert ops.get_mma() == "f16x3"
    model = _random_model(cls, base, 5)
    for seed in range(70, 120):
        x, t = _rand(seed, (1, hw, hw)).numpy(), _rand(seed + 1000, (1, hw, hw)).numpy()
        _, g64, _, margins = T.run_step(copy.deepcopy(model), x, t, torch.float64, hooks=True)
        if min(margins.values()) >= T.MARGIN:
            break
    print(f"{cls.__name__} base {base}: input seed {seed}, margins {margins}")
    _, g32, _, _ = T.run_step(copy.deepcopy(model), x, t, torch.float32)
    names = list(g64)
    flat = lambda k, g: T.trained_view(k, g).contiguous().reshape(-1).double().numpy()
    delta32 = [rel_l2(flat(k, g32[k]), flat(k, g64[k])) for k in names]
    xt, tt = torch.from_numpy(x)[:, None, None], torch.from_numpy(t)[:, None, None]
    got, _, _, _ = _device_gradients(model, xt, tt)
    got16, _, _, _ = _device_gradients(model, xt, tt, "f16")
    want_of = lambda k, g: (flat(k, g64[k]), g)
    _report_and_check(f"{cls.__name__} base {base} {hw}x{hw}", _ratios(got, want_of, delta32, names),
                      _ratios(got16, want_of, delta32, names))


def _tiny(seed=0, N=2, hw=16):
    return _rand(seed, (N, 1, 1, hw, hw)).to(DEV), _rand(seed + 1, (N, 1, 1, hw, hw)).to(DEV)


def test_optimizer_plumbing_is_adam_on_the_devices_own_gradients():
    """Two optimizer steps of accumulation 2 with a clip that engages: the device parameters equal
    torch's Adam applied on the CPU to the gradients the device accumulated (1e-6 relative), which
    holds accumulate, clip and Adam apart from Adam's sign sensitivity to near-zero gradients."""
    model = _random_model(UNet3DLight, 8, 1).to(DEV)
    state = UT.TrainState(model)
    p = state.params.cpu().clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=1e-3)
    clip, coefs = 0.05, []
    for s in range(2):
        for i in range(2):
            state.accumulate(*_tiny(10 * s + 2 * i), gscale=0.5)
        g = state.acc.cpu().clone()
        norm = float(g.double().norm())
        coef = min(1.0, clip / (norm + 1e-6))
        coefs.append(coef)
        p.grad = g * np.float32(coef)
        opt.step()
        nc = state.step(1e-3, clip).cpu()
        assert abs(float(nc[0]) - norm) <= 2 * E * norm and abs(float(nc[1]) - coef) <= 5 * E
        assert float(state.acc.abs().max()) == 0.0 and state.micro == 0
        got = state.params.cpu()
        # 1e-6 relative to the parameters' scale.  (Not per element: dcs_adam_step forms 1 - beta in
        # float32, 1.3e-5 off torch's double for beta2, which moves an early update of about lr by 6e-6
        # of itself, more than 1e-6 of a parameter that is itself below lr.)
        want = p.detach()
        assert float((got - want).abs().max()) <= 1e-6 * float(want.abs().max())
        assert float((got - want).double().norm()) <= 1e-6 * float(want.double().norm())
    assert max(coefs) < 1.0
    # the module holds the stepped values: centre taps written back, the other taps untouched
    l = state.enc[1][0]
    assert torch.equal(l.conv3d.weight[:, :, 1], l.w) and l.bn.weight.data_ptr() == l.gamma.data_ptr()
    assert torch.equal(model.outc.conv.weight.reshape(-1), state.wout)
    fresh = _random_model(UNet3DLight, 8, 1)
    w0 = fresh.down1.maxpool_conv[1].double_conv[0].weight
    assert torch.equal(l.conv3d.weight[:, :, 0].cpu(), w0[:, :, 0]) and not torch.equal(l.conv3d.weight[:, :, 1].cpu(), w0[:, :, 1])


def test_three_steps_are_bit_reproducible():
    def run():
        model = _random_model(UNet3DLight, 8, 2).to(DEV)
        state = UT.TrainState(model)
        losses = []
        for s in range(3):
            losses.append(state.accumulate(*_tiny(20 + 2 * s, hw=20)))
            state.step(1e-3, 0.05)
        return state.params.clone(), torch.cat(losses), [b.clone() for b in model.buffers()]

    a, b = run(), run()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(p, q) for p, q in zip(a[2], b[2]))


def test_a_trained_model_reaches_inference():
    """The step writes through raw pointers, which bump no version counter: the cached inference plan
    has to go.  After one step predict_volume_device answers with the updated weights and running
    statistics: it equals the updated module's folded eval forward within the forward test's bar (4 x
    the float32 spread of that forward)."""
    model = _random_model(UNet3DLight, 8, 3).to(DEV).eval()
    hu = torch.from_numpy(np.random.default_rng(1).uniform(-1100, 1500, (2, 16, 16)).astype(np.float32)).to(DEV)
    before = predict_volume_device(model, hu)
    assert getattr(model, "_dcs_unet_plan", None) is not None
    state = UT.TrainState(model)
    model.train()
    state.accumulate(*_tiny(30))
    state.step(1e-2, 1.0)
    model.eval()
    after = predict_volume_device(model, hu)
    assert not torch.equal(after, before)
    import copy
    cpu = copy.deepcopy(model).cpu()
    x = torch.from_numpy(nmodel.normalize_hu(hu.cpu().numpy()))[:, None]
    with torch.no_grad():
        y32 = forward_folded(fold(cpu, torch.float32), x)[:, 0].double()
        y64 = forward_folded(fold(cpu.double(), torch.float64), x.double())[:, 0]
    bar = 4.0 * float((y32 - y64).abs().max())
    err = float((after.cpu().double() / 2000.0 - 1.0 - y64).abs().max())
    print(f"after one step: max error of the eval forward {err:.3e} (bar {bar:.3e}); moved by "
          f"{float((after - before).abs().max()):.3e} difference-map units")
    assert err <= bar


def test_the_loss_falls():
    """20 optimizer steps on one fixed 2x16x16 batch at lr 1e-3 (the recipe in float64 on the CPU falls
    monotonically at this size); the first loss is the oracle's."""
    import copy
    model = _random_model(UNet3DLight, 8, 4)
    x, t = _tiny(40)
    want = float(reference_step(copy.deepcopy(model).double(), x.cpu().double(), t.cpu().double()))
    cfg = FastTrainConfig(make_dirs=False)
    cfg.gradient_accumulation_steps, cfg.learning_rate, cfg.use_mixed_precision = 1, 1e-3, False
    trainer = UNetTrainer(model, cfg, device=DEV)
    losses = torch.stack([trainer.train_step(x, t) for _ in range(20)]).cpu().tolist()
    print(f"loss over 20 steps: {losses[0]:.4f} -> {losses[-1]:.4f} (oracle's first {want:.4f})")
    assert abs(losses[0] - want) <= 1e-5 * want
    assert losses[-1] < losses[0]


def _load_train_nmodel():
    spec = importlib.util.spec_from_file_location("dcs_train_nmodel", os.path.join(ROOT, "ducosy-gan_amd", "train_nmodel.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_train_nmodel_end_to_end(tmp_path, tree, capsys):  # noqa: F811
    _write_patients(tmp_path / "data", 3)
    tn = _load_train_nmodel()
    base = ["--model_type", "light", "--base_channels", "8", "--data_dir", str(tmp_path / "data"), "--output_dir",
            str(tmp_path / "out"), "--patch_size", "1", "16", "16", "--patches_per_volume", "4", "--num_workers", "0",
            "--gradient_accumulation_steps", "2", "--learning_rate", "1e-3", "--save_interval", "1"]
    hist = tn.main(base + ["--num_epochs", "2"])
    assert len(hist["train"]) == 2 and all(np.isfinite(hist["train"] + hist["val"]))
    ck = tmp_path / "out" / "checkpoints"
    for name in ("latest.pth", "best.pth", "epoch_1.pth", "epoch_2.pth"):
        assert (ck / name).is_file(), name
    assert torch.load(ck / "latest.pth", weights_only=True)["epoch"] == 2
    hist = tn.main(base + ["--num_epochs", "3", "--resume"])
    assert len(hist["train"]) == 1 and "at epoch 2" in capsys.readouterr().out
    ckpt = torch.load(ck / "latest.pth", weights_only=True)
    assert ckpt["epoch"] == 3 and ckpt["optimizer_state_dict"]["step"] == 3 * 4
    model, cfg = load_model(str(ck / "best.pth"), DEV)
    assert type(model) is UNet3DLight and cfg.base_channels == 8
    # generate.py takes the trained checkpoint
    root, gen_base, _ = tree
    gen = _load_generate()
    out, work = _run(gen, root, gen_base, "trained", ["--apply_diffmap", "--nmodel_path", str(ck / "best.pth"), "--save_diff"], True)
    diff = np.load(work / "diff.npy")
    assert diff.shape == (5, 64, 64) and np.isfinite(diff).all() and len(os.listdir(out)) == 5


def test_unsupported_configurations_raise():
    for bad in (UNet3DLight(trilinear=False, base_channels=8), UNet3DLight(n_channels=2, base_channels=8),
                UNet3DLight(n_classes=2, base_channels=8)):
        with pytest.raises(ValueError):
            UT.TrainState(bad.to(DEV))
    with pytest.raises(RuntimeError):
        UT.TrainState(UNet3DLight(base_channels=8))                         # a host model: no CPU fallback
    state = UT.TrainState(UNet3DLight(base_channels=8).to(DEV))
    z = lambda *s: torch.zeros(*s, device=DEV)
    with pytest.raises(ValueError):
        state.accumulate(z(1, 1, 2, 16, 16), z(1, 1, 2, 16, 16))             # depth 2
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        state.accumulate(z(1, 1, 1, 8, 8), z(1, 1, 1, 8, 8))                 # one value per channel at the bottom
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        UT.TrainState(UNet3D(base_channels=8).to(DEV)).accumulate(z(1, 1, 1, 16, 16), z(1, 1, 1, 16, 16))
    with pytest.raises(ValueError):
        state.accumulate(z(1, 1, 1, 7, 16), z(1, 1, 1, 7, 16))               # 7 rows do not survive three pools
    with pytest.raises(RuntimeError):
        state.accumulate(torch.zeros(2, 1, 1, 16, 16), torch.zeros(2, 1, 1, 16, 16))
    cfg = FastTrainConfig(make_dirs=False)
    cfg.ssim_weight = 0.5
    with pytest.raises(ValueError):
        UNetTrainer(UNet3DLight(base_channels=8), cfg, device=DEV)
    assert bool(torch.isfinite(state.accumulate(*_tiny(50, N=2, hw=8))).all())   # two slices of 8x8: fine
