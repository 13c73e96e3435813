"""One training step of the normal-map U-Net on the device (csrc/unet_train.hip, dcs_unet_*; the 3x3
convolutions, their data and weight gradients on the rows pass through ConvGeom).

A sample is a depth-1 patch, so a micro-batch [N,1,1,H,W] runs as N slices of the folded 2-D
network (modules/nmodel/model.py) with two differences from inference: BatchNorm takes the batch
statistics over N*H*W values per channel, and only the centre depth tap of every Conv3d weight has
a gradient (the other two multiply zero padding), so the step trains the folded [Cout,Cin,3,3]
weights and writes them back into the centre tap.

``TrainState(model)`` keeps the parameters, their gradients and the Adam moments in flat device
buffers.  The module's BatchNorm weights and biases and its output convolution are re-pointed INTO
the parameter buffer (views), the 3-D convolution weights receive their centre tap after every
optimizer step, and the BatchNorm running statistics the kernels update are the module's own
buffers.  ``accumulate(x, target, gscale)`` adds the gradient of gscale * mean |model(x) - target|
to the accumulator; ``step(lr, clip)`` clips by the global L2 norm (clip_grad_norm_), applies Adam
and drops the module's cached inference plan.  Nothing in a step waits for the host.

Operand mode: the one of modules/hip/ops.py.  The forward convolutions run as in inference
(record-free modes); the gradient passes take the step's mode with their range records.

No CPU fallback: host tensors and unsupported models raise.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Tuple

import torch

from . import lib, ops
from . import unet as U
from .ops import Src, _p, _stream, workspace
from .unet import _Conv, _Geom, timed

ADAM_BETAS, ADAM_EPS = (0.9, 0.999), 1e-8   # torch.optim.Adam's defaults


def _pp(t: torch.Tensor, offset: int = 0):
    return ctypes.c_void_p(t.data_ptr() + 4 * offset)


# ---------------------------------------------------------------------------------------
# kernel wrappers
# ---------------------------------------------------------------------------------------
def _f32(t: torch.Tensor, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name}: device tensor required (no CPU fallback)")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise RuntimeError(f"{name}: contiguous float32 required")
    return t


def bn_stats(y: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5, momentum: float = 0.1,
             running_mean: Optional[torch.Tensor] = None, running_var: Optional[torch.Tensor] = None, nrep: int = 1):
    """Training-mode BatchNorm statistics of y [..., C] over all leading axes.  Returns (scale
    [nrep,C], shift [nrep,C], mean [C], invstd [C]) with scale = gamma * invstd, shift = beta - mean *
    scale; updates the running statistics in place (momentum, unbiased variance)."""
    y = _f32(y, "bn_stats")
    C = y.shape[-1]
    M = y.numel() // C
    if M < 2:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(y.shape)}")
    for t in (gamma, beta, running_mean, running_var):
        if t is not None and (_f32(t, "bn_stats").numel() != C):
            raise ValueError("bn_stats: one value per channel")
    dev = y.device
    scale, shift = torch.empty(nrep, C, device=dev), torch.empty(nrep, C, device=dev)
    mean, invstd = torch.empty(C, device=dev), torch.empty(C, device=dev)
    ws = workspace(lib.query("dcs_unet_bn_stats_workspace_size", M, C), dev)
    lib.call("dcs_unet_bn_stats", _p(y), M, C, _p(gamma), _p(beta), float(eps), float(momentum), nrep, _p(scale),
             _p(shift), _p(mean), _p(invstd), _p(running_mean), _p(running_var), _p(ws), ws.numel(), _stream())
    return scale, shift, mean, invstd


def bn_relu_backward(y, scale, shift, mean, invstd, da=None, channel_offset: int = 0, dpool=None, dout=None,
                     wout=None, dgamma=None, dbeta=None, dwout=None, dbias=None):
    """Backward of a = relu(y * scale + shift) under batch statistics; y [N,H,W,C].  The gradient of a:
    ``da`` [N,H,W,Cs] read at channels [channel_offset, channel_offset + C) (form A), plus ``dpool``
    [N,H/2,W/2,C] routed through the 2x2 max pool of a (form B), or ``dout`` [N,H,W] x ``wout`` [C] of
    the output projection (form C).  Returns (dy, dgamma, dbeta[, dwout, dbias]); the gradient
    tensors may be given (views of a flat buffer)."""
    y = _f32(y, "bn_relu_backward")
    N, H, W, C = y.shape
    dev = y.device
    for t in (scale, shift, mean, invstd):
        if _f32(t, "bn_relu_backward").numel() < C:
            raise ValueError("bn_relu_backward: one value per channel")
    cstride, da_ptr = 0, None
    if dout is not None:
        if da is not None or dpool is not None or wout is None:
            raise ValueError("bn_relu_backward: form C takes dout and wout alone")
        if _f32(dout, "bn_relu_backward").numel() != N * H * W or _f32(wout, "bn_relu_backward").numel() != C:
            raise ValueError("bn_relu_backward: dout per pixel, wout per channel")
        dwout = torch.empty(C, device=dev) if dwout is None else dwout
        dbias = torch.empty(1, device=dev) if dbias is None else dbias
    else:
        if da is None or _f32(da, "bn_relu_backward").dim() != 4 or tuple(da.shape[:3]) != (N, H, W):
            raise ValueError("bn_relu_backward: da must be [N,H,W,Cs]")
        cstride = da.shape[3]
        if channel_offset < 0 or channel_offset % 4 or channel_offset + C > cstride or cstride % 4:
            raise ValueError("bn_relu_backward: the channel slice must lie inside da at a multiple of 4")
        da_ptr = _pp(da, channel_offset)
        if dpool is not None:
            if H < 2 or W < 2 or tuple(_f32(dpool, "bn_relu_backward").shape) != (N, H // 2, W // 2, C):
                raise ValueError("bn_relu_backward: dpool must be [N,H/2,W/2,C]")
    dgamma = torch.empty(C, device=dev) if dgamma is None else dgamma
    dbeta = torch.empty(C, device=dev) if dbeta is None else dbeta
    dy = torch.empty_like(y)
    ws = workspace(lib.query("dcs_unet_bn_relu_backward_workspace_size", N, H, W, C), dev)
    args = (da_ptr, cstride, _p(dpool), _p(dout), _p(wout), _p(y), _p(scale), _p(shift), _p(mean), _p(invstd), N, H, W, C)
    lib.call("dcs_unet_bn_relu_backward_sums", *args, _p(dgamma), _p(dbeta), _p(dwout), _p(dbias), _p(ws), ws.numel(),
             _stream())
    lib.call("dcs_unet_bn_relu_backward_apply", *args, _p(dgamma), _p(dbeta), _p(dy), _stream())
    if dout is not None:
        return dy, dgamma, dbeta, dwout, dbias
    return dy, dgamma, dbeta


def l1_out(y, scale, shift, wout, bias, target, gscale: float = 1.0, want_o: bool = False):
    """The training tail: o = relu(y * scale + shift) . wout + bias per pixel of y [..., C], loss =
    gscale * mean |o - target|, dout = d loss / d o (sign(0) = 0).  Returns (loss [1], dout, o or None)."""
    y = _f32(y, "l1_out")
    C = y.shape[-1]
    P = y.numel() // C
    if _f32(target, "l1_out").numel() != P or _f32(wout, "l1_out").numel() != C or _f32(bias, "l1_out").numel() != 1:
        raise ValueError("l1_out: target per pixel, wout per channel, one bias")
    dev = y.device
    dout = torch.empty(y.shape[:-1], device=dev)
    o = torch.empty(y.shape[:-1], device=dev) if want_o else None
    loss = torch.empty(1, device=dev)
    ws = workspace(lib.query("dcs_unet_l1_out_workspace_size", P, C), dev)
    lib.call("dcs_unet_l1_out", _p(y), _p(_f32(scale, "l1_out")), _p(_f32(shift, "l1_out")), _p(wout), _p(bias),
             _p(target), P, C, float(gscale), _p(o), _p(dout), _p(loss), _p(ws), ws.numel(), _stream())
    return loss, dout, o


def upsample2_pad_backward(dcat: torch.Tensor, hw: Tuple[int, int], C: int, channel_offset: int = 0) -> torch.Tensor:
    """The adjoint of unet.upsample2_pad: the gradient [N,h,w,C] of its source from ``dcat``
    [N,Ho,Wo,Cs], read at channels [channel_offset, channel_offset + C)."""
    dcat = _f32(dcat, "upsample2_pad_backward")
    N, Ho, Wo, Cs = dcat.shape
    h, w = int(hw[0]), int(hw[1])
    if Ho < 2 * h or Wo < 2 * w or channel_offset < 0 or channel_offset % 4 or channel_offset + C > Cs or C % 4:
        raise ValueError("upsample2_pad_backward: bad sizes or channel slice")
    dx = torch.empty(N, h, w, C, device=dcat.device)
    lib.call("dcs_unet_upsample2_pad_backward", _pp(dcat, channel_offset), Cs, N, h, w, C, Ho, Wo, _p(dx), _stream())
    return dx


def sumsq_clip(g: torch.Tensor, clip: float = 0.0) -> torch.Tensor:
    """[norm, coefficient] on the device: the L2 norm of the flat gradient and clip_grad_norm_'s
    min(1, clip / (norm + 1e-6)) (1 for clip <= 0)."""
    g = _f32(g, "sumsq_clip")
    out = torch.empty(2, device=g.device)
    ws = workspace(lib.query("dcs_unet_sumsq_workspace_size", g.numel()), g.device)
    lib.call("dcs_unet_sumsq", _p(g), g.numel(), float(clip or 0.0), _p(out), _p(ws), ws.numel(), _stream())
    return out


# ---------------------------------------------------------------------------------------
# the trainable state
# ---------------------------------------------------------------------------------------
class _Layer:
    """One Conv3d + BatchNorm3d + ReLU: views of the flat buffers and the per-forward statistics."""

    def __init__(self, conv, bn, first: bool):
        self.conv3d, self.bn = conv, bn
        self.cout, self.cin = int(conv.weight.shape[0]), int(conv.weight.shape[1])
        self.first = first
        self.geom = _Geom(self.cin, self.cout, 3, 1, (1, 1, 1, 1), lib.DCS_PAD_ZERO)
        self.sizes = (self.cout * self.cin * 9, self.cout, self.cout)
        self.w = self.gamma = self.beta = self.gw = self.ggamma = self.gbeta = None
        self.fwd: Optional[_Conv] = None   # this forward's conv record: batch scale / shift [N,C]
        self.mean = self.invstd = None

    @property
    def scale(self):
        return self.fwd.scale[0]

    @property
    def shift(self):
        return self.fwd.shift[0]

    def pro(self):
        return (self.fwd.scale, self.fwd.shift, lib.ACT_RELU)


def _double(dc) -> Tuple:
    s = dc.double_conv
    return (s[0], s[1]), (s[3], s[4])


class TrainState:
    """Flat parameter / gradient / Adam buffers of one U-Net on one device, and its step."""

    def __init__(self, model, device=None):
        device = torch.device(device) if device is not None else next(model.parameters()).device
        if device.type != "cuda":
            raise RuntimeError("TrainState: a device model is required (no CPU fallback)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if not getattr(model, "trilinear", True):
            raise ValueError("the HIP path covers trilinear=True models only (no ConvTranspose3d up path)")
        if getattr(model, "n_channels", 1) != 1 or getattr(model, "n_classes", 1) != 1:
            raise ValueError("the HIP path covers one input channel and one output channel")
        for t in model.state_dict().values():
            if t.device != device or (t.is_floating_point() and t.dtype != torch.float32):
                raise RuntimeError("TrainState: the model must be float32 on the training device")
        self.model, self.device = model, device
        L = self.downs = model.DOWNS
        pairs = [_double(model.inc)] + [_double(getattr(model, f"down{i}").maxpool_conv[1]) for i in range(1, L + 1)]
        pairs += [_double(getattr(model, f"up{i}").conv) for i in range(1, L + 1)]
        self.layers: List[Tuple[_Layer, _Layer]] = []
        for i, (a, b) in enumerate(pairs):
            la, lb = _Layer(*a, first=(i == 0)), _Layer(*b, first=False)
            for l in (la, lb):
                c, bn = l.conv3d, l.bn
                if tuple(c.kernel_size) != (3, 3, 3) or tuple(c.padding) != (1, 1, 1) or c.bias is not None:
                    raise ValueError("3x3x3 convolutions with padding 1 and no bias expected")
                if bn.running_mean is None or bn.weight is None or bn.momentum is None:
                    raise ValueError("BatchNorm3d with affine parameters, running statistics and a momentum expected")
                if l.cout % 4 or l.cout <= 4 or (l.cin % 4 and not l.first):
                    raise ValueError(f"the HIP path needs channel counts that are multiples of 4 and above 4 "
                                     f"(got {l.cin} -> {l.cout})")
            self.layers.append((la, lb))
        self.enc, self.dec = self.layers[:L + 1], self.layers[L + 1:]
        for j, (a, _) in enumerate(self.dec):
            skip_c = self.enc[L - 1 - j][1].cout
            deep_c = (self.enc[-1][1] if j == 0 else self.dec[j - 1][1]).cout
            if a.cin != skip_c + deep_c:
                raise ValueError("up path: the conv's input channels are not skip + upsampled channels")
        oc = model.outc.conv
        self.cl = int(oc.in_channels)
        n = sum(sum(l.sizes) for pair in self.layers for l in pair) + self.cl + 1
        self.numel = n
        self.params = torch.empty(n, device=device)
        self.grads = torch.zeros(n, device=device)      # of the running micro-batch
        self.acc = torch.zeros(n, device=device)        # accumulated over micro-batches
        self.exp_avg = torch.zeros(n, device=device)
        self.exp_avg_sq = torch.zeros(n, device=device)
        self.steps, self.micro = 0, 0
        off = 0

        def take(k, shape):
            nonlocal off
            v = (self.params[off:off + k].view(shape), self.grads[off:off + k].view(shape))
            off += k
            return v

        with torch.no_grad():
            for pair in self.layers:
                for l in pair:
                    l.w, l.gw = take(l.sizes[0], (l.cout, l.cin, 3, 3))
                    l.gamma, l.ggamma = take(l.cout, (l.cout,))
                    l.beta, l.gbeta = take(l.cout, (l.cout,))
                    l.w.copy_(l.conv3d.weight[:, :, 1])
                    l.gamma.copy_(l.bn.weight)
                    l.beta.copy_(l.bn.bias)
                    l.bn.weight.data, l.bn.bias.data = l.gamma, l.beta          # the module reads the flat buffer
            self.wout, self.gwout = take(self.cl, (self.cl,))
            self.bout, self.gbout = take(1, (1,))
            self.wout.copy_(oc.weight.reshape(-1))
            self.bout.copy_(oc.bias.reshape(-1))
            oc.weight.data, oc.bias.data = self.wout.view(1, self.cl, 1, 1, 1), self.bout
        assert off == n
        self._weights = [l.w for pair in self.layers for l in pair]

    # ---- forward ---------------------------------------------------------------------
    def _conv_bn(self, l: _Layer, x: torch.Tensor, pro: Optional[_Layer] = None) -> torch.Tensor:
        N = x.shape[0]
        l.fwd = _Conv(l.geom, l.w, None, None, 4 if l.first else None)
        y = U._conv(l.fwd, x, pro=pro.fwd if pro is not None else None)
        with timed(f"bn_stats {l.cout} @{y.shape[1]}x{y.shape[2]}"):
            l.fwd.scale, l.fwd.shift, l.mean, l.invstd = bn_stats(
                y, l.gamma, l.beta, l.bn.eps, l.bn.momentum, l.bn.running_mean, l.bn.running_var, nrep=N)
        return y

    def _check(self, x: torch.Tensor, target: torch.Tensor):
        from ..nmodel.model import check_slice_size
        for t, name in ((x, "input"), (target, "target")):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise RuntimeError(f"{name}: device tensor required (no CPU fallback)")
            if t.dim() != 5 or t.dtype != torch.float32:
                raise ValueError(f"{name}: a float32 [N,1,1,H,W] batch of depth-1 patches required")
            if t.shape[1] != 1:
                raise ValueError("the HIP path covers one input channel and one output channel")
            if t.shape[2] != 1:
                raise ValueError("the HIP path trains on depth-1 patches (depth > 1 is a true 3-D convolution)")
        if x.shape != target.shape or x.numel() == 0:
            raise ValueError("input and target must have one non-empty shape")
        N, _, _, H, W = x.shape
        check_slice_size(self.downs, H, W)
        if N * (H >> self.downs) * (W >> self.downs) == 1:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size "
                             f"{(N, self.enc[-1][1].cout, 1, H >> self.downs, W >> self.downs)}")
        return N, H, W

    @torch.no_grad()
    def accumulate(self, x: torch.Tensor, target: torch.Tensor, gscale: float = 1.0) -> torch.Tensor:
        """Forward and backward of one micro-batch in training mode; adds the gradient of gscale *
        mean |model(x) - target| to the accumulator.  Returns that loss term as a device [1] tensor."""
        N, H, W = self._check(x, target)
        L = self.downs
        with torch.cuda.device(self.device):
            ops.range_arena_reset(self.device)   # the records of the last micro-batch are stale
            x4 = ops.pack_nhwc4(x.reshape(N, 1, H, W))
            tgt = target.reshape(N, H, W).contiguous()
            # forward, keeping every conv output, concatenated tensor and pooled map
            ins, ys, cats, cur = [], [], [], x4
            for lvl, (a, b) in enumerate(self.enc):
                y1 = self._conv_bn(a, cur)
                y2 = self._conv_bn(b, y1, pro=a)
                ins.append(cur)
                ys.append((y1, y2))
                if lvl == L:
                    break
                cat = torch.empty(N, y2.shape[1], y2.shape[2], self.dec[L - 1 - lvl][0].cin, device=self.device)
                with timed(f"affine+relu+pool {b.cout} @{y2.shape[1]}x{y2.shape[2]}"):
                    _, cur = U.affine_relu_pool(y2, b.scale, b.shift, skip=cat)
                cats.append(cat)
            deep, last = ys[-1][1], self.enc[-1][1]
            dys = []
            for j, (a, b) in enumerate(self.dec):
                cat = cats[L - 1 - j]
                with timed(f"upsample+pad {last.cout} ->{cat.shape[1]}x{cat.shape[2]}"):
                    U.upsample2_pad(deep, cat.shape[1:3], last.scale, last.shift, out=cat,
                                    channel_offset=cat.shape[3] - last.cout)
                y1 = self._conv_bn(a, cat)
                y2 = self._conv_bn(b, y1, pro=a)
                dys.append((y1, y2))
                deep, last = y2, b
            with timed(f"l1_out {last.cout}->1 @{H}x{W}"):
                loss, dout, _ = l1_out(deep, last.scale, last.shift, self.wout, self.bout, tgt, gscale)

            # backward
            with timed(f"bn_relu_backward C {last.cout} @{H}x{W}"):
                dy = bn_relu_backward(deep, last.scale, last.shift, last.mean, last.invstd, dout=dout, wout=self.wout,
                                      dgamma=last.ggamma, dbeta=last.gbeta, dwout=self.gwout, dbias=self.gbout)[0]
            dskip = [None] * L
            for j in reversed(range(L)):
                a, b = self.dec[j]
                y1, _ = dys[j]
                cat = cats[L - 1 - j]
                dcat = self._double_backward(a, b, cat, y1, dy, want_dx=True)
                dskip[L - 1 - j] = dcat
                prev = self.dec[j - 1][1] if j > 0 else self.enc[-1][1]
                yprev = dys[j - 1][1] if j > 0 else ys[-1][1]
                with timed(f"upsample+pad backward {prev.cout} @{yprev.shape[1]}x{yprev.shape[2]}"):
                    ddeep = upsample2_pad_backward(dcat, yprev.shape[1:3], prev.cout, dcat.shape[3] - prev.cout)
                with timed(f"bn_relu_backward A {prev.cout} @{yprev.shape[1]}x{yprev.shape[2]}"):
                    dy = bn_relu_backward(yprev, prev.scale, prev.shift, prev.mean, prev.invstd, da=ddeep,
                                          dgamma=prev.ggamma, dbeta=prev.gbeta)[0]
            dpool = None
            for lvl in reversed(range(L + 1)):
                a, b = self.enc[lvl]
                y1, y2 = ys[lvl]
                if lvl < L:
                    with timed(f"bn_relu_backward B {b.cout} @{y2.shape[1]}x{y2.shape[2]}"):
                        dy = bn_relu_backward(y2, b.scale, b.shift, b.mean, b.invstd, da=dskip[lvl], dpool=dpool,
                                              dgamma=b.ggamma, dbeta=b.gbeta)[0]
                dpool = self._double_backward(a, b, ins[lvl], y1, dy, want_dx=lvl > 0)
            with timed("accumulate"):
                ops.scale_add_(self.acc, self.grads, 1.0)
            for pair in self.layers:
                for l in pair:
                    l.bn.num_batches_tracked.add_(1)
            self.micro += 1
            self._invalidate()
        return loss

    def _double_backward(self, a: _Layer, b: _Layer, x: torch.Tensor, y1: torch.Tensor, dy2: torch.Tensor,
                         want_dx: bool) -> Optional[torch.Tensor]:
        """Backward of one DoubleConv given dy2 (the gradient of its second conv's output): both weight
        gradients, both BatchNorms', and the gradient of its input x when ``want_dx``."""
        N, H, W, _ = y1.shape
        tag = f"@{H}x{W}"
        with timed(f"wgrad {b.cin}->{b.cout} {tag}"):
            b.geom.wgrad(dy2, Src.nhwc(y1), pro=a.pro(), out=b.gw)
        with timed(f"dgrad {b.cout}->{b.cin} {tag}"):
            da1 = b.geom.dgrad(dy2, b.geom.pack_dgrad(b.w), H, W)
        with timed(f"bn_relu_backward A {a.cout} {tag}"):
            dy1 = bn_relu_backward(y1, a.scale, a.shift, a.mean, a.invstd, da=da1, dgamma=a.ggamma, dbeta=a.gbeta)[0]
        with timed(f"wgrad {a.cin}->{a.cout} {tag}"):
            a.geom.wgrad(dy1, Src.nhwc(x), out=a.gw)
        if not want_dx:
            return None
        with timed(f"dgrad {a.cout}->{a.cin} {tag}"):
            return a.geom.dgrad(dy1, a.geom.pack_dgrad(a.w), H, W)

    # ---- optimizer ---------------------------------------------------------------------
    @torch.no_grad()
    def step(self, lr: float, clip: Optional[float] = None) -> torch.Tensor:
        """clip_grad_norm_(clip) of the accumulated gradient, one Adam step (betas 0.9 / 0.999, eps
        1e-8, no weight decay), the write-back into the module, and a zeroed accumulator.  Returns
        the device pair [gradient norm before clipping, clip coefficient]."""
        with torch.cuda.device(self.device):
            with timed("sumsq+clip"):
                nc = sumsq_clip(self.acc, clip or 0.0)
                lib.call("dcs_scale_dev", _p(self.acc), _pp(nc, 1), _p(self.grads), self.numel, _stream())
            self.steps += 1
            with timed("adam"):
                ops.adam_step(self.params, self.grads, self.exp_avg, self.exp_avg_sq, lr, ADAM_BETAS[0], ADAM_BETAS[1],
                              ADAM_EPS, self.steps)
            self.acc.zero_()
            self.micro = 0
            self.write_back()
        return nc

    @torch.no_grad()
    def write_back(self) -> None:
        """The folded weights into the centre depth tap of the module's Conv3d parameters (the
        BatchNorm and output parameters are views of the buffer already); packs and the module's
        inference plan are dropped: a kernel's write through a raw pointer bumps no version counter."""
        for pair in self.layers:
            for l in pair:
                l.conv3d.weight.data[:, :, 1].copy_(l.w)
        ops.bump_weights_epoch(self._weights)
        self._invalidate()

    def _invalidate(self) -> None:
        if getattr(self.model, "_dcs_unet_plan", None) is not None:
            self.model._dcs_unet_plan = None

    def named_gradients(self, accumulated: bool = False) -> dict:
        """{parameter name of the module: its gradient}: of the last micro-batch, or the accumulator's
        (views; a Conv3d weight's is the [Cout,Cin,3,3] gradient of its centre depth tap)."""
        buf = self.acc if accumulated else self.grads
        by_param = {}
        for pair in self.layers:
            for l in pair:
                by_param[id(l.conv3d.weight)] = l.gw
                by_param[id(l.bn.weight)], by_param[id(l.bn.bias)] = l.ggamma, l.gbeta
        oc = self.model.outc.conv
        by_param[id(oc.weight)], by_param[id(oc.bias)] = self.gwout, self.gbout
        base = self.grads.data_ptr()
        out = {}
        for name, p in self.model.named_parameters():
            g = by_param[id(p)]
            o = (g.data_ptr() - base) // 4
            out[name] = buf[o:o + g.numel()].view(g.shape)
        return out

    # ---- checkpoint --------------------------------------------------------------------
    def optimizer_state_dict(self) -> dict:
        return {"step": self.steps, "exp_avg": self.exp_avg.cpu(), "exp_avg_sq": self.exp_avg_sq.cpu(),
                "betas": list(ADAM_BETAS), "eps": ADAM_EPS}

    def load_optimizer_state_dict(self, sd: dict) -> None:
        if sd["exp_avg"].numel() != self.numel:
            raise ValueError("optimizer state of another model")
        self.steps = int(sd["step"])
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
