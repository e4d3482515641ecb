"""LPIPS on the AlexNet trunk on the HIP path, behind the lpips 0.1.4 interface (`lpips.LPIPS(net='alex')`).

The reference's evaluators report LPIPS for every RD point (coremasic/mywork/test2_real.py:36-37, :105-112, test3_real.py:33-34,
:107-109): `loss_fn = lpips.LPIPS(net='alex', spatial=False)`, then `loss_fn.forward(target, x_hat).mean().item()` per view.

**Parity unpinned.**  lpips is neither installed here nor part of the reference tree; this module restates lpips 0.1.4's published
algorithm (tests/test_gpu_lpips.py holds the restatement in plain torch ops that the kernels are tested against):

  x <- 2x - 1 if `normalize`;  x <- (x - shift) / scale  (shift (-.030, -.088, -.188), scale (.458, .448, .450));
  AlexNet features with a tap after the ReLU of each of the five convolutions (MaxPool2d(3, 2) in front of conv2 and conv3);
  per tap and picture f / (sqrt(sum_c f^2) + 1e-10), then sum_c lin_c (f0_c - f1_c)^2, the mean over pixels, the sum over the taps.

No trained weights ship with this repository and nothing is ever downloaded: every number in its tests and documents is made with
`pnet_rand=True` / `pretrained=False` (torch's default initialisation, or seeded weights through `load_state_dict`).  Published LPIPS
values need two files: lpips's `weights/v0.1/alex.pth` (the five `lin` layers; `model_path`, default `lpips/weights/v0.1/alex.pth`
next to the `lpips` package of this repository) and torchvision's `alexnet-owt-7be5be79.pth` under
`torch.hub.get_dir()/checkpoints` (the backbone, `features.{0,3,6,8,10}.{weight,bias}`; torchvision itself is not needed).
The state dict has lpips's 22 keys, so its checkpoints load unchanged.

`forward` is a schedule of 13 HIP launches on the current stream (masic_amd/csrc/lpips.hip, conv.hip), float32 throughout whatever
`masic_amd.nn.set_precision` says, without host synchronisation: the first layer (11 x 11, stride 4) reads the two picture tensors
in place (no concat) with `normalize` and the scaling layer folded into its staging, two max-pools, layers 2-5 on the float32
implicit-GEMM convolution with bias and ReLU folded in, one distance launch per tap and one finishing launch.  The two pictures of
comparison n travel as images 2n and 2n + 1 of one batch of 2N.  A picture's value does not depend on the rest of the batch: the
reused convolution picks its K chunk (hence its summation order) from the batch size among other things, so a layer whose launch
plan for 2N images would sum in another order than the plan for 2 (ops.conv_plan_signature) runs once per picture pair instead.

**As a loss.**  `loss_fn(x_hat, x).mean().backward()`: when grad is enabled and a picture on the device requires grad, the same 13
launches run inside one `torch.autograd.Function` that keeps the five taps, and its backward is a second schedule of 12 launches
(masic_amd/csrc/lpips_bwd.hip, conv.hip): per tap, from the last to the first, one launch that forms the gradient of the normalised
distance (under the upstream gradients of `val` and of the per-layer values, read on the device), adds what arrives from the layer
above and applies the tap's ReLU mask; between the taps the input gradient of layers 5-2 as the float32 implicit-GEMM convolution run
as the opposite layer kind on the same weight, and the max-pool backward as a gather; last the input gradient of the first layer with
the scaling layer, `normalize` and the split into the two pictures' gradients folded into its store.  With one picture requiring grad
(the training case: the other is the target) the chain runs on that side's N images, with both on the 2N interleaved ones.  Float32,
no float atomics, fixed summation orders, capturable; picture n's gradient does not depend on the rest of the batch, and the
one-sided chain gives the bits of the two-sided one: a layer's input gradient runs as one launch only if its plan sums in the order of
the ONE-image plan, else per pair if the two-image plan does, else per image.  Once differentiable.  Deliberate deviation from lpips's
autograd: at a feature pixel that is zero in every channel torch's sqrt backward is 0 / 0 = NaN; here the norm's derivative is
defined as 0 there, in line with the forward's 0 / 1e-10 = 0 (include/masic_hip.h, masic_lpips_dist_bwd).

Not built (each raises): other trunks, version != '0.1', `spatial=True`, `lpips=False`, `pnet_tune=True` and any other weight gradient
(no parameter of this module requires grad, and one flipped to requires_grad raises in forward), training mode (Dropout in the lin
layers), double backward, CPU tensors (with or without grad).
"""
import os

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import nn as _mnn
from . import ops as _hip
from ._lib import PREC_F32 as _F32

__all__ = ["LPIPS"]

_CHNS = (64, 192, 384, 256, 256)
# (slice, index in torchvision's `features`, Cin, Cout, kernel, stride, padding, pool in front)
_CONVS = ((1, 0, 3, 64, 11, 4, 2, False), (2, 3, 64, 192, 5, 1, 2, True), (3, 6, 192, 384, 3, 1, 1, True),
          (4, 8, 384, 256, 3, 1, 1, False), (5, 10, 256, 256, 3, 1, 1, False))
_BACKBONE_FILE = "alexnet-owt-7be5be79.pth"
_MIN_SIDE = 31          # 31 -> 7 -> 3 -> 1: below it the second pool has no window


def default_model_path():
    """lpips/weights/v0.1/alex.pth next to this repository's `lpips` package."""
    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lpips", "weights", "v0.1", "alex.pth")


def backbone_path():
    """Where torchvision's alexnet(pretrained=True) keeps its download."""
    return os.path.join(torch.hub.get_dir(), "checkpoints", _BACKBONE_FILE)


class ScalingLayer(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.Tensor([-.030, -.088, -.188])[None, :, None, None])
        self.register_buffer("scale", torch.Tensor([.458, .448, .450])[None, :, None, None])

    def forward(self, inp):
        raise NotImplementedError("lpips.ScalingLayer: folded into the first layer's kernel (LPIPS.forward); it does not run on its own")


class NetLinLayer(nn.Module):
    """A single 1x1 convolution without bias behind an (eval-mode identity) Dropout: `model.1.weight` [1,C,1,1]."""

    def __init__(self, chn_in, chn_out=1, use_dropout=False):
        super().__init__()
        layers = [nn.Dropout()] if use_dropout else []
        layers += [nn.Conv2d(chn_in, chn_out, 1, stride=1, padding=0, bias=False)]
        self.model = nn.Sequential(*layers)

    @property
    def weight(self):
        return self.model[-1].weight

    def forward(self, x):
        raise NotImplementedError("lpips.NetLinLayer: fused into the distance kernel (LPIPS.forward); it does not run on its own")


class _AlexFeatures(nn.Module):
    """`net` of lpips's LPIPS: slice1 .. slice5 holding torchvision's `features` entries under their original indices.  The ReLU and
    MaxPool entries keep the indices; their arithmetic is fused into the launches of LPIPS.forward."""

    def __init__(self):
        super().__init__()
        self.N_slices = 5
        bounds = ((0, 2), (2, 5), (5, 8), (8, 10), (10, 12))
        convs = {idx: (cin, cout, k, s, p) for _, idx, cin, cout, k, s, p, _ in _CONVS}
        for s, (lo, hi) in enumerate(bounds, start=1):
            seq = nn.Sequential()
            for i in range(lo, hi):
                if i in convs:
                    cin, cout, k, st, p = convs[i]
                    seq.add_module(str(i), nn.Conv2d(cin, cout, kernel_size=k, stride=st, padding=p))
                elif i in (2, 5):
                    seq.add_module(str(i), nn.MaxPool2d(kernel_size=3, stride=2))
                else:
                    seq.add_module(str(i), nn.ReLU(inplace=True))
            setattr(self, f"slice{s}", seq)

    def conv(self, s):
        seq = getattr(self, f"slice{s}")
        return seq[0] if s == 1 else seq[1 if s in (2, 3) else 0]

    def forward(self, x):
        raise NotImplementedError("lpips alexnet trunk: runs as part of LPIPS.forward only")


def _conv_relu(conv, x):
    """relu(conv(x) + bias) on the float32 implicit-GEMM path for a batch of picture pairs (images 2n, 2n + 1).  One launch when its
    plan sums in the order of the two-image launch (the tiles may differ), else one launch per pair -- either way pair n gets the
    arithmetic of a call on that pair alone."""
    B, _, H, W = x.shape
    k, s, p = conv.kernel_size[0], conv.stride[0], conv.padding[0]
    w = conv.weight

    def run(xv, out=None):
        desc = _hip.make_conv_desc(xv.shape[0], conv.in_channels, H, W, conv.out_channels, k, k, s, p, act=_hip.ACT_RELU, prec=_F32)
        packed = _mnn._cached(conv, "_packed_cache", _mnn.weight_key(w), (xv.shape[0], H, W, _F32),
                              lambda: _hip.pack_conv_weight(w.detach().contiguous(), desc))
        return _hip.conv2d(xv, packed, conv.bias.detach(), desc, out=out)

    if B == 2:
        return run(x)
    d2 = _hip.make_conv_desc(2, conv.in_channels, H, W, conv.out_channels, k, k, s, p, act=_hip.ACT_RELU, prec=_F32)
    dB = _hip.make_conv_desc(B, conv.in_channels, H, W, conv.out_channels, k, k, s, p, act=_hip.ACT_RELU, prec=_F32)
    if _hip.conv_plan_signature(d2) == _hip.conv_plan_signature(dB):
        return run(x)
    y = torch.empty((B, conv.out_channels, dB.Ho, dB.Wo), dtype=torch.float32, device=x.device)
    for n in range(0, B, 2):
        run(x[n:n + 2], out=y[n:n + 2])
    return y


def _conv_dgrad(conv, g, unit):
    """The input gradient of a stride-1 layer of the trunk (pad = k // 2: the map keeps its size) from the gradient g [B,Cout,h,w] of its
    pre-activation: the float32 implicit GEMM as the opposite layer kind on the same weight.  `unit`: the images one call on a single
    comparison holds (1 for a one-sided chain, 2 for both sides).  One launch when its plan sums in the order of the one-image plan, else
    one per `unit` images if that plan does, else one per image -- image n gets the arithmetic of a one-image launch in every case, so
    the one-sided and the two-sided chain agree bit for bit."""
    B, _, H, W = g.shape
    k, p = conv.kernel_size[0], conv.padding[0]
    w = conv.weight

    def desc(b):
        return _hip.make_conv_desc(b, conv.out_channels, H, W, conv.in_channels, k, k, 1, p, transposed=True, prec=_F32)

    def run(gv, out=None):
        d = desc(gv.shape[0])
        packed = _mnn._cached(conv, "_packed_dgrad_cache", _mnn.weight_key(w), (gv.shape[0], H, W, _F32),
                              lambda: _hip.pack_conv_weight(w.detach().contiguous(), d))
        return _hip.conv2d(gv, packed, None, d, out=out)

    one = _hip.conv_plan_signature(desc(1))
    step = next(u for u in (B, unit, 1) if u == 1 or (B % u == 0 and _hip.conv_plan_signature(desc(u)) == one))
    if step == B:
        return run(g)
    y = torch.empty((B, conv.in_channels, H, W), dtype=torch.float32, device=g.device)
    for n in range(0, B, step):
        run(g[n:n + step], out=y[n:n + step])
    return y


class _LpipsFn(torch.autograd.Function):
    """out [6,N] (row 0 the value, rows 1-5 the per-layer values) of LPIPS._run with the five taps kept for the backward schedule."""

    @staticmethod
    def forward(ctx, in0, in1, mod, normalize):
        taps, lins, out = mod._run(in0, in1, normalize)
        ctx.mod, ctx.normalize, ctx.hw = mod, normalize, tuple(in0.shape[2:])
        ctx.save_for_backward(*taps, *lins)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        taps, lins = ctx.saved_tensors[:5], ctx.saved_tensors[5:]
        mod = ctx.mod
        sides = (1 if ctx.needs_input_grad[0] else 0) | (2 if ctx.needs_input_grad[1] else 0)
        if not sides:
            return None, None, None, None
        unit, stride, off = (2, 1, 0) if sides == 3 else (1, 2, sides - 1)
        gout = gout.contiguous()
        g = None
        for t in range(4, -1, -1):
            g = _hip.lpips_dist_bwd(taps[t], lins[t], gout, t, sides, g_in=g, out=g)
            if t:
                s, *_, pool = _CONVS[t]
                g = _conv_dgrad(mod.net.conv(s), g, unit)
                if pool:
                    g = _hip.maxpool3s2_bwd(taps[t - 1], g, stride, off)
        c1 = mod.net.conv(1)
        w = c1.weight
        packed = _mnn._cached(c1, "_packed_lpips_bwd_cache", _mnn.weight_key(w), (),
                              lambda: _hip.pack_lpips_conv1_bwd_weight(w.detach().contiguous()))
        d0, d1 = _hip.lpips_conv1_bwd(g, packed, mod.scaling_layer.scale, ctx.hw[0], ctx.hw[1], ctx.normalize, sides)
        return d0, d1, None, None


class LPIPS(nn.Module):
    def __init__(self, pretrained=True, net='alex', version='0.1', lpips=True, spatial=False, pnet_rand=False, pnet_tune=False,
                 use_dropout=True, model_path=None, eval_mode=True, verbose=True):
        super().__init__()
        for what, bad in ((f"net={net!r} (only 'alex')", net != 'alex'), (f"version={version!r} (only '0.1')", version != '0.1'),
                          ("spatial=True", bool(spatial)), ("lpips=False (the unweighted baseline)", not lpips),
                          ("pnet_tune=True (no weight gradients)", bool(pnet_tune))):
            if bad:
                raise NotImplementedError(f"lpips.LPIPS: {what} is not built on the HIP path")
        if verbose:
            print('Setting up [%s] perceptual loss: trunk [%s], v[%s], spatial [%s]' % ('LPIPS', net, version, 'off'))
        self.pnet_type = net
        self.pnet_tune = pnet_tune
        self.pnet_rand = pnet_rand
        self.spatial = spatial
        self.lpips = lpips
        self.version = version
        self.scaling_layer = ScalingLayer()
        self.chns = list(_CHNS)
        self.L = len(self.chns)
        self.net = _AlexFeatures()
        for i, c in enumerate(self.chns):
            setattr(self, f"lin{i}", NetLinLayer(c, use_dropout=use_dropout))
        self.lins = nn.ModuleList([getattr(self, f"lin{i}") for i in range(self.L)])

        want_lin, want_net = bool(pretrained), not pnet_rand
        if want_lin or want_net:
            lin_path = default_model_path() if model_path is None else model_path
            net_path = backbone_path()
            missing = [p for p, want in ((lin_path, want_lin), (net_path, want_net)) if want and not os.path.isfile(p)]
            if missing:
                raise FileNotFoundError(
                    f"lpips.LPIPS: missing {missing}. Trained weights are read from two files and never downloaded: the lin layers from "
                    f"{lin_path} (lpips's weights/v0.1/alex.pth; `model_path`) and the AlexNet backbone from {net_path} (torchvision's "
                    f"{_BACKBONE_FILE}). Pass pretrained=False / pnet_rand=True to do without them.")
            if want_net:
                sd = torch.load(net_path, map_location="cpu")
                for s, idx, *_ in _CONVS:
                    conv = self.net.conv(s)
                    with torch.no_grad():
                        conv.weight.copy_(sd[f"features.{idx}.weight"])
                        conv.bias.copy_(sd[f"features.{idx}.bias"])
            if want_lin:
                if verbose:
                    print('Loading model from: %s' % lin_path)
                self.load_state_dict(torch.load(lin_path, map_location="cpu"), strict=False)
        for prm in self.parameters():          # no weight gradient exists for any of them
            prm.requires_grad = False
        if eval_mode:
            self.eval()

    def _check(self, in0, in1):
        if self.training:
            raise NotImplementedError("lpips.LPIPS: forward in training mode (Dropout in the lin layers) is not built -- call .eval()")
        for t in (in0, in1):
            if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.shape[1] != 3:
                raise ValueError(f"lpips.LPIPS: inputs must be [N,3,H,W] tensors, got {tuple(getattr(t, 'shape', ()))}")
        if in0.shape != in1.shape:
            raise ValueError(f"lpips.LPIPS: inputs differ in shape: {tuple(in0.shape)} and {tuple(in1.shape)}")
        if in0.dtype != torch.float32 or in1.dtype != torch.float32:
            raise ValueError(f"lpips.LPIPS: float32 only, got {in0.dtype} and {in1.dtype}")
        if in0.shape[0] < 1 or min(in0.shape[2:]) < _MIN_SIDE:
            raise ValueError(f"lpips.LPIPS: {tuple(in0.shape)}: at least one picture with sides >= {_MIN_SIDE} (the second max-pool "
                             "would have no window)")
        grad = torch.is_grad_enabled() and (in0.requires_grad or in1.requires_grad)
        if grad and not (in0.is_cuda and in1.is_cuda):
            raise NotImplementedError("lpips.LPIPS: no backward is built for CPU tensors -- the gradients run on the MI355X path only")
        if torch.is_grad_enabled() and any(prm.requires_grad for prm in self.parameters()):
            raise NotImplementedError("lpips.LPIPS: a parameter requires grad, but no weight gradient is built (only the pictures' "
                                      "gradients) -- keep the parameters at requires_grad=False or call under torch.no_grad()")
        for t, name in ((in0, "in0"), (in1, "in1")):
            if not t.is_cuda:
                raise RuntimeError(f"lpips.LPIPS: {name} must be a CUDA (HIP) tensor -- the MI355X path has no CPU fallback")
        return grad

    def _taps(self, in0, in1, normalize):
        c1 = self.net.conv(1)
        w = c1.weight
        packed = _mnn._cached(c1, "_packed_lpips_cache", _mnn.weight_key(w), (),
                              lambda: _hip.pack_lpips_conv1_weight(w.detach().contiguous()))
        sl = self.scaling_layer
        taps = [_hip.lpips_conv1(in0.detach().contiguous(), in1.detach().contiguous(), packed, c1.bias.detach(), sl.shift, sl.scale, normalize)]
        for s, *_, pool in _CONVS[1:]:
            x = _hip.maxpool3s2(taps[-1]) if pool else taps[-1]
            taps.append(_conv_relu(self.net.conv(s), x))
        return taps

    def _run(self, in0, in1, normalize):
        """The 13 launches: (taps, lin weights, out [6,N])."""
        taps = self._taps(in0, in1, normalize)
        lins = [self.lins[i].weight.detach() for i in range(self.L)]
        return taps, lins, _hip.lpips_distance(taps, lins)

    def features(self, in0, in1, normalize=False):
        """The five taps [2N,C,h,w] (float32 NCHW), in0[n] as image 2n and in1[n] as image 2n + 1.  Not differentiable: gradients flow
        through `forward` only."""
        if self._check(in0, in1):
            raise NotImplementedError("lpips.LPIPS.features: the taps carry no gradient -- differentiate forward(), or call under "
                                      "torch.no_grad()")
        with torch.no_grad():
            return self._taps(in0, in1, normalize)

    def forward(self, in0, in1, retPerLayer=False, normalize=False):
        if self._check(in0, in1):
            out = _LpipsFn.apply(in0, in1, self, bool(normalize))
        else:
            with torch.no_grad():
                out = self._run(in0, in1, normalize)[2]
        N = in0.shape[0]
        val = out[0].view(N, 1, 1, 1)
        if retPerLayer:
            return val, [out[1 + i].view(N, 1, 1, 1) for i in range(self.L)]
        return val
