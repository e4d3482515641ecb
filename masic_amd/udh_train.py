"""Training stage of the UDH homography net (the reference's udh/udh/model.py + the step of udh/udh/train.py:26-31), MI355X-native.

    delta = Net(patch_a, patch_b)
    loss  = photometric_loss(delta, img_a, patch_b, corners)
    loss.backward(); Adam.step()

`Net` has the 20 state-dict tensors of the reference (and of the codec-side, inference-only `coremasic/mywork/model.py: Net`, into
which a checkpoint trained here loads unchanged).  With grad enabled, a forward records ONE autograd node for the whole net
(`_NetFn`, in the style of masic_amd/autograd.py: AnalysisFn): the forward is the inference schedule of 13 launches plus the
Dropout masks, the backward a schedule of HIP launches (masic_amd/csrc/udh_train.hip, the float32 implicit-GEMM convolution run as
the transposed layer, ops.conv2d_wgrad, ops.channel_sum).  The node keeps the eight convolution outputs and the two linear inputs;
the three pooled tensors are re-made in the backward (one small launch each).  Only the parameters receive gradients: the patches
are data.  In `eval()` under `no_grad` the forward IS the inference schedule, bit for bit.

Dropout: in training mode both Dropout(0.5) layers are active.  Their masks are uint8 keep-bits drawn on the device by torch
(`torch.rand(...) >= 0.5` on the device generator); the kernels apply them with scale 2.  The mask STREAM therefore differs from
the reference's (its CPU generator, or CUDA's Philox layout): only the distribution is the same.  `forward(a, b, dropout_masks=(m1,
m2))` takes fixed masks, m1 [B, 128 (p/8)^2] and m2 [B, 1024].

Always float32 operands, whatever `masic_amd.nn.set_precision` says (the inference net's policy).  No CPU path: tensors must live
on an MI355X (`cuda`) device.  Weight gradients of layers 2-8 follow `masic_amd.determinism`; every kernel new to this stage has a
fixed summation order with or without it.

`photometric_loss(delta, img_a, patch_b, corners)` is the reference's (udh/udh/model.py:18-45): the mean over B*h*w of
|warp_perspective(img_a, inverse(h), patch_b.shape[-2:]) - patch_b| with h = get_perspective_transform(corners - corners[:, :1],
corners + delta), kornia 0.5.0's warp as everywhere in this library (ops.set_warp_align_corners is honoured).  The gradient flows to
`delta` only.  A degenerate quadrilateral gives a NaN loss and NaN gradients.
"""
import torch
import torch.nn as nn
from torch.autograd import Function

from . import nn as _mnn
from . import ops as _hip
from ._lib import PREC_F32 as _F32

_PATCH_SIZES = (32, 64, 128)
_WIDTHS = (2, 64, 64, 128, 128)
_HIDDEN = 1024


class Flatten(nn.Module):
    """[B, C, H, W] -> [B, C * H * W] in NCHW order (`fc.0` of the reference's layout; holds no parameters)."""

    def forward(self, x):
        return x.flatten(1)


def _conv3x3_relu(conv, x):
    """relu(conv(x) + bias) on the float32 implicit-GEMM path, the pack cached per weight version."""
    B, _, H, W = x.shape
    desc = _hip.make_conv_desc(B, conv.in_channels, H, W, conv.out_channels, 3, 3, 1, 1, act=_hip.ACT_RELU, prec=_F32)
    w = conv.weight
    packed = _mnn._cached(conv, "_packed_cache", _mnn.weight_key(w), (B, H, W, _F32),
                          lambda: _hip.pack_conv_weight(w.detach().contiguous(), desc))
    return _hip.conv2d(x, packed, conv.bias.detach(), desc)


def _conv3x3_backward(conv, x, y, g, need_gx=True):
    """(dx, dW, db) of y = relu(conv(x) + bias) from g = dL/dy; float32 whatever the library's precision setting."""
    g = _hip.elementwise(_hip.EW_ACT_BWD, g, y, s0=_hip.ACT_RELU)
    return _conv3x3_backward_pre(conv, x, g, need_gx)


def _conv3x3_backward_pre(conv, x, g, need_gx=True):
    """The same from g = the gradient in front of the ReLU."""
    B, Cin, H, W = x.shape
    Cout = conv.out_channels
    w = conv.weight.detach().contiguous()
    gx = None
    if need_gx:
        d = _hip.make_conv_desc(B, Cout, H, W, Cin, 3, 3, 1, 1, transposed=True, prec=_F32)
        gx = _hip.conv2d(g, _hip.pack_conv_weight(w, d), None, d)
    dw = _hip.make_conv_desc(B, Cin, H, W, Cout, 3, 3, 1, 1, prec=_F32)
    return gx, _hip.conv2d_wgrad(x, g, dw, tuple(w.shape)), _hip.channel_sum(g)


class Block(nn.Module):
    """Two 3x3 convolutions, each followed by ReLU, and an optional 2x2 max-pool.  The parameters sit at `layers.0` and `layers.2`
    (the state-dict contract); the ReLU and pool entries of `layers` are placeholders that keep the indices.  On its own a Block is
    the inference block (no autograd graph); gradients are recorded by `Net`."""

    def __init__(self, inchannels, outchannels, batch_norm=False, pool=True):
        super().__init__()
        if batch_norm:
            raise NotImplementedError("udh model.Block: batch_norm=True is not built (no published checkpoint uses it)")
        self.pool = bool(pool)
        self.layers = nn.Sequential()
        for index, cin in ((0, inchannels), (2, outchannels)):
            self.layers.add_module(str(index), nn.Conv2d(cin, outchannels, kernel_size=3, padding=1))
            self.layers.add_module(str(index + 1), nn.ReLU())
        if self.pool:
            self.layers.add_module("4", nn.MaxPool2d(2, 2))

    def run(self, x, pair=None, keep=None):
        """`pair` = (a, b): the two input channels as two [B,1,H,W] tensors (the first-layer kernel, no concat).  `keep`: a list
        that receives the two convolution outputs."""
        first, second = self.layers[0], self.layers[2]
        with torch.no_grad():
            if pair is None and first.in_channels == 2:
                _hip._dev(x, "block input")
                pair = (x[:, 0:1].contiguous(), x[:, 1:2].contiguous())
            if pair is not None:
                if first.in_channels != 2:
                    raise ValueError("udh model.Block: a patch pair feeds a block with two input channels only")
                y1 = _hip.udh_conv1(pair[0], pair[1], first.weight.detach(), first.bias.detach())
            else:
                y1 = _conv3x3_relu(first, x)
            y2 = _conv3x3_relu(second, y1)
            if keep is not None:
                keep += [y1, y2]
            return _hip.maxpool2(y2) if self.pool else y2

    def forward(self, x):
        return self.run(x)


def _schedule(net, a, b, masks, keep=None):
    """The forward of the whole net: the inference schedule, plus the Dropout masks when given.  Returns out [B,8] (and fills `keep`
    with the eight convolution outputs, then the two linear inputs)."""
    x = net.cnn[0].run(None, pair=(a, b), keep=keep)
    for blk in list(net.cnn)[1:]:
        x = blk.run(x, keep=keep)
    l1, l2 = net.fc[2], net.fc[5]
    w1, b1, w2, b2 = l1.weight.detach(), l1.bias.detach(), l2.weight.detach(), l2.bias.detach()
    if keep is None and masks is None:
        return _hip.udh_fc(x, w1, b1, w2, b2)
    m1, m2 = masks if masks is not None else (None, None)
    xd, hidden, out = _hip.udh_fc_train(x, w1, b1, w2, b2, m1, m2)
    if keep is not None:
        keep += [xd, hidden]
    return out


class _NetFn(Function):
    """delta = Net(a, b) as one node over the 20 parameters (a and b are data: no gradient)."""

    @staticmethod
    def forward(ctx, net, a, b, m1, m2, *params):
        keep = []
        out = _schedule(net, a, b, None if m1 is None else (m1, m2), keep)
        ctx.net, ctx.masks = net, (m1, m2)
        # the parameters are saved too (no copy): autograd's version check then refuses a backward after an in-place update of
        # a weight, which would otherwise mix the forward's weights with newer ones
        ctx.save_for_backward(a, b, *keep, *params)
        return out.view(-1, 4, 2)

    @staticmethod
    def backward(ctx, g):
        net = ctx.net
        m1, m2 = ctx.masks
        a, b = ctx.saved_tensors[:2]
        y = ctx.saved_tensors[2:10]
        xd, hidden = ctx.saved_tensors[10:12]
        B = a.shape[0]
        convs = [c for blk in net.cnn for c in (blk.layers[0], blk.layers[2])]
        l1, l2 = net.fc[2], net.fc[5]
        for q, saved in zip(net.parameters(), ctx.saved_tensors[12:]):
            if q.data_ptr() != saved.data_ptr():
                raise RuntimeError("udh model.Net: a parameter was replaced between forward and backward")
        g = g.contiguous().view(B, 8)
        gw1, gb1, gw2, gb2, gx = _hip.udh_fc_bwd(g, xd, hidden, l1.weight.detach(), l2.weight.detach(), m1, m2)
        grads = [None] * 20
        grads[16:20] = [gw1, gb1, gw2, gb2]
        g = gx.view(y[7].shape)                         # dL / d(relu output of layer 8)
        pre = False                                     # g is in front of the ReLU already (the pool kernel folds it in)
        for i in range(7, 0, -1):                       # layers 8 .. 2
            pooled_in = i in (2, 4, 6)                  # layers 3, 5, 7 read the pooled output of the layer before
            x = _hip.maxpool2(y[i - 1]) if pooled_in else y[i - 1]
            gx, gw, gb = (_conv3x3_backward_pre if pre else _conv3x3_backward)(convs[i], x, *((g,) if pre else (y[i], g)))
            grads[2 * i], grads[2 * i + 1] = gw, gb
            if pooled_in:
                g, pre = _hip.maxpool2_relu_bwd(y[i - 1], gx), True
            else:
                g, pre = gx, False
        g = _hip.elementwise(_hip.EW_ACT_BWD, g, y[0], s0=_hip.ACT_RELU)
        grads[0], grads[1] = _hip.udh_conv1_wgrad(a, b, g)
        return (None, None, None, None, None) + tuple(grads)


class Net(nn.Module):
    def __init__(self, batch_norm=False, patch_size=128):
        super().__init__()
        if batch_norm:
            raise NotImplementedError("udh model.Net: batch_norm=True is not built (no published checkpoint uses it)")
        if patch_size not in _PATCH_SIZES:
            raise ValueError(f"udh model.Net: patch_size must be one of {_PATCH_SIZES}, got {patch_size} (the reference's --patchsize 256 "
                             "default would make Linear 1 a 537 MB weight; it is not supported)")
        self.patch_size = patch_size
        self.cnn = nn.Sequential(*[Block(_WIDTHS[i], _WIDTHS[i + 1], pool=i < 3) for i in range(4)])
        side = patch_size // 8
        self.fc = nn.Sequential()
        for index, (cin, cout) in ((2, (_WIDTHS[-1] * side * side, _HIDDEN)), (5, (_HIDDEN, 8))):
            self.fc.add_module(str(index - 2), Flatten() if index == 2 else nn.ReLU())
            self.fc.add_module(str(index - 1), nn.Dropout(p=0.5))
            self.fc.add_module(str(index), nn.Linear(cin, cout))

    def _check(self, a, b):
        _hip._dev(a, "patch a")
        _hip._dev(b, "patch b")
        p = self.patch_size
        if a.shape != b.shape or a.dim() != 4 or tuple(a.shape[1:]) != (1, p, p):
            raise ValueError(f"udh model.Net: patches must be two [B,1,{p},{p}] tensors, got {tuple(a.shape)} and {tuple(b.shape)}")
        if a.shape[0] < 1:
            raise ValueError("udh model.Net: empty batch")

    def draw_masks(self, B, device):
        """The two Dropout(0.5) keep-masks (uint8) from torch's device generator."""
        k = self.fc[2].in_features
        return ((torch.rand((B, k), device=device) >= 0.5).to(torch.uint8), (torch.rand((B, _HIDDEN), device=device) >= 0.5).to(torch.uint8))

    def forward(self, a, b, dropout_masks=None):
        """delta [B,4,2].  `dropout_masks` = (m1 [B, 128 (p/8)^2], m2 [B, 1024]) uint8 keep-bits fixes the masks of training mode
        (ignored in eval mode, where Dropout is the identity)."""
        self._check(a, b)
        masks = None
        if self.training:
            masks = dropout_masks if dropout_masks is not None else self.draw_masks(a.shape[0], a.device)
            if len(masks) != 2:
                raise ValueError("udh model.Net: dropout_masks must be (m1, m2)")
        params = list(self.parameters())
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            m1, m2 = masks if masks is not None else (None, None)
            return _NetFn.apply(self, a.detach(), b.detach(), m1, m2, *params)
        with torch.no_grad():
            return _schedule(self, a, b, masks).view(-1, 4, 2)

    def get_h(self, a, b, corners):
        """inverse(get_perspective_transform(corners, corners + delta)) [B,3,3] (reference model.py:100-111); no gradient."""
        with torch.no_grad():
            return _hip.homography_from_corners(corners, self.forward(a, b).detach(), (1, 1), (1, 1))


class _PhotoFn(Function):
    @staticmethod
    def forward(ctx, delta, img_a, patch_b, corners):
        delta = delta.contiguous()
        src_hw, dst_hw = tuple(img_a.shape[-2:]), tuple(patch_b.shape[-2:])
        S = _hip.udh_photo_matrix(corners, delta, src_hw, dst_hw)
        loss = _hip.udh_photo_loss(img_a, S, patch_b)
        ctx.save_for_backward(delta, img_a, patch_b, corners, S)
        ctx.align = _hip.get_warp_align_corners()
        return loss

    @staticmethod
    def backward(ctx, g):
        delta, img_a, patch_b, corners, S = ctx.saved_tensors
        if ctx.align != _hip.get_warp_align_corners():
            raise RuntimeError("udh photometric_loss: the warp convention (set_warp_align_corners) changed between forward and backward")
        part = _hip.udh_photo_loss_bwd(img_a, S, patch_b, g.contiguous())
        return _hip.udh_photo_matrix_bwd(corners, delta, part, tuple(img_a.shape[-2:]), tuple(patch_b.shape[-2:])), None, None, None


def photometric_loss(delta, img_a, patch_b, corners):
    """mean |warp_perspective(img_a, inverse(h), patch_b.shape[-2:]) - patch_b| as a 0-d autograd tensor; delta, corners [B,4,2],
    img_a [B,1,H,W] of any size, patch_b [B,1,h,w].  The gradient flows to `delta` only."""
    for t, n in ((delta, "delta"), (img_a, "img_a"), (patch_b, "patch_b"), (corners, "corners")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"udh photometric_loss: {n} must be a CUDA (HIP) tensor -- the MI355X path has no CPU fallback")
    return _PhotoFn.apply(delta, _hip._dev(img_a.detach(), "img_a"), _hip._dev(patch_b.detach(), "patch_b"),
                          _hip._dev(corners.detach(), "corners"))
