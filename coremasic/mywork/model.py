"""UDH homography net, MI355X-native (module signature of the reference's coremasic/mywork/model.py).

`from model import Net, photometric_loss` gives the drivers the same names, and `Net()` has the reference's 20 state-dict
tensors (`cnn.{0..3}.layers.{0,2}.{weight,bias}`, `fc.{2,5}.{weight,bias}`), so a `homo_best.pth.tar` loads unchanged through
the drivers' `HomographyModel` wrapper.  `forward` is a schedule of 13 HIP launches (masic_amd/csrc/udh.hip, conv.hip), not a
graph of ATen ops:

  * the first layer reads the two patch tensors directly (no torch.cat);
  * layers 2-8 are the float32 implicit-GEMM convolution with bias and ReLU folded in;
  * the three max-pools are one small kernel each;
  * Linear(128 (p/8)^2, 1024) streams its weight once per group of <= 8 pairs and Linear(1024, 8) rides in its finishing kernel.

Always float32 operands, whatever `masic_amd.nn.set_precision` says: the matrix this net produces decides the warp masks that the
project keeps bit-compatible with the oracle ("The homography"), so it is not the place for bf16 operands.

Inference only: `forward` raises in training mode.  The reference's `train_epoch` never switches its frozen net to eval, so its
two Dropout(0.5) layers perturb `h_matrix` at random there; this port does not reproduce that -- call `.eval()`.  No autograd
graph is recorded.  There is no CPU path: tensors must live on an MI355X (`cuda`) device.
"""
import torch
import torch.nn as nn

from masic_amd import nn as _mnn
from masic_amd import ops as _hip
from masic_amd._lib import PREC_F32 as _F32

_PATCH_SIZES = (32, 64, 128)


def photometric_loss(delta, img_a, patch_b, corners):
    raise NotImplementedError("model.photometric_loss: training the homography net is a separate stage -- use udh/udh/model.py "
                              "(masic_amd.udh_train: Net, photometric_loss); this Net is inference only")


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


class Block(nn.Module):
    """Two 3x3 convolutions, each followed by ReLU, and an optional 2x2 max-pool.  The parameters sit at `layers.0` and `layers.2`
    (the state-dict contract); the ReLU and pool entries of `layers` are placeholders that keep the indices, the arithmetic
    is fused into the HIP launches of `forward`."""

    def __init__(self, inchannels, outchannels, batch_norm=False, pool=True):
        super().__init__()
        if batch_norm:
            raise NotImplementedError("model.Block: batch_norm=True is not built (no published checkpoint uses it)")
        self.pool = bool(pool)
        self.layers = nn.Sequential()
        for index, cin in ((0, inchannels), (2, outchannels)):
            self.layers.add_module(str(index), nn.Conv2d(cin, outchannels, kernel_size=3, padding=1))
            self.layers.add_module(str(index + 1), nn.ReLU())
        if self.pool:
            self.layers.add_module("4", nn.MaxPool2d(2, 2))

    def run(self, x, pair=None):
        """`pair` = (a, b): the block's two input channels given as two [B,1,H,W] tensors (the first-layer kernel, no concat);
        otherwise `x` [B,C,H,W].  A two-channel `x` is split into its planes, so a Block used on its own takes the same kernels as
        inside Net."""
        first, second = self.layers[0], self.layers[2]
        with torch.no_grad():
            if pair is None and first.in_channels == 2:
                _hip._dev(x, "block input")
                pair = (x[:, 0:1].contiguous(), x[:, 1:2].contiguous())
            if pair is not None:
                if first.in_channels != 2:
                    raise ValueError("model.Block: a patch pair feeds a block with two input channels only")
                y = _hip.udh_conv1(pair[0], pair[1], first.weight.detach(), first.bias.detach())
            else:
                y = _conv3x3_relu(first, x)
            y = _conv3x3_relu(second, y)
            return _hip.maxpool2(y) if self.pool else y

    def forward(self, x):
        return self.run(x)


class Net(nn.Module):
    def __init__(self, batch_norm=False, patch_size=128):
        super().__init__()
        if batch_norm:
            raise NotImplementedError("model.Net: batch_norm=True is not built (no published checkpoint uses it)")
        if patch_size not in _PATCH_SIZES:
            raise ValueError(f"model.Net: patch_size must be one of {_PATCH_SIZES}, got {patch_size}")
        self.patch_size = patch_size
        widths = (2, 64, 64, 128, 128)
        self.cnn = nn.Sequential(*[Block(widths[i], widths[i + 1], pool=i < 3) for i in range(4)])
        side = patch_size // 8
        # parameters at fc.2 and fc.5 (the state-dict contract); Flatten, Dropout and ReLU entries keep the indices -- in eval mode
        # the dropouts are identities, and flatten / ReLU / both linear layers run as the two launches of ops.udh_fc
        self.fc = nn.Sequential()
        for index, (cin, cout) in ((2, (widths[-1] * side * side, 1024)), (5, (1024, 8))):
            self.fc.add_module(str(index - 2), Flatten() if index == 2 else nn.ReLU())
            self.fc.add_module(str(index - 1), nn.Dropout(p=0.5))
            self.fc.add_module(str(index), nn.Linear(cin, cout))

    def _check(self, a, b):
        if self.training:
            raise RuntimeError("model.Net is inference only: call .eval() first (in training mode the reference's Dropout layers "
                               "would perturb h_matrix at random)")
        _hip._dev(a, "patch a")
        _hip._dev(b, "patch b")
        p = self.patch_size
        if a.shape != b.shape or a.dim() != 4 or tuple(a.shape[1:]) != (1, p, p):
            raise ValueError(f"model.Net: patches must be two [B,1,{p},{p}] tensors, got {tuple(a.shape)} and {tuple(b.shape)}")
        if a.shape[0] < 1:
            raise ValueError("model.Net: empty batch")

    def features(self, a, b):
        """The outputs of the four blocks (float32 NCHW)."""
        self._check(a, b)
        outs = [self.cnn[0].run(None, pair=(a, b))]
        for blk in list(self.cnn)[1:]:
            outs.append(blk.run(outs[-1]))
        return outs

    def forward(self, a, b):
        x = self.features(a, b)[-1]
        l1, l2 = self.fc[2], self.fc[5]
        with torch.no_grad():
            out = _hip.udh_fc(x, l1.weight.detach(), l1.bias.detach(), l2.weight.detach(), l2.bias.detach())
        return out.view(-1, 4, 2)

    def get_h(self, a, b, corners):
        """inverse(get_perspective_transform(corners, corners + delta)) [B,3,3] (reference model.py:100-111)."""
        return _hip.homography_from_corners(corners, self.forward(a, b), (1, 1), (1, 1))

    def h_matrix(self, a, b, corners, ori_hw, resized_hw):
        """The codec's `h_matrix` [B,3,3] from the dataset's patches and patch corners (newtrain_codec_real.py:123-129): the corners
        are shifted to the first corner, the net runs, and the inverse homography is rescaled by h_adjust from the `resized_hw`
        picture the patches were cut from to the `ori_hw` picture the codec sees."""
        delta = self.forward(a, b)
        return _hip.homography_from_corners(_hip.udh_shift_corners(corners), delta, ori_hw, resized_hw)
