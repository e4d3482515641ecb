"""MASIC stereo codec, MI355X-native (module signature of the reference's coremasic/mywork/MASIC.py).

`from MASIC import *` gives the unchanged drivers the same names (HSIC, Independent_EN, GMM_together,
mask, RateDistortionLoss, AverageMeter, ...) and `HSIC(N,M,K)` has the reference's 17 child modules and
248 state-dict tensors, but `forward` is a schedule of fused HIP launches (masic_amd/csrc/*.hip), not
a graph of ATen ops:

  * convs write straight into the channel slices that the reference builds with torch.cat
    (MASIC.py:765, 827) and fold in bias, ReLU/LeakyReLU, |y| and round();
  * the three mask2weights gates multiply inside the producing kernels' epilogues;
  * the softmax over the K mixture weights runs inside the GMM likelihood kernel;
  * `x1_hat` is warped once (the reference warps it twice with identical arguments, :821 and :833);
  * the masked context convs contract only their 12 live taps.

There is no CPU path: tensors must live on an MI355X (`cuda`) device.
"""
import math
import os

import numpy as np

import torch
import torch.nn as nn
import torch.nn.functional as F  # noqa: F401  (re-exported through `from MASIC import *`)

from compressai.entropy_models import (EntropyBottleneck, GaussianConditional, GaussianMixtureConditional,  # noqa: F401
                                       GaussianMixtureConditional_gf)
from compressai.layers import GDN, MaskedConv2d, ResidualBlock, conv3x3  # noqa: F401
from compressai.models.utils import conv, deconv, update_registered_buffers  # noqa: F401
from masic_amd import ops as _hip
from masic_amd.homography import warp_matrices as _warp_matrices
from masic_amd import autograd as _ag
from masic_amd.streams import ForkJoin as _ForkJoin
from masic_amd import fp8 as _fp8
from masic_amd import deconv as _deconv
from masic_amd import conv_s2 as _conv_s2
from masic_amd import latent as _latent
from masic_amd import d2s_layer as _d2s_layer
from masic_amd.bands import check_band_rows as _check_band_rows
from masic_amd.f16k import F16K as _F16K, F8K as _F8K

_RELU, _LEAKY, _NONE = _hip.ACT_RELU, _hip.ACT_LEAKY, _hip.ACT_NONE
_CAT_F16K = True           # F16K concat buffers in front of the heads; tests set False for the float32 concat as their reference
_HEADS_GROUPED = True      # layer i of a head's three stacks in one launch; tests set False for one launch per layer as their reference


class CompressionModel(nn.Module):
    """Two-bottleneck base class (reference MASIC.py:40-109). `parameters()` hides the entropy
    bottlenecks, `aux_parameters()` yields all of their parameters."""

    def __init__(self, entropy_bottleneck_channels, init_weights=True):
        super().__init__()
        self.entropy_bottleneck1 = EntropyBottleneck(entropy_bottleneck_channels)
        self.entropy_bottleneck2 = EntropyBottleneck(entropy_bottleneck_channels)
        if init_weights:
            self._initialize_weights()

    def aux_loss(self):
        return sum(m.loss() for m in self.modules() if isinstance(m, EntropyBottleneck))

    def _initialize_weights(self):
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
                nn.init.kaiming_normal_(m.weight)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)

    def forward(self, *args):
        raise NotImplementedError()

    def parameters(self):
        for child in self.children():
            if not isinstance(child, EntropyBottleneck):
                yield from child.parameters()

    def aux_parameters(self):
        for child in self.children():
            if isinstance(child, EntropyBottleneck):
                yield from child.parameters()

    def update(self, force=False):
        for child in self.children():
            if isinstance(child, EntropyBottleneck):
                child.update(force=force)


class RateDistortionLoss(nn.Module):
    """Single-view RD loss kept for `from MASIC import *` (reference MASIC.py:113-132); the stereo
    loss the trainers use lives in masic_amd/loss.py."""

    def __init__(self, lmbda=1e-2):
        super().__init__()
        self.lmbda = lmbda

    def forward(self, output, target):
        N, _, H, W = target.size()
        n = N * H * W
        bpp = sum(_hip.sum_log(l.contiguous()) for l in output["likelihoods"].values()) / (-math.log(2) * n)
        mse = _hip.sse(output["x_hat"].contiguous(), target.contiguous()) / target.numel()
        return {"bpp_loss": bpp.float(), "mse_loss": mse.float(), "loss": (self.lmbda * 255 ** 2 * mse + bpp).float()}


class AverageMeter:
    def __init__(self):
        self.val = self.avg = self.sum = self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


_SIDE_STREAMS = {}


def _side_streams(device, n=4):
    """Extra HIP streams per device for independent branches of the forward (captured into graphs like any other work):
    0 the right view's branch, 1 the left view's entropy chain, 2-3 the side stacks of the entropy-parameter heads when those
    are issued from the main stream (compress / decompress)."""
    key = torch.device(device).index
    pool = _SIDE_STREAMS.get(key)
    if pool is None:
        # torch hands out Stream objects round-robin from a pool of 32 HIP streams per device: two Stream objects may BE the same HIP
        # stream.  n + 1 pairwise different ones are kept, so that n remain when the caller's current stream (a stream of its own, e.g.
        # the warm-up stream of a graph capture) happens to be one of them -- a side stream that is the current stream would make the
        # forward wait for its own events (capture rule 3 of masic_amd/streams.py)
        pool, seen = [], set()
        for _ in range(64):
            s = torch.cuda.Stream(device=device)
            if s.cuda_stream not in seen:
                seen.add(s.cuda_stream)
                pool.append(s)
            if len(pool) == n + 1:
                break
        pool = _SIDE_STREAMS[key] = tuple(pool)
    cur = torch.cuda.current_stream(device).cuda_stream
    return tuple(s for s in pool if s.cuda_stream != cur)[:n]


_TRAIN_STREAMS = os.environ.get("MASIC_TRAIN_STREAMS", "1") != "0"      # 0: the whole TRAINING forward (and so its backward) on one stream (A/B timing)


def _keep_until(t, stream):
    """Tensor.record_stream for a tensor used on another stream than the one it was allocated on.  Skipped inside a HIP-graph
    capture: there every cross-stream tensor of the forward lives until all streams have joined the capturing one (and
    record_stream with a non-capturing-origin stream ends torch's capture with a fault on this ROCm)."""
    if not (torch.is_tensor(t) or isinstance(t, _F16K)):
        return
    if not torch.cuda.is_current_stream_capturing():
        t.record_stream(stream)


def _bf16_inference(*tensors):
    """True when the forward runs with bf16 operands and nothing needs a gradient: the F16K chains apply."""
    from masic_amd import nn as _mnn
    if not _mnn.reduced_precision():
        return False
    return not (torch.is_grad_enabled() and any(t.requires_grad for t in tensors))


def _f16k_chain(convs, acts, x, in_op=0, out=None, out_coff=0, gate=None, gate_c=0):
    """A chain of convolutions with the activations between them in F16K bf16 (conv_f16k.hip).  x: a float32 NCHW tensor -- |x| /
    round(x) is applied while converting it -- or the F16K that already holds that converted input (written by the layer that produced
    it, Encoder1.latent_layouts).  The last layer writes float32 NCHW (channels out_coff.. of the concat buffer `out`, optionally gated)
    -- or, with `out` an F16K view of a concat buffer, that view.  None if a layer shape has no F16K configuration."""
    B, _, H, W = x.shape
    hw = (H, W)
    for cv in convs:
        if not cv.f16k_supported(B, *hw):
            return None
        hw = cv.out_hw(*hw)
    t = x if isinstance(x, _F16K) else _F16K.from_nchw(x, in_op=in_op)
    for cv, act in zip(convs[:-1], acts):
        t = cv.run_f16k(t, act=act)
    return convs[-1].run_f16k(t, act=acts[-1], want_nchw=out is None, out=out, out_coff=out_coff, gate=gate, gate_c=gate_c)


def _pair_conv(conv, xa, xb, gdn_in=None, gdn_out=None):
    """The 6 -> 3 k5 s1 (transposed) convolution of encoder2 / decoder2 on two 3-channel sources with the neighbouring
    3-channel GDN fused (masic_conv5s1_pair_fwd); float32 arithmetic in the order of the separate kernels."""
    B, _, H, W = xa.shape
    desc = conv._desc((B, 6, H, W))
    def g(m):
        return None if m is None else (m.beta.detach(), m.gamma.detach().contiguous(), m.inverse)
    bm = (gdn_in or gdn_out).beta_min if (gdn_in or gdn_out) is not None else 1e-6
    return _hip.conv5s1_pair(xa, xb, conv.packed_weight(desc), None if conv.bias is None else conv.bias.detach(),
                             gdn_in=g(gdn_in), gdn_out=g(gdn_out), beta_min=bm)


def _gdn_f16k(gdn, x):
    return _hip.gdn_f16k(x, gdn.beta.detach(), gdn.gamma.detach(), inverse=gdn.inverse, beta_min=gdn.beta_min)


def _own_kernel_takes(kernel, cv, t, *gdn):
    """does the own-layer module `kernel` (masic_amd.conv_s2 / deconv with the layer's GDN, latent / d2s_layer without: conv_f16k's packs,
    conv_f16k's bits) take the layer cv on the F16K t?  Where not, the caller keeps the conv_f16k method that kernel.run stands for."""
    return t.whole and kernel.supported(cv, *gdn, t.B, t.H, t.W) and kernel.preferred(cv, t.B, t.H, t.W)


def _analysis_f16k(owner, x, layouts=None):
    """conv+GDN x3 -> conv of the analysis transform `owner` on the float32 NCHW image `x` with bf16 operands: every GDN runs in
    the epilogue of the convolution that feeds it and the 128-channel activations stay in F16K bf16 in between
    (conv_f16k.hip). None if a shape has no such configuration (the caller then takes the NCHW path).
    layouts (keyword arguments of Conv2d.run_f16k_multi): the last layer writes the latent once in every layout its consumers read
    and the dict of those tensors is returned instead of the float32 latent -- None (nothing launched) where that form does not
    apply: fp8 operands / calibration, a shape without the multi-output configuration.
    fp8 mode (masic_amd/fp8.py; `owner` calibrated): the two 128 -> 128 layers take fp8 operands -- the first layer and the
    second write F8K, the third writes F16K for the latent-producing last layer, which stays bf16."""
    from masic_amd import nn as _mnn
    convs = (owner.g_a_conv1, owner.g_a_conv2, owner.g_a_conv3, owner.g_a_conv4)
    gdns = (owner.g_a_gdn1, owner.g_a_gdn2, owner.g_a_gdn3)
    B, C, H, W = x.shape
    c1 = convs[0]
    if (C, c1.out_channels, tuple(c1.kernel_size), tuple(c1.stride), tuple(c1.padding)) != (3, 128, (5, 5), (2, 2), (2, 2)):
        return None
    sizes = [((H - 1) // 2 + 1, (W - 1) // 2 + 1)]
    for cv in convs[1:]:
        if not cv.f16k_supported(B, *sizes[-1]):
            return None
        sizes.append(cv.out_hw(*sizes[-1]))
    if convs[1].out_channels != 128 or convs[2].out_channels != 128:
        return None
    b1 = None if c1.bias is None else c1.bias.detach()
    sc = _fp8.scales(owner)
    if layouts is not None and (sc is not None or _mnn._FP8 or _fp8.recording() or not convs[3].f16k_multi_supported(B, *sizes[2])):
        return None
    if sc is not None and convs[1].f8k_supported(B, *sizes[0]) and convs[2].f8k_supported(B, *sizes[1]):
        t8 = _hip.conv_a_gdn_f8k(x, c1.packed_first_layer_weight(), b1, (_mnn.packed_gdn_f16k(gdns[0]), gdns[0].inverse), sc["a1"])[0]
        t = convs[1].run_f8k(_F8K(t8, B, 128, *sizes[0], sc["a1"]), gdn=gdns[1], out="f8k", out_scale=sc["a2"])
        t = convs[2].run_f8k(t, gdn=gdns[2], out="f16k")
        return convs[3].run_f16k(t, want_nchw=True)
    t = _F16K(_hip.conv_a_gdn_f16k(x, c1.packed_first_layer_weight(), b1, (_mnn.packed_gdn_f16k(gdns[0]), gdns[0].inverse))[0], B, 128, *sizes[0], 128, 0)
    _fp8.record(owner, "a1", t.buf)
    for i in (1, 2):
        # g_a_conv2 / g_a_conv3 (128 -> 128): conv_s2_gdn_f16k
        t = _conv_s2.run(convs[i], gdns[i], t) if _own_kernel_takes(_conv_s2, convs[i], t, gdns[i]) else convs[i].run_f16k(t, gdn=gdns[i])
        if i == 1:
            _fp8.record(owner, "a2", t.buf)
    if layouts is not None:
        # g_a_conv4 (128 -> 192): conv_s2_latent_f16k where the launch is large enough for it, else conv_f16k_multi; the same bits
        if _own_kernel_takes(_latent, convs[3], t):
            return _latent.run(convs[3], t, **layouts)
        return convs[3].run_f16k_multi(t, **layouts)
    return convs[3].run_f16k(t, want_nchw=True)


# ------------------------------------------------------------------------------------------ sub-networks
class encode_hyper(nn.Module):
    """|y| -> conv5x5 s1 -> ReLU -> conv5x5 s2 -> ReLU -> conv5x5 s2 (reference :170-187)."""

    def __init__(self, N, M):
        super().__init__()
        self.encode_hyper = nn.Sequential(
            conv(M, N, kernel_size=5, stride=1), nn.ReLU(inplace=True),
            conv(N, N, kernel_size=5), nn.ReLU(inplace=True),
            conv(N, N, kernel_size=5))

    def forward(self, y, abs16=None):
        """abs16: bf16(|y|) as an F16K, where the layer that produced y wrote it (the bf16 eval forward)."""
        s = self.encode_hyper
        if _bf16_inference(y, s[0].weight):
            z = _f16k_chain((s[0], s[2], s[4]), (_RELU, _RELU, _NONE), y if abs16 is None else abs16, in_op=_hip.INOP_ABS)
            if z is not None:
                return z
        t = s[0].run(y, in_op=_hip.INOP_ABS, act=_RELU)
        t = s[2].run(t, act=_RELU)
        return s[4].run(t)


class _GmmHeads(nn.Module):
    """Three 3-layer 1x1 stacks -> sigma (ReLU), means, mixture-weight logits (reference :330-468)."""

    def _branch(self, seq, x, acts):
        t = seq[0].run(x, act=acts[0])
        t = seq[2].run(t, act=acts[1])
        return seq[4].run(t, act=acts[2])

    def _branch_f16k(self, seq, x, acts):
        """The same three layers as bf16 GEMMs on the whole F16K x; activations between them stay in the F16K layout on the device."""
        t, (B, _, H, W) = x.buf, x.shape
        for i, (layer, act) in enumerate(zip((seq[0], seq[2], seq[4]), acts)):
            last = i == 2
            if layer.in_channels % 16 == 0 and layer.out_channels % 32 == 0:          # both operands staged by DMA
                t = _hip.gemm_f16k(t, layer.packed_gemm_dma_weight(), layer.bias.detach(), B, layer.in_channels, layer.out_channels,
                                   H, W, act, want_nchw=last)
            else:                                                                      # register-streamed kernel (any width)
                t = _hip.gemm1x1_bf16(t, layer.packed_gemm_weight(), layer.bias.detach(), B, layer.in_channels, layer.out_channels,
                                      H, W, act, want_nchw=last)
        return t

    def _branch_f8k(self, seq, x, sc, tag, acts):
        """fp8 mode: the first two layers with fp8 operands (x an F8K; the first writes F8K, the second F16K), the last -- the one
        that produces sigma / means / weight logits -- with bf16 operands."""
        l0, l1, l2 = seq[0], seq[2], seq[4]
        x8, (B, _, H, W) = x.buf, x.shape
        wp, ws = l0.packed_gemm_f8k_weight(sc["c"])
        t = _hip.gemm_f8k(x8, wp, ws, l0.bias.detach(), B, l0.in_channels, l0.out_channels, H, W, acts[0], out="f8k", out_scale=sc[tag])
        wp, ws = l1.packed_gemm_f8k_weight(sc[tag])
        t = _hip.gemm_f8k(t, wp, ws, l1.bias.detach(), B, l1.in_channels, l1.out_channels, H, W, acts[1], out="f16k")
        return _hip.gemm_f16k(t, l2.packed_gemm_dma_weight(), l2.bias.detach(), B, l2.in_channels, l2.out_channels, H, W, acts[2], want_nchw=True)

    _STACKS = (("gmm_sigma", "h_sigma", (_RELU, _RELU, _RELU)), ("gmm_means", "h_means", (_LEAKY, _LEAKY, _NONE)),
               ("gmm_weights", "h_weights", (_LEAKY, _LEAKY, _NONE)))

    def _grouped_heads_ok(self):
        return all(getattr(self, n)[i].in_channels % 16 == 0 and getattr(self, n)[i].out_channels % 32 == 0
                   for n, _, _ in self._STACKS for i in (0, 2, 4))

    def _heads_grouped(self, x, sc):
        """sigma, means, weight logits with layer i of the three stacks in one launch each (_hip.gemm_f16k_group); x: the whole F16K
        input and sc None (bf16 operands, as _branch_f16k), or an F8K and the fp8 scales of this head (first two layers with fp8
        operands, as _branch_f8k)."""
        B, _, H, W = x.shape
        t = [x.buf] * 3
        for i in range(3):
            layers = []
            for k, (name, tag, acts) in enumerate(self._STACKS):
                layer = getattr(self, name)[2 * i]
                L = dict(x=t[k], bias=layer.bias.detach(), Cin=layer.in_channels, Cout=layer.out_channels, act=acts[i],
                         out="nchw" if i == 2 else "f16k")
                if sc is not None and i < 2:
                    L["wp"], L["ws"] = layer.packed_gemm_f8k_weight(sc["c"] if i == 0 else sc[tag])
                    if i == 0:
                        L["out"], L["out_scale"] = "f8k", sc[tag]
                else:
                    L["wp"] = layer.packed_gemm_dma_weight()
                layers.append(L)
            t = _hip.gemm_f16k_group(layers, B, H, W)
        return tuple(t)

    def _f8k_heads_ok(self):
        return all(seq[i].in_channels % 32 == 0 and seq[i].out_channels % 32 == 0 for seq in (self.gmm_sigma, self.gmm_means, self.gmm_weights) for i in (0, 2)) \
            and all(seq[4].in_channels % 16 == 0 and seq[4].out_channels % 32 == 0 for seq in (self.gmm_sigma, self.gmm_means, self.gmm_weights))

    def heads(self, x, parallel=True):
        """x: float32 NCHW, or the concat as a whole F16K (HSIC's bf16 eval forward builds it there).
        parallel: the means / weights stacks on two side streams forked from the current one.  Callers that are themselves on
        a side stream pass False: a side stream that forks further streams (or a stream waiting for its own event) ends a
        HIP-graph capture on this ROCm with a fault in hipStreamEndCapture (measured; torch 2.10 / ROCm 7)."""
        from masic_amd import nn as _mnn
        if isinstance(x, _F16K):
            if not x.whole:
                raise RuntimeError(f"_GmmHeads.heads: the grouped GEMMs read a whole buffer, not {x!r}")
            return self._heads_grouped(x, None)
        if _mnn.reduced_precision() and not (torch.is_grad_enabled() and (x.requires_grad or self.gmm_sigma[0].weight.requires_grad)):
            B, _, H, W = x.shape
            sc = _fp8.scales(self)
            use_f8 = sc is not None and self._f8k_heads_ok()
            if use_f8:
                xv = _F8K(_hip.nchw_to_f8k(x, sc["c"]), *x.shape, sc["c"])          # quantised once, read by the three stacks
                branch = lambda seq, tag, acts: self._branch_f8k(seq, xv, sc, tag, acts)
            else:
                xv = _F16K.from_nchw(x)          # converted once, read by the three stacks
                xf = xv.buf

                def branch(seq, tag, acts):
                    if _fp8.recording():
                        _fp8.record(self, "c", x)
                        l0 = seq[0]
                        _fp8.record(self, tag, _hip.gemm_f16k(xf, l0.packed_gemm_dma_weight(), l0.bias.detach(), B, l0.in_channels, l0.out_channels, H, W, acts[0])
                                    if l0.in_channels % 16 == 0 and l0.out_channels % 32 == 0 else
                                    _hip.gemm1x1_bf16(xf, l0.packed_gemm_weight(), l0.bias.detach(), B, l0.in_channels, l0.out_channels, H, W, acts[0]))
                    return self._branch_f16k(seq, xv, acts)
            # layer i of the three stacks as ONE launch (640 ... 864 workgroups instead of 3 x 192 ... 288): no streams needed
            if _HEADS_GROUPED and not _fp8.recording() and self._grouped_heads_ok():
                return self._heads_grouped(xv, sc if use_f8 else None)
            # the three stacks are independent and each of their GEMMs fills about one wave of workgroups: run them on
            # three HIP streams so that their tails overlap
            if not parallel:
                return (branch(self.gmm_sigma, "h_sigma", (_RELU, _RELU, _RELU)),
                        branch(self.gmm_means, "h_means", (_LEAKY, _LEAKY, _NONE)),
                        branch(self.gmm_weights, "h_weights", (_LEAKY, _LEAKY, _NONE)))
            fj = _ForkJoin()               # raises (instead of faulting in hipStreamEndCapture) if we are on a side stream of a capture
            cur = fj.main
            side = _side_streams(x.device)[2:4]
            outs = [None, None, None]
            for i, (st, (seq, tag, acts)) in enumerate(zip(side, ((self.gmm_means, "h_means", (_LEAKY, _LEAKY, _NONE)),
                                                                  (self.gmm_weights, "h_weights", (_LEAKY, _LEAKY, _NONE))))):
                fj.fork(st)
                with fj.on(st):
                    outs[i + 1] = branch(seq, tag, acts)
            outs[0] = branch(self.gmm_sigma, "h_sigma", (_RELU, _RELU, _RELU))
            for st in side:
                fj.join(st)
            for t in outs[1:] + [xv.buf]:
                _keep_until(t, cur)
            return tuple(outs)
        if torch.is_grad_enabled() and _ag.gmm_heads_supported(self, x):
            return _ag.gmm_heads(self, x)             # bf16-mode training: the nine layers as one autograd node on F16K
        sigma = self._branch(self.gmm_sigma, x, (_RELU, _RELU, _RELU))
        means = self._branch(self.gmm_means, x, (_LEAKY, _LEAKY, _NONE))
        logits = self._branch(self.gmm_weights, x, (_LEAKY, _LEAKY, _NONE))
        return sigma, means, logits

    def forward(self, x):
        sigma, means, logits = self.heads(x)
        return sigma, means, _hip.softmax_k(logits, self.K)


class gmm_hyper_y1_same_resolution(_GmmHeads):
    """Left-view heads: the first two layers of each branch are ConvTranspose2d(k=1) (reference :338-376)."""

    def __init__(self, N, M, K):
        super().__init__()
        self.N, self.M, self.K = N, M, K
        self.gmm_sigma = nn.Sequential(
            deconv(4 * M, 6 * M, kernel_size=1, stride=1), nn.ReLU(inplace=True),
            deconv(6 * M, 4 * M, kernel_size=1, stride=1), nn.ReLU(inplace=True),
            conv(4 * M, M * K, kernel_size=1, stride=1), nn.ReLU(inplace=True))
        self.gmm_means = nn.Sequential(
            deconv(4 * M, 6 * M, kernel_size=1, stride=1), nn.LeakyReLU(inplace=True),
            deconv(6 * M, 4 * M, kernel_size=1, stride=1), nn.LeakyReLU(inplace=True),
            conv(4 * M, M * K, kernel_size=1, stride=1))
        self.gmm_weights = nn.Sequential(
            deconv(4 * M, 6 * M, kernel_size=1, stride=1), nn.LeakyReLU(inplace=True),
            deconv(6 * M, M * K, kernel_size=1, stride=1), nn.LeakyReLU(inplace=True),
            conv(M * K, M * K, kernel_size=1, stride=1))


class gmm_hyper_y2_same_resolution(_GmmHeads):
    """Right-view heads on the 5M-channel gated concat (reference :399-468)."""

    def __init__(self, N, M, K):
        super().__init__()
        self.N, self.M, self.K = N, M, K
        self.gmm_sigma = nn.Sequential(
            conv(5 * M, 6 * M, kernel_size=1, stride=1), nn.ReLU(inplace=True),
            conv(6 * M, 4 * M, kernel_size=1, stride=1), nn.ReLU(inplace=True),
            conv(4 * M, M * K, kernel_size=1, stride=1), nn.ReLU(inplace=True))
        self.gmm_means = nn.Sequential(
            conv(5 * M, 6 * M, kernel_size=1, stride=1), nn.LeakyReLU(inplace=True),
            conv(6 * M, 4 * M, kernel_size=1, stride=1), nn.LeakyReLU(inplace=True),
            conv(4 * M, M * K, kernel_size=1, stride=1))
        self.gmm_weights = nn.Sequential(
            conv(5 * M, 6 * M, kernel_size=1, stride=1), nn.LeakyReLU(inplace=True),
            conv(6 * M, M * K, kernel_size=1, stride=1), nn.LeakyReLU(inplace=True),
            conv(M * K, M * K, kernel_size=1, stride=1))


class mask2weights(nn.Module):
    """Right-view mask -> Kw softmax-normalised gate maps at latent resolution (reference :472-506)."""

    def __init__(self, N, M, Kw):
        super().__init__()
        self.maskconv = nn.Sequential(
            conv(1, 3, kernel_size=3, stride=2), nn.ReLU(inplace=True),
            conv(3, 6, kernel_size=3), nn.ReLU(inplace=True),
            conv(6, 6, kernel_size=3), nn.ReLU(inplace=True),
            conv(6, 3, kernel_size=3))
        self.N, self.M, self.Kw = N, M, Kw

    def forward(self, m):
        s = self.maskconv
        t = s[0].run(m, act=_RELU)
        t = s[2].run(t, act=_RELU)
        t = s[4].run(t, act=_RELU)
        return s[6].run(t, act=_hip.ACT_SOFTMAX_C)


def _synthesis_f16k(dec, y_hat):
    """The synthesis transform deconv+IGDN x3 -> deconv(128 -> 3) with bf16 operands: F16K activations in between, the
    inverse GDNs fused into the transposed convolutions, the last layer as a 3x3 convolution with a depth-to-space store.
    y_hat: float32 NCHW, or an F16K (written by the analysis transform, _analysis_f16k(layouts=...)).
    Returns the float32 NCHW output of g_s_conv4, or None if a shape is unsupported."""
    B, _, H, W = y_hat.shape
    convs = (dec.g_s_conv1, dec.g_s_conv2, dec.g_s_conv3)
    gdns = (dec.g_s_gdn1, dec.g_s_gdn2, dec.g_s_gdn3)
    sizes = [(H, W)]
    for cv in convs:
        if cv.out_channels != 128 or not cv.f16k_supported(B, *sizes[-1]):
            return None
        sizes.append(cv.out_hw(*sizes[-1]))
    if not dec.g_s_conv4.d2s_supported(B, *sizes[3]):
        return None
    t = y_hat if isinstance(y_hat, _F16K) else _F16K.from_nchw(y_hat)
    sc = _fp8.scales(dec)
    if sc is not None and convs[1].f8k_supported(B, *sizes[1]) and convs[2].f8k_supported(B, *sizes[2]):
        # fp8 mode: g_s_conv1 keeps bf16 operands (its input are the integer symbols) and writes F8K for the two 128 -> 128 layers
        t = convs[0].run_f16k_f8out(t, sc["d1"], gdn=gdns[0])
        t = convs[1].run_f8k(t, gdn=gdns[1], out="f8k", out_scale=sc["d2"])
        t = convs[2].run_f8k(t, gdn=gdns[2], out="f16k")
        return dec.g_s_conv4.run_f16k_d2s(t)
    for i in range(3):
        # g_s_conv2 / g_s_conv3 (128 -> 128): deconv_igdn_f16k
        t = _deconv.run(convs[i], gdns[i], t) if _own_kernel_takes(_deconv, convs[i], t, gdns[i]) else convs[i].run_f16k(t, gdn=gdns[i])
        if i < 2:
            _fp8.record(dec, "d%d" % (i + 1), t.buf)
    # g_s_conv4 (128 -> 3): d2s_layer_f16k where it takes the shape (masic_amd.d2s_layer: conv_f16k's pack, conv_f16k's bits)
    if _own_kernel_takes(_d2s_layer, dec.g_s_conv4, t):
        return _d2s_layer.run(dec.g_s_conv4, t)
    return dec.g_s_conv4.run_f16k_d2s(t)


class Encoder1(nn.Module):
    """Left analysis transform (reference :510-531)."""

    def __init__(self, N, M, **kwargs):
        super().__init__()
        self.g_a_conv1 = conv(3, N)
        self.g_a_gdn1 = GDN(N)
        self.g_a_conv2 = conv(N, N)
        self.g_a_gdn2 = GDN(N)
        self.g_a_conv3 = conv(N, N)
        self.g_a_gdn3 = GDN(N)
        self.g_a_conv4 = conv(N, M)

    def forward(self, x):
        g1 = self.g_a_gdn1(self.g_a_conv1(x))
        g2 = self.g_a_gdn2(self.g_a_conv2(g1))
        g3 = self.g_a_gdn3(self.g_a_conv3(g2))
        return self.g_a_conv4(g3), g1, g2, g3

    def latent(self, x):
        """forward(x)[0]; with bf16 operands and no autograd the intermediate activations stay in F16K."""
        if _bf16_inference(x, self.g_a_conv1.weight):
            y = _analysis_f16k(self, x.contiguous())
            if y is not None:
                return y
        return self.forward(x)[0]

    def latent_layouts(self, x, **layouts):
        """latent(x) written once in the layouts its consumers read (bf16 eval forward; _analysis_f16k(layouts=...)): a dict of the
        tensors, or None where that form does not apply -- the caller then uses latent() and the stand-alone conversions."""
        if _bf16_inference(x, self.g_a_conv1.weight):
            return _analysis_f16k(self, x.contiguous(), layouts=layouts)
        return None

    def latent_train(self, x):
        """forward(x)[0] inside the training graph: in the bf16-operand mode ONE node that runs the DMA-staged inference kernels and
        keeps bf16 activations for its backward (masic_amd/autograd.py: AnalysisFn); otherwise the per-layer nodes."""
        if _ag.analysis_supported(self, x):
            return _ag.analysis(self, x)
        return self.forward(x)[0]


class Decoder1(nn.Module):
    """Left synthesis transform (reference :533-554)."""

    def __init__(self, N, M, **kwargs):
        super().__init__()
        self.g_s_conv1 = deconv(M, N)
        self.g_s_gdn1 = GDN(N, inverse=True)
        self.g_s_conv2 = deconv(N, N)
        self.g_s_gdn2 = GDN(N, inverse=True)
        self.g_s_conv3 = deconv(N, N)
        self.g_s_gdn3 = GDN(N, inverse=True)
        self.g_s_conv4 = deconv(N, 3)

    def forward(self, y_hat):
        g1 = self.g_s_gdn1(self.g_s_conv1(y_hat))
        g2 = self.g_s_gdn2(self.g_s_conv2(g1))
        g3 = self.g_s_gdn3(self.g_s_conv3(g2))
        return self.g_s_conv4(g3), g1, g2, g3

    def reconstruct(self, y_hat):
        """forward(y_hat)[0]; F16K chain with bf16 operands and no autograd.  y_hat: float32 NCHW, or an F16K holding it -- then the
        result is None where the F16K chain does not apply (the caller passes the float32 tensor instead)."""
        if isinstance(y_hat, _F16K):
            return _synthesis_f16k(self, y_hat) if _bf16_inference(self.g_s_conv1.weight) else None
        if _bf16_inference(y_hat, self.g_s_conv1.weight):
            x_hat = _synthesis_f16k(self, y_hat)
            if x_hat is not None:
                return x_hat
        return self.forward(y_hat)[0]

    def reconstruct_train(self, y_hat):
        if _ag.synthesis_supported(self, y_hat):
            return _ag.synthesis(self, y_hat)
        return self.forward(y_hat)[0]


class Encoder2(nn.Module):
    """Right analysis transform conditioned on the warped left view (reference :556-585)."""

    def __init__(self, N, M, **kwargs):
        super().__init__()
        self.pre_conv = conv(6, 3, stride=1)
        self.pre_gdn = GDN(3)
        self.g_a_conv1 = conv(3, N)
        self.g_a_gdn1 = GDN(N)
        self.g_a_conv2 = conv(N, N)
        self.g_a_gdn2 = GDN(N)
        self.g_a_conv3 = conv(N, N)
        self.g_a_gdn3 = GDN(N)
        self.g_a_conv4 = conv(N, M)

    def forward(self, x1_warp, x2):
        if not (torch.is_grad_enabled() and (x1_warp.requires_grad or x2.requires_grad or self.pre_conv.weight.requires_grad)):
            return self.forward_views(x1_warp, x2)
        return self.forward_pair(_ag.cat(x1_warp, x2))

    def forward_views(self, x1_warp, x2, layouts=None):
        """Inference: pre_conv on [x1_warp | x2] read from the two tensors (no torch.cat) with pre_gdn in its epilogue.
        layouts: as Encoder1.latent_layouts -- the dict of latent layouts where that form applies, else the float32 latent."""
        t = _pair_conv(self.pre_conv, x1_warp.contiguous(), x2.contiguous(), gdn_out=self.pre_gdn)
        if layouts is not None and _bf16_inference(t, self.g_a_conv1.weight):
            lay = _analysis_f16k(self, t, layouts=layouts)
            if lay is not None:
                return lay
        return self._analysis(t)

    def forward_pair(self, pair):
        return self._analysis(self.pre_gdn(self.pre_conv(pair)))

    def _analysis(self, t):
        if _bf16_inference(t, self.g_a_conv1.weight):
            y = _analysis_f16k(self, t)
            if y is not None:
                return y
        if torch.is_grad_enabled() and _ag.analysis_supported(self, t):
            return _ag.analysis(self, t)
        t = self.g_a_gdn1(self.g_a_conv1(t))
        t = self.g_a_gdn2(self.g_a_conv2(t))
        t = self.g_a_gdn3(self.g_a_conv3(t))
        return self.g_a_conv4(t)


class Decoder2(nn.Module):
    """Right synthesis transform; its tail fuses the warped left reconstruction (reference :587-622)."""

    def __init__(self, N, M, **kwargs):
        super().__init__()
        self.g_s_conv1 = deconv(M, N)
        self.g_s_gdn1 = GDN(N, inverse=True)
        self.g_s_conv2 = deconv(N, N)
        self.g_s_gdn2 = GDN(N, inverse=True)
        self.g_s_conv3 = deconv(N, N)
        self.g_s_gdn3 = GDN(N, inverse=True)
        self.g_s_conv4 = deconv(N, 3)
        self.after_gdn = GDN(3, inverse=True)
        self.after_conv = deconv(6, 3, stride=1)

    def forward(self, y_hat, x1_hat_warp):
        """y_hat: float32 NCHW, or (bf16 eval forward) round(y2) as an F16K where the analysis transform wrote it -- the result is
        then None where the F16K chain does not apply (the caller quantises to float32 and calls again)."""
        if isinstance(y_hat, _F16K):
            t = _synthesis_f16k(self, y_hat) if _bf16_inference(x1_hat_warp, self.g_s_conv1.weight) else None
            if t is None:
                return None
        else:
            t = _synthesis_f16k(self, y_hat) if _bf16_inference(y_hat, self.g_s_conv1.weight) else None
        if t is None and torch.is_grad_enabled() and _ag.synthesis_supported(self, y_hat):
            t = _ag.synthesis(self, y_hat)
        if t is None:
            t = self.g_s_gdn1(self.g_s_conv1(y_hat))
            t = self.g_s_gdn2(self.g_s_conv2(t))
            t = self.g_s_gdn3(self.g_s_conv3(t))
            t = self.g_s_conv4(t)
        if not (torch.is_grad_enabled() and (t.requires_grad or x1_hat_warp.requires_grad or self.after_conv.weight.requires_grad)):
            # inference: after_gdn applied while after_conv stages its first source; [t | x1_hat_warp] read in place
            return _pair_conv(self.after_conv, t.contiguous(), x1_hat_warp.contiguous(), gdn_in=self.after_gdn)
        t = self.after_gdn(t)
        return self.after_conv(_ag.cat(t, x1_hat_warp))


def mask(im1, H_inv):
    """Validity masks of the left->right->left warp (reference :627-649). As there, the masks are NOT
    binarised (the reference discards its torch.where results) and keep bilinear border values."""
    B, _, h, w = im1.shape
    m_fwd, m_back = _warp_matrices(H_inv, (h, w), (h, w), want_inverse=True)
    mask_r = _hip.warp_perspective(None, m_fwd, (h, w), ones_like=(B, h, w))
    mask_l = _hip.warp_perspective(mask_r, m_back, (h, w))
    return mask_r, mask_l


class HSIC(CompressionModel):
    """Homography-aware stereo image codec (reference :652-851)."""

    def __init__(self, N=128, M=192, K=5, **kwargs):
        super().__init__(entropy_bottleneck_channels=N, **kwargs)
        self.gaussian1 = GaussianMixtureConditional_gf(K=K)
        self.gaussian2 = GaussianMixtureConditional_gf(K=K)
        self.N, self.M, self.K = int(N), int(M), int(K)
        self.encoder1 = Encoder1(N, M)
        self.encoder2 = Encoder2(N, M)
        self.decoder1 = Decoder1(N, M)
        self.decoder2 = Decoder2(N, M)
        self._h_a1 = encode_hyper(N=N, M=M)
        self._h_a2 = encode_hyper(N=N, M=M)

        def up():
            return nn.Sequential(
                deconv(N, M, stride=2, kernel_size=5), nn.LeakyReLU(inplace=True),
                deconv(M, M * 3 // 2, stride=2, kernel_size=5), nn.LeakyReLU(inplace=True),
                conv(M * 3 // 2, M * 2, stride=1, kernel_size=3))

        self.h_s1_up = up()
        self.h_s2_up = up()
        self.context_prediction1 = MaskedConv2d(M, 2 * M, kernel_size=5, padding=2, stride=1)
        self.context_prediction2 = MaskedConv2d(M, 2 * M, kernel_size=5, padding=2, stride=1)
        self._h_s1_same_resolution = gmm_hyper_y1_same_resolution(N=N, M=M, K=K)
        self._h_s2_same_resolution = gmm_hyper_y2_same_resolution(N=N, M=M, K=K)
        self.mask2weights_unit = mask2weights(N=N, M=M, Kw=3)
        self._band_rows = 0
        # NB: as in the reference, _initialize_weights() ran inside super().__init__() before any of
        # these children existed, so the convs keep torch's default initialisation.

    @property
    def band_rows(self):
        """The row bands of the file this model ESTIMATES (DESIGN.md section 8.1 "Row bands in the model"): with S > 0 every context model
        evaluated outside the coder -- forward in all its modes, the training graph, _forward_refine, _eval_from_latents -- is the banded
        one of `compress(..., band_rows=S)`, whose bands of S latent rows do not see across their top edge.  0 (default): the unbanded
        model, today's launches.  A plain attribute: no constructor argument, not in the state dict; how a file is CODED stays the
        band_rows argument of compress / compress_batch.  masic_amd.bands.model_band_rows sets and restores it."""
        return self.__dict__.get("_band_rows", 0)

    @band_rows.setter
    def band_rows(self, value):
        self._band_rows = _check_band_rows(value, "HSIC.band_rows")

    def _model_bands(self, h):
        """self.band_rows as it cuts a latent of h rows: 0 where that is one band.  fp8 operands are refused: their scales were calibrated
        on whole latents and the folded path has not been validated against them."""
        S = self.band_rows
        if not 0 < S < h:
            return 0
        from masic_amd import nn as _mnn
        if _mnn._FP8 or _fp8.recording():
            raise NotImplementedError(f"HSIC.band_rows = {S}: the band-aware entropy model runs with float32 or bf16 operands only; with fp8 operands "
                                      "it is refused instead of returning the unbanded estimate (set band_rows = 0 or leave the fp8 mode)")
        return S

    # `_quantize` / `_standardized_cumulative` duplicates of the reference (:710-742) for callers that
    # reach into the model
    def _quantize(self, inputs, mode, means=None):
        return self.gaussian1._quantize(inputs, mode, means)

    def _standardized_cumulative(self, inputs):
        return self.gaussian1._standardized_cumulative(inputs)

    @staticmethod
    def _slice(cat32, cat16, coff, C):
        """Channels [coff, coff + C) of a head's concat as the `out` arguments of the layer that writes them: a view of the F16K buffer
        where there is one, else the float32 buffer and the offset."""
        return dict(out=cat32, out_coff=coff) if cat16 is None else dict(out=cat16.channels(coff, C))

    def _hyper_up(self, seq, z_hat, out=None, out_coff=0, gate=None, gate_c=0):
        """out: the float32 concat buffer (written at out_coff) or an F16K view of the F16K one; None: a fresh float32 tensor."""
        if _bf16_inference(z_hat, seq[0].weight):
            # the two small transposed layers (8^2 -> 16^2 -> 32^2: a few dozen workgroups) are quicker on the register-streamed
            # NCHW kernel; the 3x3 288 -> 384 layer at 32^2 on the F16K one (measured: 21 + 58 + 46 us against 47 + 92 + 46)
            t = seq[0].run(z_hat, act=_LEAKY)
            if seq[2].f16k_out_supported(t.shape) and seq[4].f16k_supported(t.shape[0], *seq[2].out_hw(*t.shape[2:])):
                # the second layer stores bf16 records for the 3x3 layer itself: no float32 tensor and no conversion pass in between
                return _f16k_chain((seq[4],), (_NONE,), seq[2].run_f16k_out(t, act=_LEAKY), out=out, out_coff=out_coff, gate=gate, gate_c=gate_c)
            t = seq[2].run(t, act=_LEAKY)
            r = _f16k_chain((seq[4],), (_NONE,), t, out=out, out_coff=out_coff, gate=gate, gate_c=gate_c)
            if r is not None:
                return r
            if isinstance(out, _F16K):           # a layer without an F16K configuration: its float32 result converted into the slice
                return out.fill_from_nchw(seq[4].run(t, gate=gate, gate_c=gate_c))
            return seq[4].run(t, out=out, out_coff=out_coff, gate=gate, gate_c=gate_c)
        t = seq[0].run(z_hat, act=_LEAKY)
        t = seq[2].run(t, act=_LEAKY)
        return seq[4].run(t, out=out, out_coff=out_coff, gate=gate, gate_c=gate_c)

    def _context(self, ctx, y, out, out_coff=0, gate=None, gate_c=0, round16=None, band_rows=0):
        """Eval-mode context model: masked conv of round(y) into a slice of the concat buffer (`out` as in _hyper_up; optionally gated).
        round16: bf16(round(y)) as an F16K, where the layer that produced y wrote it.  band_rows: the row bands of the bitstream coder
        (_context_bands)."""
        if 0 < band_rows < y.shape[-2]:
            return self._context_bands(ctx, y, out, out_coff, gate, gate_c, band_rows)
        if _bf16_inference(y, ctx.weight):
            ctx.zero_masked_taps()
            r = _f16k_chain((ctx,), (_NONE,), y if round16 is None else round16, in_op=_hip.INOP_ROUND, out=out, out_coff=out_coff, gate=gate, gate_c=gate_c)
            if r is not None:
                return r
        if isinstance(out, _F16K):
            return out.fill_from_nchw(ctx.run(y, in_op=_hip.INOP_ROUND, gate=gate, gate_c=gate_c))
        return ctx.run(y, in_op=_hip.INOP_ROUND, out=out, out_coff=out_coff, gate=gate, gate_c=gate_c)

    def _context_bands(self, ctx, y, out, out_coff, gate, gate_c, S):
        """The context model of the full-latent parameter form with the latent cut into bands of S rows that do not see across their top
        edge (masic_amd.codec.wavefront_steps): the bands as images of one call of _context.  h is padded to a multiple of S with zero
        rows at the bottom (the mask is causal: they reach no row above them), [B, M, T S, w] is folded to [B T, M, S, w], the
        convolution's own zero padding above each image is the band top, and the rows go back in place -- one launch each way
        (masic_amd/bandfold.py).  The gate multiplies in float32 as in the layers' epilogues.  Encoder and decoder both come through
        here, so their tables agree; so does the model's own estimate (HSIC.band_rows)."""
        return _ag.banded_context(ctx, y, S, call=lambda t: self._context(ctx, t, None), out=out, out_coff=out_coff, gate=gate, gate_c=gate_c)

    def _needs_graph(self):
        return self.training and torch.is_grad_enabled() and any(p.requires_grad for p in self.encoder1.parameters())

    def _forward_graph(self, x1, x2, h_matrix):
        """Training-mode forward as a differentiable graph of HIP nodes (masic_amd/autograd.py): same arithmetic and
        the same 7 noise draws in the same order as the fused path, without the inference-only fusions (writes into
        concat buffers, gate products in conv epilogues)."""
        x1 = x1.contiguous()
        x2 = x2.contiguous()
        B, _, H, W = x1.shape
        # reduced-precision training: the sampling matrices from the float64 device kernel -- the host evaluation of the reference's
        # float32 chain (bit-compatible, the float32 parity path keeps it) costs a device -> host copy that makes the host wait for
        # the previous step's last kernel before it may launch this step's first
        from masic_amd import nn as _mnn
        # h_matrix.requires_grad: the sampling matrices and the four warps (x1_warp, x1_mask_R, x1_mask_L, x1_hat_warp) are nodes that
        # carry the gradient back to h_matrix (kornia.warp_perspective is differentiable in the matrix, reference :638,644,781,821/833);
        # otherwise -- every driver of the reference detaches it -- exactly the calls below as they were
        hgrad = h_matrix.requires_grad
        if hgrad:
            m_fwd, m_back = _ag.WarpMatricesFn.apply(h_matrix, (H, W), (H, W), _mnn.reduced_precision())
        else:
            m_fwd, m_back = _warp_matrices(h_matrix, (H, W), (H, W), want_inverse=True, device=_mnn.reduced_precision())
        y1 = self.encoder1.latent_train(x1)
        S = self._model_bands(y1.shape[-2])             # 0: the calls below are the unbanded ones
        # Two branches of the step need nothing of the main chain (encoder1 -> y1 + noise -> decoder1 -> warp -> encoder1 -> heads2 ->
        # decoder2) until late: the left view's entropy chain (only its likelihoods leave it) and the right view up to its entropy
        # parameters.  With MASIC_TRAIN_STREAMS each is ISSUED where the reference has it -- the noise draws are numbered by the host --
        # but on a side stream of its own, beside the main stream's work; autograd runs every node's backward on the stream of its
        # forward, so their backward passes run beside the main chain's too.  (Not inside a HIP-graph capture: one stream there.)
        fj = _ForkJoin()
        side = _side_streams(x1.device) if (_TRAIN_STREAMS and not torch.cuda.is_current_stream_capturing()) else None
        sA, sE = (side[0], side[1]) if side is not None else (fj.main, fj.main)
        fj.fork(sE)
        with fj.on(sE):
            z1 = self._h_a1(y1)
            z1_hat, z1_lik = self.entropy_bottleneck1(z1)                                   # draw 1
            params1 = self._hyper_up(self.h_s1_up, z1_hat)
            ctx1 = _ag.banded_context(self.context_prediction1, self.gaussian1._quantize(y1, "noise"), S,      # draw 2
                                      call=self.context_prediction1.run)
            s1, m1, l1 = self._h_s1_same_resolution.heads(_ag.cat(params1, ctx1))
        # gaussian1(y1, s1, m1, l1) of the reference (:767) in its two halves: the draw here, the likelihood beside the synthesis transform
        y1_hat = self.gaussian1._quantize(y1, "noise")                                      # draw 3
        fj.fork(sE)
        with fj.on(sE):
            y1_lik = self.gaussian1.likelihood_of(y1_hat, s1, m1, l1, weights_are_logits=True)
        x1_hat = self.decoder1.reconstruct_train(y1_hat)

        fj.fork(sA)
        with fj.on(sA):
            x1_warp = _ag.WarpFn.apply(x1, m_fwd, (H, W)) if hgrad else _hip.warp_perspective(x1, m_fwd, (H, W))
            y2 = self.encoder2(x1_warp, x2)
            z2 = self._h_a2(y2)
            z2_hat, z2_lik = self.entropy_bottleneck2(z2)                                   # draw 4
            params2 = self._hyper_up(self.h_s2_up, z2_hat)
            ctx2 = _ag.banded_context(self.context_prediction2, self.gaussian2._quantize(y2, "noise"), S,      # draw 5
                                      call=self.context_prediction2.run)
            if hgrad:
                x1_mask_R = _ag.WarpOnesFn.apply(m_fwd, (B, H, W), (H, W))
                x1_mask_L = _ag.WarpFn.apply(x1_mask_R, m_back, (H, W))
            else:
                x1_mask_R = _hip.warp_perspective(None, m_fwd, (H, W), ones_like=(B, H, W))
                x1_mask_L = _hip.warp_perspective(x1_mask_R, m_back, (H, W))
            gates = self.mask2weights_unit(x1_mask_R)
        x1_hat_warp = _ag.WarpFn.apply(x1_hat, m_fwd, (H, W))
        y1_warp = self.encoder1.latent_train(x1_hat_warp)
        y1_warp_hat = self.gaussian1._quantize(y1_warp, "noise")                        # draw 6
        if fj.join(sA) is not None:
            for t in (m_fwd, m_back):
                _keep_until(t, sA)
            for t in (y2, z2_lik, params2, ctx2, x1_mask_R, x1_mask_L, gates):
                _keep_until(t, fj.main)
        cat2 = _ag.cat(_ag.GateFn.apply(params2, gates, 0), _ag.GateFn.apply(ctx2, gates, 1),
                       _ag.GateFn.apply(y1_warp_hat, gates, 2))
        s2, m2, l2 = self._h_s2_same_resolution.heads(cat2)
        y2_hat, y2_lik = self.gaussian2(y2, s2, m2, l2, weights_are_logits=True)       # draw 7
        x2_hat = self.decoder2(y2_hat, x1_hat_warp)
        if fj.join(sE) is not None:
            for t in (y1, y1_hat):
                _keep_until(t, sE)
            for t in (y1_lik, z1_lik, z1_hat):
                _keep_until(t, fj.main)
        return {
            "x1_hat": x1_hat, "x2_hat": x2_hat, "y1_hat": y1_hat, "z1_hat": z1_hat,
            "x1_mask_R": x1_mask_R, "x1_mask_L": x1_mask_L,
            "likelihoods": {"y1": y1_lik, "y2": y2_lik, "z1": z1_lik, "z2": z2_lik},
        }

    def _forward_refine(self, y1, y2, z1, z2, x1, x2, m_fwd, m_back, noise, gates=None):
        """The graph of the encoder-side latent refinement (masic_amd/refine.py): from the four latents as
        leaves to the reconstructions and likelihoods, built from the nodes of _forward_graph.  "Mixed" quantisation -- everything the
        decoder will see is the rounded value with an identity gradient (autograd.RoundSteFn): round(y) into the synthesis transforms,
        both context models and, through x1_hat -> warp -> encoder1, round(y1_warp) into the right heads; round(z - median) + median
        into the hyper synthesis.  Only the points where a likelihood is evaluated carry noise: the mixtures at y + u, the bottlenecks
        at z + u, u = noise[0..3] for (y1, y2, z1, z2) in the tensors' own [B, C, h, w] layout.  m_fwd / m_back: the sampling matrices;
        gates: mask2weights_unit of the right-view mask, computed once per call by the caller (None: computed here, without a
        graph).  The weights are the caller's business: with requires_grad off everywhere (refine._Frozen) no weight-, bias- or
        table-gradient launch runs.  x2 is not read: y2 is a leaf, and the picture enters through the objective only."""
        B, _, H, W = x1.shape
        n_y1, n_y2, n_z1, n_z2 = noise
        if gates is None:
            with torch.no_grad():
                gates = self.mask2weights_unit(_hip.warp_perspective(None, m_fwd, (H, W), ones_like=(B, H, W)))

        def bottleneck(eb, z, u):
            """(round(z - median) + median with the identity gradient, the likelihood at z + u)"""
            med = eb.quantiles.detach()[:, 0, 1].contiguous()
            table = eb._table().detach()
            lb = eb.likelihood_bound if eb.use_likelihood_bound else 0.0
            # EntropyBottleneckFn reads its noise in the reference's (C, 1, h w B) draw layout
            lik = _ag.EntropyBottleneckFn.apply(z, table, u.permute(1, 2, 3, 0).contiguous(), med, lb)[1]
            return _ag.RoundSteFn.apply(z, med, table), lik

        # ---- left view
        y1_r = _ag.RoundSteFn.apply(y1, None, None)
        z1_r, z1_lik = bottleneck(self.entropy_bottleneck1, z1, n_z1)
        params1 = self._hyper_up(self.h_s1_up, z1_r)
        S = self._model_bands(y1.shape[-2])
        ctx1 = _ag.banded_context(self.context_prediction1, y1_r, S, call=self.context_prediction1.run)
        s1, m1, l1 = self._h_s1_same_resolution.heads(_ag.cat(params1, ctx1))
        y1_lik = self.gaussian1.likelihood_of(_ag.AddNoiseFn.apply(y1, n_y1), s1, m1, l1, weights_are_logits=True)
        x1_hat = self.decoder1.reconstruct_train(y1_r)
        # ---- right view
        y2_r = _ag.RoundSteFn.apply(y2, None, None)
        z2_r, z2_lik = bottleneck(self.entropy_bottleneck2, z2, n_z2)
        params2 = self._hyper_up(self.h_s2_up, z2_r)
        ctx2 = _ag.banded_context(self.context_prediction2, y2_r, S, call=self.context_prediction2.run)
        x1_hat_warp = _ag.WarpFn.apply(x1_hat, m_fwd, (H, W))
        y1_warp_r = _ag.RoundSteFn.apply(self.encoder1.latent_train(x1_hat_warp), None, None)
        cat2 = _ag.cat(_ag.GateFn.apply(params2, gates, 0), _ag.GateFn.apply(ctx2, gates, 1), _ag.GateFn.apply(y1_warp_r, gates, 2))
        s2, m2, l2 = self._h_s2_same_resolution.heads(cat2)
        y2_lik = self.gaussian2.likelihood_of(_ag.AddNoiseFn.apply(y2, n_y2), s2, m2, l2, weights_are_logits=True)
        x2_hat = self.decoder2(y2_r, x1_hat_warp)
        return {"x1_hat": x1_hat, "x2_hat": x2_hat, "likelihoods": {"y1": y1_lik, "y2": y2_lik, "z1": z1_lik, "z2": z2_lik}}

    def _eval_from_latents(self, y1, y2, z1, z2, m_fwd, gates):
        """The eval-mode forward from GIVEN latents (called under no_grad): what a file coded from them costs and reconstructs -- the
        pieces of _forward_eval on one stream, with z1 / z2 taken as given instead of computed from y1 / y2.  The true objective of the
        latent refinement (masic_amd/refine.py)."""
        M = self.M
        B, _, h, w = y1.shape
        H, W = 16 * h, 16 * w
        # left view
        z1_hat, z1_lik = self.entropy_bottleneck1(z1)
        cat16 = self._cat_f16k(self._h_s1_same_resolution, y1, 4 * M)
        cat1 = None if cat16 is not None else torch.empty((B, 4 * M, h, w), dtype=y1.dtype, device=y1.device)
        S = self._model_bands(h)
        self._context(self.context_prediction1, y1, band_rows=S, **self._slice(cat1, cat16, 2 * M, 2 * M))
        self._hyper_up(self.h_s1_up, z1_hat, **self._slice(cat1, cat16, 0, 2 * M))
        s1, m1, l1 = self._h_s1_same_resolution.heads(cat1 if cat16 is None else cat16, parallel=False)
        _, y1_lik = self.gaussian1(y1, s1, m1, l1, weights_are_logits=True, want_y_hat=False)
        x1_hat = self.decoder1.reconstruct(_hip.quantize(y1, "dequantize"))
        x1_hat_warp = _hip.warp_perspective(x1_hat, m_fwd, (H, W))
        # right view
        z2_hat, z2_lik = self.entropy_bottleneck2(z2)
        cat16 = self._cat_f16k(self._h_s2_same_resolution, y2, 5 * M)
        cat2 = None if cat16 is not None else torch.empty((B, 5 * M, h, w), dtype=y2.dtype, device=y2.device)
        self._hyper_up(self.h_s2_up, z2_hat, gate=gates, gate_c=0, **self._slice(cat2, cat16, 0, 2 * M))
        self._context(self.context_prediction2, y2, gate=gates, gate_c=1, band_rows=S, **self._slice(cat2, cat16, 2 * M, 2 * M))
        y2_lik = self._eval_right_entropy(x1_hat_warp, {"cat2": cat2, "cat16": cat16, "gates": gates, "y2": y2})
        x2_hat = self.decoder2(_hip.quantize(y2, "dequantize"), x1_hat_warp)
        return {"x1_hat": x1_hat, "x2_hat": x2_hat, "likelihoods": {"y1": y1_lik, "y2": y2_lik, "z1": z1_lik, "z2": z2_lik}}

    def forward(self, x1, x2, h_matrix, warp_matrices=None):
        """`warp_matrices` (optional): the (forward, inverse) normalised sampling matrices of masic_amd.homography for
        this h_matrix, precomputed by the caller -- lets the whole forward be captured into a HIP graph
        (masic_amd/graph.py), since their host-side float32 evaluation is the only synchronising step."""
        if self._needs_graph():
            return self._forward_graph(x1, x2, h_matrix)
        if torch.is_grad_enabled() and h_matrix.requires_grad:
            raise NotImplementedError("HSIC.forward: the gradient with respect to h_matrix exists in the training-mode graph only (.train() with "
                                      "trainable parameters); this call would leave h_matrix.grad None -- detach h_matrix or call under no_grad")
        M, K = self.M, self.K
        x1 = x1.contiguous()
        x2 = x2.contiguous()
        B, _, H, W = x1.shape

        m_fwd, m_back = warp_matrices if warp_matrices is not None else _warp_matrices(h_matrix, (H, W), (H, W), want_inverse=True)
        if not self.training:
            if torch.is_grad_enabled():
                # eval mode WITHOUT no_grad -- how the CQE driver calls the codec (newtrain_cqe_real.py:130, :160).  round() has zero
                # gradient, so of the graph the reference records only the two synthesis transforms (and the warp between them) carry
                # any: those are recorded as differentiable HIP nodes, the rest stays the fused inference schedule.  `eval_autograd`:
                # None (default) -- record them iff a synthesis parameter requires grad (what the reference's graph would hold; a frozen
                # HSIC, requires_grad_(False), costs nothing); True / False force it.  The likelihoods carry no graph in eval mode.
                want = getattr(self, "eval_autograd", None)
                if want is None:
                    want = any(p.requires_grad for m in (self.decoder1, self.decoder2) for p in m.parameters())
                with torch.no_grad():
                    return self._forward_eval(x1, x2, m_fwd, m_back, synthesis_grad=bool(want))
            return self._forward_eval(x1, x2, m_fwd, m_back)

        # ---- left view
        y1 = self.encoder1.latent(x1)
        z1 = self._h_a1(y1)
        z1_hat, z1_lik = self.entropy_bottleneck1(z1)
        h, w = y1.shape[-2:]
        cat1 = torch.empty((B, 4 * M, h, w), dtype=x1.dtype, device=x1.device)      # params1 | ctx_params1
        self._hyper_up(self.h_s1_up, z1_hat, cat1, 0)
        y1_ctx = self.gaussian1._quantize(y1, "noise")
        S = self._model_bands(h)
        _ag.banded_context(self.context_prediction1, y1_ctx, S, call=self.context_prediction1.run, out=cat1, out_coff=2 * M)
        s1, m1, l1 = self._h_s1_same_resolution.heads(cat1)
        y1_hat, y1_lik = self.gaussian1(y1, s1, m1, l1, weights_are_logits=True)
        x1_hat = self.decoder1.reconstruct(y1_hat)

        # ---- right view
        y2 = self.encoder2.forward_views(_hip.warp_perspective(x1, m_fwd, (H, W)), x2)
        z2 = self._h_a2(y2)
        z2_hat, z2_lik = self.entropy_bottleneck2(z2)

        x1_mask_R = _hip.warp_perspective(None, m_fwd, (H, W), ones_like=(B, H, W))
        x1_mask_L = _hip.warp_perspective(x1_mask_R, m_back, (H, W))
        gates = self.mask2weights_unit(x1_mask_R)                                    # [B,3,h,w]

        cat2 = torch.empty((B, 5 * M, h, w), dtype=x1.dtype, device=x1.device)      # params2*g0 | ctx2*g1 | y1_warp_hat*g2
        self._hyper_up(self.h_s2_up, z2_hat, cat2, 0, gate=gates, gate_c=0)
        y2_ctx = self.gaussian2._quantize(y2, "noise")
        _ag.banded_context(self.context_prediction2, y2_ctx, S, call=self.context_prediction2.run, out=cat2, out_coff=2 * M, gate=gates, gate_c=1)

        x1_hat_warp = _hip.warp_perspective(x1_hat, m_fwd, (H, W))                   # used twice (:821, :833)
        y1_warp = self.encoder1.latent(x1_hat_warp)
        noise = self.gaussian1._get_noise_cached(y1_warp)
        _hip.quantize(y1_warp, "noise", noise=noise, out=cat2, out_coff=4 * M, gate=gates, gate_c=2)

        s2, m2, l2 = self._h_s2_same_resolution.heads(cat2)
        y2_hat, y2_lik = self.gaussian2(y2, s2, m2, l2, weights_are_logits=True)
        x2_hat = self.decoder2(y2_hat, x1_hat_warp)

        return {
            "x1_hat": x1_hat, "x2_hat": x2_hat, "y1_hat": y1_hat, "z1_hat": z1_hat,
            "x1_mask_R": x1_mask_R, "x1_mask_L": x1_mask_L,
            "likelihoods": {"y1": y1_lik, "y2": y2_lik, "z1": z1_lik, "z2": z2_lik},
        }

    # ---- eval-mode forward (no noise draws, so the order of its branches is free).  What the reconstructions need is short:
    #   x1_hat = decoder1(round(y1)),  x2_hat = decoder2(round(y2), warp(x1_hat))
    # -- the quantised latents do not depend on the entropy parameters (entropy_models.py:851-853: means = None).  Everything
    # else only produces likelihoods: the hyper transforms, context models and head stacks are chains of small, latency-bound
    # kernels (a few dozen workgroups each).  They run on two side streams and fill the machine while the large analysis /
    # synthesis convolutions run:
    #   main : encoder1 -> round -> decoder1 -> warp -> [y2 from A] round -> decoder2
    #   E    : context model 1, h_a1 -> EB1 -> h_s1_up -> heads1 -> GMM likelihood
    #   A    : warp(x1) -> encoder2 -> h_a2 -> EB2 -> masks -> mask2weights -> h_s2_up, context model 2
    #          -> [warp(x1_hat) from main] encoder1 -> round into cat2 -> heads2 -> GMM likelihood
    # Every fork of this DAG starts on the main stream (nested forks break HIP-graph capture here, see _GmmHeads.heads).  masic_amd/graph.py captures the whole DAG; issued eagerly the same events order it.
    def _eval_right_branch(self, x1, x2, m_fwd, m_back, on_y2=None):
        M = self.M
        B, _, H, W = x1.shape
        # y2 once, in the layouts of its readers: float32 (likelihood), round (context model, decoder2), |y2| (hyper analysis)
        lay = self.encoder2.forward_views(_hip.warp_perspective(x1, m_fwd, (H, W)), x2, layouts={"want": ("y32", "round16", "abs16")})
        y2, y2_round16, y2_abs16 = (lay["y32"], lay["round16"], lay["abs16"]) if isinstance(lay, dict) else (lay, None, None)
        if on_y2 is not None:
            on_y2()                # the reconstruction chain on the main stream only needs y2, not the entropy side of this branch
        z2 = self._h_a2(y2, abs16=y2_abs16)
        z2_hat, z2_lik = self.entropy_bottleneck2(z2)
        h, w = y2.shape[-2:]
        cat16 = self._cat_f16k(self._h_s2_same_resolution, y2, 5 * M)
        cat2 = None if cat16 is not None else torch.empty((B, 5 * M, h, w), dtype=x1.dtype, device=x1.device)       # params2*g0 | ctx2*g1 | y1_warp_hat*g2
        # masks and gates: a chain of tiny kernels first needed here; at the head of the forward it would only delay the
        # analysis transform
        x1_mask_R = _hip.warp_perspective(None, m_fwd, (H, W), ones_like=(B, H, W))
        x1_mask_L = _hip.warp_perspective(x1_mask_R, m_back, (H, W))
        gates = self.mask2weights_unit(x1_mask_R)                                    # [B,3,h,w]
        self._hyper_up(self.h_s2_up, z2_hat, gate=gates, gate_c=0, **self._slice(cat2, cat16, 0, 2 * M))
        self._context(self.context_prediction2, y2, gate=gates, gate_c=1, round16=y2_round16, band_rows=self._model_bands(h),
                      **self._slice(cat2, cat16, 2 * M, 2 * M))
        return {"y2": y2, "y2_round16": y2_round16, "y2_abs16": y2_abs16, "z2_hat": z2_hat, "z2_lik": z2_lik, "cat2": cat2, "cat16": cat16, "gates": gates, "x1_mask_R": x1_mask_R, "x1_mask_L": x1_mask_L}

    def _cat_f16k(self, head, y, C):
        """A whole F16K of C channels for the concat in front of an entropy-parameter head when the bf16 eval forward can keep it in F16K: the
        producers (last hyper-synthesis layer, context model, the rounded warped latent) then write their gated slices as bf16 records
        and the head's grouped GEMMs read them directly -- no float32 concat, no conversion pass of the whole buffer on the entropy
        chain (same values bit for bit: the gate multiplies in float32 before the one rounding to bf16 either way).  None otherwise
        (float32 / fp8 operands, fp8 calibration, head widths without the grouped GEMM form; _CAT_F16K off)."""
        from masic_amd import nn as _mnn
        if not (_CAT_F16K and _HEADS_GROUPED and _bf16_inference(y) and not _mnn._FP8 and not _fp8.recording() and C % 16 == 0
                and _fp8.scales(head) is None and head._grouped_heads_ok()):
            return None
        B, _, h, w = y.shape
        return _F16K.empty(B, C, h, w, y.device)

    def _eval_left_entropy(self, y1, round16=None, abs16=None):
        """On the current (side) stream: everything of the left view that only feeds likelihoods.
        round16 / abs16: bf16(round(y1)) / bf16(|y1|) in F16K where encoder1 wrote them."""
        M = self.M
        B = y1.shape[0]
        cat16 = self._cat_f16k(self._h_s1_same_resolution, y1, 4 * M)
        cat1 = None if cat16 is not None else torch.empty((B, 4 * M) + tuple(y1.shape[-2:]), dtype=y1.dtype, device=y1.device)   # params1 | ctx_params1
        self._context(self.context_prediction1, y1, round16=round16, band_rows=self._model_bands(y1.shape[-2]),
                      **self._slice(cat1, cat16, 2 * M, 2 * M))
        z1 = self._h_a1(y1, abs16=abs16)
        z1_hat, z1_lik = self.entropy_bottleneck1(z1)
        self._hyper_up(self.h_s1_up, z1_hat, **self._slice(cat1, cat16, 0, 2 * M))
        s1, m1, l1 = self._h_s1_same_resolution.heads(cat1 if cat16 is None else cat16, parallel=False)
        _, y1_lik = self.gaussian1(y1, s1, m1, l1, weights_are_logits=True, want_y_hat=False)
        return {"z1_hat": z1_hat, "z1_lik": z1_lik, "y1_lik": y1_lik}

    def _eval_right_entropy(self, x1_hat_warp, right):
        """On the right view's stream, after its branch: the warped left reconstruction through the left analysis transform
        (the one left -> right dependency of the entropy model), then the right view's heads and likelihood."""
        M = self.M
        cat2, cat16, gates, y2 = right["cat2"], right["cat16"], right["gates"], right["y2"]
        if cat16 is not None:             # round(y1_warp) * gate straight into its F16K slice ...
            # ... from the epilogue of the analysis transform's last layer: no float32 y1_warp, no pass over it in front of the heads
            dst = cat16.channels(4 * M, M)
            if self.encoder1.latent_layouts(x1_hat_warp, want=("round16",), round16=dst, gate=gates, gate_c=2) is None:
                dst.fill_from_nchw(self.encoder1.latent(x1_hat_warp), in_op=_hip.INOP_ROUND, gate=gates, gate_c=2)
        else:
            _hip.quantize(self.encoder1.latent(x1_hat_warp), "dequantize", out=cat2, out_coff=4 * M, gate=gates, gate_c=2)
        s2, m2, l2 = self._h_s2_same_resolution.heads(cat2 if cat16 is None else cat16, parallel=False)
        _, y2_lik = self.gaussian2(y2, s2, m2, l2, weights_are_logits=True, want_y_hat=False)
        return y2_lik

    def _forward_eval(self, x1, x2, m_fwd, m_back, synthesis_grad=False):
        """synthesis_grad (called under no_grad): decoder1 -> warp -> decoder2 are recorded as differentiable HIP nodes, the
        rest of the forward stays the fused inference schedule (`eval_autograd`, see forward)."""
        import contextlib
        recorded = torch.enable_grad if synthesis_grad else contextlib.nullcontext
        B, _, H, W = x1.shape
        fj = _ForkJoin()             # every cross-stream wait goes through it: the three capture rules raise instead of faulting
        cur = fj.main
        sA, sE = _side_streams(x1.device)[:2]
        if getattr(self, "serial_schedule", False):      # everything on the current stream, in issue order (kernel timing in isolation; eager only)
            sA = sE = cur
        serial = sA is cur
        if not serial:
            fj.fork(sA)
        with fj.on(sA):
            y2_ready = []
            right = self._eval_right_branch(x1, x2, m_fwd, m_back, on_y2=lambda: y2_ready.append(fj.record(sA)))
            ev_y2 = y2_ready[0]
        # left view: analysis, then the reconstruction chain here and the entropy chain beside it
        # y1 once, in the layouts of its readers: float32 (likelihood), float32 round = the y1_hat returned, F16K round (context model and
        # decoder1 share the buffer), F16K |y1| (hyper analysis); where that form does not apply, the separate launches
        lay = self.encoder1.latent_layouts(x1, want=("y32", "round32", "round16", "abs16"))
        if lay is not None:
            y1, y1_hat, y1_round16, y1_abs16 = lay["y32"], lay["round32"], lay["round16"], lay["abs16"]
        else:
            y1, y1_hat, y1_round16, y1_abs16 = self.encoder1.latent(x1), None, None, None
        if not serial:
            fj.fork(sE)
        with fj.on(sE):
            left = self._eval_left_entropy(y1, round16=y1_round16, abs16=y1_abs16)
            ev_left = fj.record(sE)
        for t in (y1, y1_round16, y1_abs16):
            _keep_until(t, sE)
        if y1_hat is None:
            y1_hat = _hip.quantize(y1, "dequantize")
        with recorded():
            x1_hat = None if synthesis_grad or y1_round16 is None else self.decoder1.reconstruct(y1_round16)    # the context model's F16K round(y1)
            if x1_hat is None:
                x1_hat = self.decoder1(y1_hat)[0] if synthesis_grad else self.decoder1.reconstruct(y1_hat)
            x1_hat_warp = (_ag.WarpFn.apply(x1_hat, m_fwd, (H, W)) if synthesis_grad
                           else _hip.warp_perspective(x1_hat, m_fwd, (H, W)))        # used twice (:821, :833)
        if not serial:
            fj.fork(sA)
        with fj.on(sA):
            y2_lik = self._eval_right_entropy(x1_hat_warp, right)
            ev_right = fj.record(sA)
        _keep_until(x1_hat_warp, sA)
        # right view reconstruction
        if not serial:
            fj.wait(cur, ev_y2)
        x2_hat = None
        if right["y2_round16"] is not None and not synthesis_grad:       # round(y2) is there in F16K: the float32 y2_hat is no output of the model
            x2_hat = self.decoder2(right["y2_round16"], x1_hat_warp)
        if x2_hat is None:
            y2_hat = _hip.quantize(right["y2"], "dequantize")
            with recorded():
                x2_hat = self.decoder2(y2_hat, x1_hat_warp)
        if not serial:
            fj.wait(cur, ev_left)
            fj.wait(cur, ev_right)
        for t in list(right.values()) + list(left.values()) + [y2_lik]:
            _keep_until(t, cur)
        return {
            "x1_hat": x1_hat, "x2_hat": x2_hat, "y1_hat": y1_hat, "z1_hat": left["z1_hat"],
            "x1_mask_R": right["x1_mask_R"], "x1_mask_L": right["x1_mask_L"],
            "likelihoods": {"y1": left["y1_lik"], "y2": y2_lik, "z1": left["z1_lik"], "z2": right["z2_lik"]},
        }

    def latents(self, x1, x2, h_matrix):
        """Unquantised latents (y1, y2, z1, z2) -- the inputs of the int32 symbol streams that feed the
        range coder (reference compress(): MASIC.py:855-868)."""
        x1 = x1.contiguous()
        B, _, H, W = x1.shape
        y1 = self.encoder1.latent(x1)
        z1 = self._h_a1(y1)
        m_fwd, _ = _warp_matrices(h_matrix, (H, W), (H, W))
        x1_warp = _hip.warp_perspective(x1, m_fwd, (H, W))
        y2 = self.encoder2(x1_warp, x2.contiguous())
        z2 = self._h_a2(y2)
        return y1, y2, z1, z2

    def symbol_streams(self, x1, x2, h_matrix):
        """int32 symbols round(y1), round(y2), round(z1 - med1), round(z2 - med2)."""
        y1, y2, z1, z2 = self.latents(x1, x2, h_matrix)
        med1 = self.entropy_bottleneck1.quantiles.detach()[:, 0, 1].contiguous()
        med2 = self.entropy_bottleneck2.quantiles.detach()[:, 0, 1].contiguous()
        return {"y1": _hip.symbols(y1), "y2": _hip.symbols(y2), "z1": _hip.symbols(z1, med1), "z2": _hip.symbols(z2, med2)}

    # ---- bitstream (reference :855-1408).  masic_amd/codec.py holds the wavefront coder; here the model
    # side: which tensors condition the tables of each view, computed identically by compress and decompress.
    def _codec_check(self, who, H=None, W=None):
        if self.training:
            raise RuntimeError(f"{who}: call .eval() first (the reference quantises with noise in training mode)")
        if H is not None and (H % 64 or W % 64):
            # the header stores H, W and the decoder derives the latent geometry as H//16, H//64 (reference :1308-1322); other
            # sizes would be written with ceil-div latents that decompress cannot reproduce
            raise ValueError(f"{who}: picture size {H}x{W} must be a multiple of 64 in both dimensions "
                             "(pad the pairs as the reference's drivers do)")

    class _PairParams:
        """The entropy parameters of one pair's view for the bitstream coder, as far as they are known before the latent.  Callable:
        y_hat -> (sigma, mu, logits) over the full latent (the coder's form for float32 / fp8 operands).  cat16 / gate: the view's F16K
        concat buffer (hyper part filled) and gates, which _batch_params stacks for the pixel-list form."""

        def __init__(self, full, cat16=None, gate=None):
            self._full, self.cat16, self.gate = full, cat16, gate

        def __call__(self, y_hat):
            return self._full(y_hat)

    class _PixelParams:
        """The same layers, with bf16 operands, evaluated on a LIST OF PIXELS of B pairs by the kernels of masic_amd/csrc/skinny.hip --
        `run(pix, step, list_stride, npix, band_rows=0)` reads the latent from `y16` (F16K; the device decoder writes it, the encoder fills it with
        `set_latent`) and writes `sigma`, `mu`, `logits` ([B, K*M, h, w] float32) at those pixels.  Encoder (all pixels in one launch
        per layer) and decoder (one coding wavefront per launch) run the same kernels with the same k order, and a pixel's result does
        not depend on its tile mates: bit-identical parameters on both sides."""
        skinny = True

        def __init__(self, sk):
            self._sk = sk
            self.y16, self.sigma, self.mu, self.logits = sk["y16"], sk["sigma"], sk["mu"], sk["logits"]

        def set_latent(self, y_hat):
            _hip.nchw_to_f16k_view(y_hat.contiguous(), self.y16, self._sk["M16"], 0)

        def run(self, pix, step, list_stride, npix, band_rows=0):
            k = self._sk
            _hip.skinny_group([k["ctx"]], pix, step, list_stride, npix, k["h"], k["w"], ctx=True, gate=k["gate"], gate_c=1, nimg=k["B"],
                              band_rows=band_rows)
            for layers in k["heads"]:
                _hip.skinny_group(layers, pix, step, list_stride, npix, k["h"], k["w"], nimg=k["B"])

    def _skinny_params(self, head, ctx, cat16, gate):
        """Buffers and layer descriptions of _PixelParams over B pairs (cat16: the pairs' F16K concat buffers stacked into one whole
        F16K, gate stacked [B, ...]), or None when the pixel-list form does not apply (widths the kernels are not built for)."""
        from masic_amd import nn as _mnn
        M, K = self.M, self.K
        if (M % 16 or (2 * M) % 32 or not head._grouped_heads_ok()
                or ctx.kernel_size != (5, 5)):
            return None
        B, C, h, w = cat16.shape
        dev = cat16.buf.device
        ctx.zero_masked_taps()
        wpc = _mnn._cached(ctx, "_packed_skinny_cache", _mnn.weight_key(ctx.weight), (), lambda: _hip.pack_skinny_ctx_weight(ctx.weight.detach()))
        M16 = (M + 15) // 16 * 16
        y16 = torch.zeros(B * M16 * h * w, dtype=torch.int16, device=dev)
        outs = [torch.empty((B, K * M, h, w), dtype=torch.float32, device=dev) for _ in range(3)]
        heads, t = [], [cat16.buf] * 3
        for i in range(3):
            layers, nxt = [], []
            for k_, (name, tag, acts) in enumerate(head._STACKS):
                layer = getattr(head, name)[2 * i]
                L = dict(x=t[k_], wp=layer.packed_gemm_dma_weight(), bias=layer.bias.detach(), Cin=layer.in_channels, Cout=layer.out_channels, act=acts[i])
                if i == 2:
                    L["y32"], L["out_ctot"] = outs[k_], layer.out_channels
                else:
                    L["out_ctot"] = (layer.out_channels + 15) // 16 * 16
                    L["y16"] = torch.zeros(B * L["out_ctot"] * h * w, dtype=torch.int16, device=dev)
                    nxt.append(L["y16"])
                layers.append(L)
            heads.append(layers)
            t = nxt
        ctxl = dict(x=y16, wp=wpc, bias=None if ctx.bias is None else ctx.bias.detach(), Cin=M16, Cout=2 * M, act=_NONE, y16=cat16.buf, out_ctot=C, out_coff=2 * M)
        return dict(y16=y16, M16=M16, sigma=outs[0], mu=outs[1], logits=outs[2], ctx=ctxl, heads=heads, h=h, w=w, gate=gate, B=B)

    def _left_params_fn(self, z1_hat, h, w, band_rows=0):
        M = self.M
        # (bf16 operands: the concat buffer is F16K, as in the eval forward -- the context model writes its slice as bf16 records and the
        # grouped head GEMMs read the buffer directly: no conversion pass over the 768-channel buffer per coding step)
        cat16 = self._cat_f16k(self._h_s1_same_resolution, z1_hat.new_empty((1, M, h, w)), 4 * M)
        cat1 = None if cat16 is not None else torch.empty((1, 4 * M, h, w), dtype=torch.float32, device=z1_hat.device)      # params1 | ctx_params1
        self._hyper_up(self.h_s1_up, z1_hat, **self._slice(cat1, cat16, 0, 2 * M))

        def params(y_hat):
            self._context(self.context_prediction1, y_hat, band_rows=band_rows, **self._slice(cat1, cat16, 2 * M, 2 * M))
            return self._h_s1_same_resolution.heads(cat1 if cat16 is None else cat16)
        return HSIC._PairParams(params, cat16)

    def _right_params_fn(self, z2_hat, x1_hat, m_fwd, m_back, H, W, h, w, band_rows=0):
        """-> (params_fn, x1_hat_warp): everything of the right view's tables that the decoder knows before y2.  band_rows: the row
        bands of the full-latent form's context model (the pixel-list form takes them per launch)."""
        M = self.M
        dev = z2_hat.device
        x1_mask_R = _hip.warp_perspective(None, m_fwd, (H, W), ones_like=(1, H, W))
        gates = self.mask2weights_unit(x1_mask_R)
        cat16 = self._cat_f16k(self._h_s2_same_resolution, z2_hat.new_empty((1, M, h, w)), 5 * M)
        cat2 = None if cat16 is not None else torch.empty((1, 5 * M, h, w), dtype=torch.float32, device=dev)   # params2*g0 | ctx2*g1 | y1_warp_hat*g2
        self._hyper_up(self.h_s2_up, z2_hat, gate=gates, gate_c=0, **self._slice(cat2, cat16, 0, 2 * M))
        x1_hat_warp = _hip.warp_perspective(x1_hat, m_fwd, (H, W))
        y1_warp = self.encoder1.latent(x1_hat_warp)
        if cat16 is not None:
            cat16.channels(4 * M, M).fill_from_nchw(y1_warp, in_op=_hip.INOP_ROUND, gate=gates, gate_c=2)
        else:
            _hip.quantize(y1_warp, "dequantize", out=cat2, out_coff=4 * M, gate=gates, gate_c=2)

        def params(y_hat):
            self._context(self.context_prediction2, y_hat, gate=gates, gate_c=1, band_rows=band_rows, **self._slice(cat2, cat16, 2 * M, 2 * M))
            return self._h_s2_same_resolution.heads(cat2 if cat16 is None else cat16)
        return HSIC._PairParams(params, cat16, gates.contiguous()), x1_hat_warp

    @staticmethod
    def _channel_flags(y_hat):
        """Reference :925-940: which channels hold a non-zero symbol (bit-packed into the header) and the alphabet half-width."""
        a = y_hat[0].abs()
        flags = (a.flatten(1).amax(1) > 0).cpu().numpy().astype(np.uint8)
        return flags, max(int(a.max().item()), 1)

    # ---- compress / decompress code one pair per call (the reference's methods), compress_batch / decompress_batch B pairs
    # (INTEGRATION.md "Batched bitstream coding"); one implementation per direction serves both.  A pair's files do not depend on its
    # batch mates: the once-per-call work (transforms, hyper path, reconstruction, warp, gates, z coder) runs per pair as B = 1 calls --
    # several bf16 layers pick or order their kernels by batch shape, so their bits at B > 1 differ from those at B = 1 -- and the
    # coding-step loops, where the time goes, run over all B pairs at once (codec.encode_views / decode_views).  float32 / fp8 operands
    # (no pixel-list form) code the pairs one after the other.
    def compress(self, x1, x2, h_matrix, output_name, output_path="", device="cpu", band_rows=0, latents=None):
        """Writes <output_name>.npz (picture size, z1 / z2 strings, channel flags, minmax: the reference's header layout,
        :916-948) and <output_name>.bin (the y1 / y2 streams, masic_amd/codec.py) under output_path.  `device` is accepted
        for signature compatibility; tensors stay where x1 is.  band_rows (0 .. 255; 0: off, today's file): code the y latents in
        independent bands of that many latent rows -- w + 3 (band_rows - 1) decode steps instead of w + 3 (h - 1), a slightly larger
        .bin that carries the value ("MSR3"; decompress reads it from there).  latents (None: off, today's file): a
        masic_amd.refine.Refined or a 4-tuple (y1, y2, z1, z2) of float latents that are coded INSTEAD of the analysis transforms'
        outputs -- rounded and entropy-coded exactly as those are; the file decodes with decompress as any other."""
        band_rows = _check_band_rows(band_rows, "HSIC.compress")
        out = self._compress_pairs("HSIC.compress", x1, x2, h_matrix, [output_name], output_path, batch=False, band_rows=band_rows,
                                   latents=latents)
        out["bytes"], out["bpp"] = out["bytes"][0], out["bpp"][0]
        return out

    def decompress(self, x1, x2, h_matrix, output_name, output_path="", device="cpu"):
        """Reads the two files compress wrote.  x1 / x2 are not used for decoding (the reference only takes sizes from them,
        :1308-1310) and may be None; tensors are created on the model's device."""
        return self._decompress_pairs("HSIC.decompress", [output_name], h_matrix, output_path, batch=False)

    def compress_batch(self, x1, x2, h_matrix, output_names, output_path="", band_rows=0, latents=None):
        """compress for B pairs: x1, x2 [B, 3, H, W], h_matrix [B, 3, 3], B output names.  Writes <name_i>.npz / <name_i>.bin, byte for
        byte what compress(x1[i:i+1], x2[i:i+1], h_matrix[i:i+1], name_i) writes, and returns compress's dict with [B, ...] tensors
        ("bytes" / "bpp": lists of B).  band_rows: as in compress, one value for the batch.  latents: as in compress, [B, ...] tensors."""
        band_rows = _check_band_rows(band_rows, "HSIC.compress_batch")
        return self._compress_pairs("HSIC.compress_batch", x1, x2, h_matrix, output_names, output_path, batch=True, band_rows=band_rows,
                                    latents=latents)

    def decompress_batch(self, output_names, h_matrix, output_path=""):
        """decompress for B pairs written by compress or compress_batch (one picture size, one band_rows, the current operand mode, in
        the fp8 mode one activation-scale table) -> decompress's dict with [B, ...] tensors; slice i equals decompress of pair i alone."""
        return self._decompress_pairs("HSIC.decompress_batch", output_names, h_matrix, output_path, batch=True)

    @staticmethod
    def _write_pair(output_path, output_name, H, W, views, fp8_table, band_rows=0):
        """The two files of one pair; views: per view (z string, channel flags, minmax, framed y streams).  -> bytes written.
        band_rows = 0: magic "MSR2", bytes 6-7 zero; > 0: magic "MSR3" with byte 6 = band_rows, so that a build without the row bands
        refuses the file at the magic."""
        import os
        from masic_amd import codec, nn as _mnn
        for s_z, _, mm, _ in views:
            if len(s_z) > 65535 or mm > 65535:
                raise ValueError("HSIC.compress: the header stores string lengths and minmax as uint16 (reference :941-946)")
        out1 = os.path.join(output_path, str(output_name) + ".npz")
        with open(out1, "wb") as f:
            f.write(np.array([H, W], dtype=np.uint16).tobytes())
            for s_z, flag, mm, _ in views:
                f.write(np.array([len(s_z), mm], dtype=np.uint16).tobytes())
                f.write(np.packbits(flag).tobytes())
                f.write(s_z)
        out2 = os.path.join(output_path, str(output_name) + ".bin")
        with open(out2, "wb") as f:
            f.write((codec.MAGIC_BANDS if band_rows else codec.MAGIC)
                    + bytes([{"f32": 0, "bf16": 1, "fp8": 2}[_mnn.get_precision()], 1 if fp8_table is not None else 0, band_rows, 0]))
            if fp8_table is not None:
                # the coding tables of the fp8 mode depend on the activation scales of masic_amd.fp8.calibrate, which live outside
                # state_dict(): the stream carries them, so any decoder holding the same weights rebuilds the same tables
                f.write(np.array([len(fp8_table)], dtype=np.uint32).tobytes())
                f.write(fp8_table)
            for _, _, _, s_y in views:      # each: u32 n, n x u32 lengths, the n channel streams (masic_amd/codec.py)
                f.write(s_y)
        return os.path.getsize(out1) + os.path.getsize(out2)

    def _read_pair(self, output_path, output_name, who):
        """The two files of one pair -> H, W, per view (z string, minmax, coded channels as a list), per view the framed
        y streams, the fp8 scale table or None, band_rows (0 for an "MSR2" file, whose bytes 6-7 are not read; byte 6 of an "MSR3"
        file, where 0 is an error).  ValueError for a foreign stream, one written in another operand mode, or a
        container that is cut short, holds impossible length fields or carries bytes after its last field."""
        import os
        from masic_amd import codec, nn as _mnn
        M = self.M

        def take(f, n, what):
            data = f.read(n)
            if len(data) != n:
                raise ValueError(f"{who}: truncated file: {what} needs {n} bytes, {len(data)} are left")
            return data

        with open(os.path.join(output_path, str(output_name) + ".npz"), "rb") as f:
            H, W = (int(v) for v in np.frombuffer(take(f, 4, "the picture size"), dtype=np.uint16))
            views = []
            for v in range(2):
                length, minmax = (int(x) for x in np.frombuffer(take(f, 4, f"the header of view {v + 1}"), dtype=np.uint16))
                flags = np.unpackbits(np.frombuffer(take(f, M // 8, f"the channel flags of view {v + 1}"), dtype=np.uint8))
                views.append((take(f, length, f"the z string of view {v + 1}"), minmax, np.flatnonzero(flags).tolist()))
            if f.read(1):
                raise ValueError(f"{who}: bytes follow the second view in the .npz header file")
        with open(os.path.join(output_path, str(output_name) + ".bin"), "rb") as f:
            head = f.read(8)
            if head[:4] not in (codec.MAGIC, codec.MAGIC_BANDS):
                raise ValueError(f"{who}: not a stream of this library (magic %r)" % head[:4])
            if len(head) != 8:
                raise ValueError(f"{who}: truncated file: the .bin header needs 8 bytes, {len(head)} are there")
            band_rows = head[6] if head[:4] == codec.MAGIC_BANDS else 0
            if head[:4] == codec.MAGIC_BANDS and band_rows == 0:
                raise ValueError(f"{who}: an MSR3 stream must carry its band_rows (1 .. 255) in byte 6 of the .bin header, found 0")
            if head[4] != {"f32": 0, "bf16": 1, "fp8": 2}[_mnn.get_precision()]:
                raise ValueError(f"{who}: the stream was written in the %s operand mode; the coding tables depend on it "
                                 "(masic_amd.nn.set_precision)" % ("f32", "bf16", "fp8")[head[4] if head[4] < 3 else 0])
            fp8_table = None
            if head[5] & 1:
                n = int(np.frombuffer(take(f, 4, "the length of the fp8 table"), dtype=np.uint32)[0])
                fp8_table = take(f, n, "the fp8 table")
            elif head[4] == 2:
                raise ValueError(f"{who}: an fp8-mode stream without its activation-scale table")
            try:
                streams = codec.split_views(f.read(), 2)
            except ValueError as e:
                raise ValueError(f"{who}: {e}") from e
        return H, W, views, streams, fp8_table, band_rows

    def _batch_params(self, parts, head, ctx, C, h, w):
        """One _PixelParams over the B >= 1 pairs of `parts` (_PairParams): their concat buffers and gates stacked, the pixel-list
        buffers sized for B; None when the pixel-list form does not apply."""
        if any(p.cat16 is None for p in parts):
            return None
        cat = _F16K.wrap(torch.cat([p.cat16.buf for p in parts]), len(parts), C, h, w)
        gate = torch.cat([p.gate for p in parts]) if parts[0].gate is not None else None
        sk = self._skinny_params(head, ctx, cat, gate)
        return None if sk is None else HSIC._PixelParams(sk)

    def _code_views(self, parts, head, ctx, C, y_hat, chans, minmaxes, bound, names, band_rows=0):
        """compress side of one view over the pairs -> per pair the framed y streams.  names: the pairs' names for error messages (a
        batch) or None."""
        from masic_amd import codec
        h, w = y_hat.shape[-2:]
        bp = self._batch_params(parts, head, ctx, C, h, w)
        if bp is not None:
            return codec.encode_views(bp, y_hat, self.M, self.K, chans, minmaxes, bound, names=names, band_rows=band_rows)
        out = []
        for i, p in enumerate(parts):
            with _pair_errors(i, names):
                out += codec.encode_views(p, y_hat[i:i + 1], self.M, self.K, chans[i:i + 1], minmaxes[i:i + 1], bound, band_rows=band_rows)
        return out

    def _decode_views(self, parts, head, ctx, C, blobs, hw, chans, minmaxes, bound, names, dev, band_rows=0):
        """decompress side of one view over the pairs -> y_hat [B, M, h, w]."""
        from masic_amd import codec
        bp = self._batch_params(parts, head, ctx, C, *hw)
        if bp is not None:
            return codec.decode_views(bp, blobs, hw, self.M, self.K, chans, minmaxes, bound, dev, names=names, band_rows=band_rows)
        out = []
        for i, p in enumerate(parts):
            with _pair_errors(i, names):
                out.append(codec.decode_views(p, blobs[i:i + 1], hw, self.M, self.K, chans[i:i + 1], minmaxes[i:i + 1], bound, dev,
                                              band_rows=band_rows))
        return torch.cat(out)

    def _given_latents(self, who, latents, B, H, W):
        """latents= of compress / compress_batch -> four contiguous float32 tensors [B, M | N, ...] on the device, shapes checked."""
        lat = tuple(latents[:4]) if isinstance(latents, tuple) else tuple(latents)
        if len(lat) != 4:
            raise ValueError(f"{who}: latents must be a masic_amd.refine.Refined or a 4-tuple (y1, y2, z1, z2)")
        want = [(B, self.M, H // 16, W // 16)] * 2 + [(B, self.N, H // 64, W // 64)] * 2
        for t, name, shape in zip(lat, ("y1", "y2", "z1", "z2"), want):
            if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) != shape:
                raise ValueError(f"{who}: latents: {name} must be a float32 device tensor of shape {shape}")
        return [t.detach().contiguous() for t in lat]

    def _compress_pairs(self, who, x1, x2, h_matrix, output_names, output_path, batch, band_rows=0, latents=None):
        from masic_amd import nn as _mnn
        x1, x2 = x1.contiguous(), x2.contiguous()
        B, _, H, W = x1.shape
        names = [str(n) for n in output_names]
        self._codec_check(who, H, W)
        if not batch and B != 1:
            raise ValueError(f"{who} codes one stereo pair per call (the reference codes batch element 0 only)")
        if B < 1 or len(names) != B:
            raise ValueError(f"{who}: {B} pairs and {len(names)} output names")
        if batch and (x2.shape != x1.shape or h_matrix.shape[0] != B):
            raise ValueError(f"{who}: x1, x2 and h_matrix must hold the same number of pairs")
        M = self.M
        tags = names if batch else None
        fp8_table = _fp8.stream_table(self) if _mnn.get_precision() == "fp8" else None
        given = None if latents is None else self._given_latents(who, latents, B, H, W)
        pr = []
        with torch.no_grad():
            for i in range(B):          # left view, per pair
                a, b_ = x1[i:i + 1], x2[i:i + 1]
                m_fwd, m_back = _warp_matrices(h_matrix[i:i + 1], (H, W), (H, W), want_inverse=True)
                y1 = self.encoder1.latent(a) if given is None else given[0][i:i + 1]
                z1 = self._h_a1(y1) if given is None else given[2][i:i + 1]
                z1_strings = self.entropy_bottleneck1.compress(z1)
                z1_hat = self.entropy_bottleneck1.decompress(z1_strings, z1.size()[-2:])
                y1_hat = _hip.quantize(y1, "dequantize")
                flag1, minmax1 = self._channel_flags(y1_hat)
                pr.append(dict(i=i, x1=a, x2=b_, m_fwd=m_fwd, m_back=m_back, z1_strings=z1_strings, z1_hat=z1_hat, y1_hat=y1_hat, flag1=flag1,
                               minmax1=minmax1))
            h, w = pr[0]["y1_hat"].shape[-2:]
            s_y1 = self._code_views([self._left_params_fn(p["z1_hat"], h, w, band_rows) for p in pr], self._h_s1_same_resolution,
                                    self.context_prediction1, 4 * M, torch.cat([p["y1_hat"] for p in pr]),
                                    [np.flatnonzero(p["flag1"]).tolist() for p in pr], [p["minmax1"] for p in pr],
                                    self.gaussian1._scale_bound_value, tags, band_rows)
            parts2 = []
            for p in pr:                # right view, per pair
                p["x1_hat"] = self.decoder1.reconstruct(p["y1_hat"])
                y2 = self.encoder2.forward_views(_hip.warp_perspective(p["x1"], p["m_fwd"], (H, W)), p["x2"]) if given is None else given[1][p["i"]:p["i"] + 1]
                z2 = self._h_a2(y2) if given is None else given[3][p["i"]:p["i"] + 1]
                p["z2_strings"] = self.entropy_bottleneck2.compress(z2)
                p["z2_hat"] = self.entropy_bottleneck2.decompress(p["z2_strings"], z2.size()[-2:])
                p["y2_hat"] = _hip.quantize(y2, "dequantize")
                p["flag2"], p["minmax2"] = self._channel_flags(p["y2_hat"])
                params2, p["x1_hat_warp"] = self._right_params_fn(p["z2_hat"], p["x1_hat"], p["m_fwd"], p["m_back"], H, W, h, w, band_rows)
                parts2.append(params2)
            s_y2 = self._code_views(parts2, self._h_s2_same_resolution, self.context_prediction2, 5 * M, torch.cat([p["y2_hat"] for p in pr]),
                                    [np.flatnonzero(p["flag2"]).tolist() for p in pr], [p["minmax2"] for p in pr],
                                    self.gaussian2._scale_bound_value, tags, band_rows)
            for p in pr:
                p["x2_hat"] = self.decoder2(p["y2_hat"], p["x1_hat_warp"])
        nbytes = [self._write_pair(output_path, names[i], H, W, ((p["z1_strings"][0], p["flag1"], p["minmax1"], s_y1[i]),
                                                                  (p["z2_strings"][0], p["flag2"], p["minmax2"], s_y2[i])), fp8_table,
                                    band_rows)
                  for i, p in enumerate(pr)]
        out = {k: torch.cat([p[k] for p in pr]) for k in ("x1_hat", "x2_hat", "y1_hat", "y2_hat", "z1_hat", "z2_hat")}
        out.update(bytes=nbytes, bpp=[n * 8.0 / (H * W) for n in nbytes])
        return out

    def _decompress_pairs(self, who, output_names, h_matrix, output_path, batch):
        names = [str(n) for n in output_names]
        B = len(names)
        self._codec_check(who)
        if B < 1:
            raise ValueError(f"{who}: no output names")
        if batch and h_matrix.shape[0] != B:
            raise ValueError(f"{who}: h_matrix must hold one matrix per name")
        M = self.M
        tags = names if batch else None
        dev = self.encoder1.g_a_conv1.weight.device
        files = [self._read_pair(output_path, n, f"{who}: pair {i} ({n})" if batch else who) for i, n in enumerate(names)]
        H, W = files[0][:2]
        for i, f in enumerate(files):
            if f[:2] != (H, W):
                raise ValueError(f"{who}: pair {i} ({names[i]}) is {f[0]}x{f[1]}, pair 0 is {H}x{W}: one picture size per batch")
            if f[4] != files[0][4]:
                raise ValueError(f"{who}: pair {i} ({names[i]}) carries other fp8 activation scales than pair 0: one calibration per batch")
            if f[5] != files[0][5]:
                raise ValueError(f"{who}: pair {i} ({names[i]}) was coded with band_rows {f[5]}, pair 0 with {files[0][5]}: one band_rows per batch")
        band_rows = files[0][5]
        self._codec_check(who, H, W)
        h, w = H // 16, W // 16
        views = [f[2] for f in files]
        with torch.no_grad(), _fp8.stream_scales(self, files[0][4]):
            pr = []
            for i in range(B):
                m_fwd, m_back = _warp_matrices(h_matrix[i:i + 1], (H, W), (H, W), want_inverse=True)
                pr.append(dict(m_fwd=m_fwd, m_back=m_back,
                               z1_hat=self.entropy_bottleneck1.decompress([views[i][0][0]], (h // 4, w // 4)),
                               z2_hat=self.entropy_bottleneck2.decompress([views[i][1][0]], (h // 4, w // 4))))
            y1_hat = self._decode_views([self._left_params_fn(p["z1_hat"], h, w, band_rows) for p in pr], self._h_s1_same_resolution,
                                        self.context_prediction1, 4 * M, [f[3][0] for f in files], (h, w), [v[0][2] for v in views],
                                        [v[0][1] for v in views], self.gaussian1._scale_bound_value, tags, dev, band_rows)
            parts2 = []
            for i, p in enumerate(pr):
                p["y1_hat"] = y1_hat[i:i + 1]
                p["x1_hat"] = self.decoder1.reconstruct(p["y1_hat"])
                params2, p["x1_hat_warp"] = self._right_params_fn(p["z2_hat"], p["x1_hat"], p["m_fwd"], p["m_back"], H, W, h, w, band_rows)
                parts2.append(params2)
            y2_hat = self._decode_views(parts2, self._h_s2_same_resolution, self.context_prediction2, 5 * M, [f[3][1] for f in files], (h, w),
                                        [v[1][2] for v in views], [v[1][1] for v in views], self.gaussian2._scale_bound_value, tags, dev,
                                        band_rows)
            for i, p in enumerate(pr):
                p["y2_hat"] = y2_hat[i:i + 1]
                p["x2_hat"] = self.decoder2(p["y2_hat"], p["x1_hat_warp"])
        return {k: torch.cat([p[k] for p in pr]) for k in ("x1_hat", "x2_hat", "y1_hat", "y2_hat", "z1_hat", "z2_hat")}


class _pair_errors:
    """Coding errors of the pair-by-pair path of a batch name their pair, as the batched kernels' do (names None: one pair, no tag)."""

    def __init__(self, i, names):
        self.i, self.names = i, names

    def __enter__(self):
        return self

    def __exit__(self, et, ev, tb):
        if (self.names is not None and et is not None and issubclass(et, (RuntimeError, ValueError))
                and not isinstance(ev, torch.cuda.OutOfMemoryError)):
            from masic_amd import codec
            if isinstance(ev, codec.PairStreamError):        # keeps its type (CorruptStreamError) and gets its index in the batch
                raise type(ev)(self.i, f"{ev} -- pair {self.i} ({self.names[self.i]}) of the batch") from ev
            raise (ValueError if issubclass(et, ValueError) else RuntimeError)(f"{ev} -- pair {self.i} ({self.names[self.i]}) of the batch") from ev
        return False


# ------------------------------------------------------------------------------------------ CQE network
class Enhancement_Block(nn.Module):
    """Three residual blocks plus a skip over all of them (reference :149-164)."""

    def __init__(self, shape):
        super().__init__()
        self.RB1 = ResidualBlock(shape, shape)
        self.RB2 = ResidualBlock(shape, shape)
        self.RB3 = ResidualBlock(shape, shape)

    def forward(self, x):
        if torch.is_grad_enabled() and _ag.enhancement_block_supported(self, x) and (x.requires_grad or self.RB1.conv1.weight.requires_grad):
            return _ag.enhancement_block(self, x)   # bf16 mode training: one node, forward and backward on F16K buffers
        t = self.RB2(self.RB1(x))
        return self.RB3(t, extra_identity=x)        # (RB3(t)) + x, the outer add fused into RB3's last conv

    def f16k_supported(self, B, H, W):
        return all(rb.f16k_supported(B, H, W) for rb in (self.RB1, self.RB2, self.RB3))

    def forward_f16k(self, x, out=None):
        t = self.RB2.forward_f16k(self.RB1.forward_f16k(x))
        return self.RB3.forward_f16k(t, extra=x, out=out)


class mask2weights_EN(nn.Module):
    """mask -> Kw softmax-normalised gate maps at full resolution (reference :1411-1434)."""

    def __init__(self, Kw=2):
        super().__init__()
        self.Kw = Kw
        self.maskconv = nn.Sequential(
            conv(1, Kw, kernel_size=3, stride=1), nn.ReLU(inplace=True),
            conv(Kw, Kw * 2, kernel_size=3, stride=1), nn.ReLU(inplace=True),
            conv(Kw * 2, Kw * 2, kernel_size=3, stride=1), nn.ReLU(inplace=True),
            conv(Kw * 2, Kw, kernel_size=3, stride=1))

    def forward(self, m):
        s = self.maskconv
        if self.Kw == 2 and not (torch.is_grad_enabled() and (m.requires_grad or s[0].weight.requires_grad)):
            # inference: the four layers and the softmax in one launch, intermediates in LDS (csrc/m2w.hip; bit-identical to the chain below)
            return _hip.mask2weights_en(m, [p for i in (0, 2, 4, 6) for p in (s[i].weight, s[i].bias)])
        t = s[0].run(m, act=_RELU)
        t = s[2].run(t, act=_RELU)
        t = s[4].run(t, act=_RELU)
        return s[6].run(t, act=_hip.ACT_SOFTMAX_C)


class Independent_EN(nn.Module):
    """Cross quality-enhancement network (reference :1436-1501): each view is refined with features of the other
    view warped by the homography, mixed through mask-derived 2-way gates.  Warps, gate products and concats are
    fused (gated writes straight into the concat buffers); residual adds run in conv epilogues."""

    def __init__(self):
        super().__init__()
        self.EBl1 = Enhancement_Block(shape=32)
        self.EBl2 = Enhancement_Block(shape=64)
        self.EBl3 = Enhancement_Block(shape=96)
        self.EBr1 = Enhancement_Block(shape=32)
        self.EBr2 = Enhancement_Block(shape=64)
        self.EBr3 = Enhancement_Block(shape=96)
        self.conv0 = conv3x3(3, 32)
        self.conv1 = conv3x3(6, 32)
        self.conv2 = conv3x3(96, 3)
        self.mask2weights_unit = mask2weights_EN()

    def _needs_graph(self, *inputs):
        return torch.is_grad_enabled() and (any(t.requires_grad for t in inputs) or any(p.requires_grad for p in self.parameters()))

    def _forward_graph(self, x1_hat, x2_hat, h_matrix):
        """The same arithmetic as a differentiable graph of HIP nodes (masic_amd/autograd.py) for the CQE training step
        (reference newtrain_cqe_real.py:128-174): every warp of a tensor that carries gradient, every gate product and every
        concat is a node with a HIP backward, so all 86 parameters receive their gradient; the inference-only fusions (gated
        writes into concat buffers) are not used.  The masks carry no gradient (functions of h_matrix only, which the drivers
        detach)."""
        x1_hat = x1_hat.contiguous()
        x2_hat = x2_hat.contiguous()
        B, _, H, W = x1_hat.shape
        from masic_amd import nn as _mnn     # reduced-precision training: device kernel, no host round trip (see HSIC._forward_graph)
        m_fwd, m_back = _warp_matrices(h_matrix, (H, W), (H, W), want_inverse=True, device=_mnn.reduced_precision())
        mask_R = _hip.warp_perspective(None, m_fwd, (H, W), ones_like=(B, H, W))
        mask_L = _hip.warp_perspective(mask_R, m_back, (H, W))
        w_R = self.mask2weights_unit(mask_R)
        w_L = self.mask2weights_unit(mask_L)

        def warp(t, m):
            return _ag.WarpFn.apply(t, m, (H, W)) if t.requires_grad else _hip.warp_perspective(t, m, (H, W))
        gate = _ag.GateFn.apply
        x1_warp, x2_warp = warp(x1_hat, m_fwd), warp(x2_hat, m_back)
        x1c, x2c = self.conv0(x1_hat), self.conv0(x2_hat)
        out1 = self.EBl1(self.conv1(_ag.cat(gate(x2_warp, w_L, 0), gate(x1_hat, w_L, 1))))      # :1470
        out2 = self.EBr1(self.conv1(_ag.cat(gate(x1_warp, w_R, 0), gate(x2_hat, w_R, 1))))      # :1471
        out1_warp, out2_warp = warp(out1, m_fwd), warp(out2, m_back)
        out1 = self.EBl2(_ag.cat(gate(out1, w_L, 1), gate(out2_warp, w_L, 0)))                  # :1481
        out2 = self.EBr2(_ag.cat(gate(out2, w_R, 1), gate(out1_warp, w_R, 0)))                  # :1482
        def last(eb, feats, x_hat):                 # conv2(EB3(feats)) + x_hat   (:1485-1488)
            if _ag.enhancement_block_supported(eb, feats, tail=self.conv2):
                return _ag.enhancement_block(eb, feats, tail=self.conv2, res=x_hat)
            return self.conv2.run(eb(feats), res1=x_hat)
        return {"x1_hat": last(self.EBl3, _ag.cat(out1, x1c), x1_hat), "x2_hat": last(self.EBr3, _ag.cat(out2, x2c), x2_hat)}

    def _forward_f16k(self, x1_hat, x2_hat, h_matrix):
        """Inference with bf16 operands: the 32 / 64 / 96-channel full-resolution activations stay in F16K bf16 between the 36
        3x3 convolutions (DMA-staged MFMA kernels, LeakyReLU and residual adds in their epilogues); every gated / warped concat
        operand of :1470-1482 is written straight into its channel slice (masic_f16k_gate: whole 32-byte records per tap)."""
        B, _, H, W = x1_hat.shape
        dev = x1_hat.device
        m_fwd, m_back = _warp_matrices(h_matrix, (H, W), (H, W), want_inverse=True)
        mask_R = _hip.warp_perspective(None, m_fwd, (H, W), ones_like=(B, H, W))
        mask_L = _hip.warp_perspective(mask_R, m_back, (H, W))
        w_R = self.mask2weights_unit(mask_R)
        w_L = self.mask2weights_unit(mask_L)
        x1_warp = _hip.warp_perspective(x1_hat, m_fwd, (H, W))
        x2_warp = _hip.warp_perspective(x2_hat, m_back, (H, W))
        outs = []
        feats = []
        for x_own, x_other_warp, w, EB1 in ((x1_hat, x2_warp, w_L, self.EBl1), (x2_hat, x1_warp, w_R, self.EBr1)):
            inp = torch.empty((B, 6, H, W), dtype=torch.float32, device=dev)                  # other_warp * w0 | own * w1   (:1470-1471)
            _hip.quantize(x_other_warp, "copy", out=inp, out_coff=0, gate=w, gate_c=0)
            _hip.quantize(x_own, "copy", out=inp, out_coff=3, gate=w, gate_c=1)
            if self.conv1.resident_supported(B, H, W):       # 6 -> 32 on the resident-weight kernel: one zero-padded record per pixel in, F16K out
                t = self.conv1.run_f16k_res(_F16K.from_nchw(inp))
            else:
                t = _F16K.from_nchw(self.conv1.run(inp))
            feats.append(EB1.forward_f16k(t))
        # stage 2: own * w1 | warp(other) * w0   (:1481-1482)
        c1 = _F16K.empty(B, 64, H, W, dev)
        c2 = _F16K.empty(B, 64, H, W, dev)
        c1.channels(0, 32).fill_gated(feats[0], gate=w_L, gate_c=1)
        c1.channels(32, 32).fill_gated(feats[1], gate=w_L, gate_c=0, minv=m_back)
        c2.channels(0, 32).fill_gated(feats[1], gate=w_R, gate_c=1)
        c2.channels(32, 32).fill_gated(feats[0], gate=w_R, gate_c=0, minv=m_fwd)
        for x_own, c, EB2, EB3 in ((x1_hat, c1, self.EBl2, self.EBl3), (x2_hat, c2, self.EBr2, self.EBr3)):
            d = _F16K.empty(B, 96, H, W, dev)                                                 # stage-2 output | conv0(x_hat)   (:1486-1487)
            EB2.forward_f16k(c, out=d.channels(0, 64))
            if self.conv0.resident_supported(B, H, W):       # 3 -> 32 straight into channels [64, 96) of the concat buffer
                self.conv0.run_f16k_res(_F16K.from_nchw(x_own), out=d.channels(64, 32))
            else:
                d.channels(64, 32).fill_from_nchw(self.conv0.run(x_own))
            o = EB3.forward_f16k(d)
            if self.conv2.few_supported(B, H, W):
                outs.append(self.conv2.run_f16k_few(o, res32=x_own))                          # 96 -> 3 on the MFMA kernel + the picture (:1495-1496)
            else:
                outs.append(self.conv2.run(o.to_nchw(), res1=x_own))
        return {"x1_hat": outs[0], "x2_hat": outs[1]}

    def _f16k_ok(self, B, H, W):
        return all(eb.f16k_supported(B, H, W) for eb in (self.EBl1, self.EBl2, self.EBl3, self.EBr1, self.EBr2, self.EBr3))

    def forward(self, x1_hat, x2_hat, h_matrix):
        if torch.is_grad_enabled() and h_matrix.requires_grad:
            raise NotImplementedError("Independent_EN.forward: no gradient with respect to h_matrix (its masks and warps treat it as data); "
                                      "detach h_matrix")
        if self._needs_graph(x1_hat, x2_hat):
            return self._forward_graph(x1_hat, x2_hat, h_matrix)
        x1_hat = x1_hat.contiguous()
        x2_hat = x2_hat.contiguous()
        B, _, H, W = x1_hat.shape
        dev, dt = x1_hat.device, x1_hat.dtype
        if _bf16_inference(x1_hat, x2_hat) and self._f16k_ok(B, H, W):
            return self._forward_f16k(x1_hat, x2_hat, h_matrix)
        m_fwd, m_back = _warp_matrices(h_matrix, (H, W), (H, W), want_inverse=True)
        mask_R = _hip.warp_perspective(None, m_fwd, (H, W), ones_like=(B, H, W))
        mask_L = _hip.warp_perspective(mask_R, m_back, (H, W))
        w_R = self.mask2weights_unit(mask_R)        # [B,2,H,W]
        w_L = self.mask2weights_unit(mask_L)
        x1_warp = _hip.warp_perspective(x1_hat, m_fwd, (H, W))
        x2_warp = _hip.warp_perspective(x2_hat, m_back, (H, W))
        x1c = self.conv0(x1_hat)
        x2c = self.conv0(x2_hat)

        in1 = torch.empty((B, 6, H, W), dtype=dt, device=dev)       # x2_warp*wL0 | x1*wL1   (:1470)
        _hip.quantize(x2_warp, "copy", out=in1, out_coff=0, gate=w_L, gate_c=0)
        _hip.quantize(x1_hat, "copy", out=in1, out_coff=3, gate=w_L, gate_c=1)
        in2 = torch.empty((B, 6, H, W), dtype=dt, device=dev)       # x1_warp*wR0 | x2*wR1   (:1471)
        _hip.quantize(x1_warp, "copy", out=in2, out_coff=0, gate=w_R, gate_c=0)
        _hip.quantize(x2_hat, "copy", out=in2, out_coff=3, gate=w_R, gate_c=1)
        out1 = self.EBl1(self.conv1(in1))
        out2 = self.EBr1(self.conv1(in2))

        out1_warp = _hip.warp_perspective(out1, m_fwd, (H, W))
        out2_warp = _hip.warp_perspective(out2, m_back, (H, W))
        c1 = torch.empty((B, 64, H, W), dtype=dt, device=dev)       # out1*wL1 | out2_warp*wL0   (:1481)
        _hip.quantize(out1, "copy", out=c1, out_coff=0, gate=w_L, gate_c=1)
        _hip.quantize(out2_warp, "copy", out=c1, out_coff=32, gate=w_L, gate_c=0)
        c2 = torch.empty((B, 64, H, W), dtype=dt, device=dev)       # out2*wR1 | out1_warp*wR0   (:1482)
        _hip.quantize(out2, "copy", out=c2, out_coff=0, gate=w_R, gate_c=1)
        _hip.quantize(out1_warp, "copy", out=c2, out_coff=32, gate=w_R, gate_c=0)
        out1 = self.EBl2(c1)
        out2 = self.EBr2(c2)

        d1 = torch.empty((B, 96, H, W), dtype=dt, device=dev)       # out1 | conv0(x1_hat)   (:1486)
        _hip.copy_view(out1, d1, 0)
        _hip.copy_view(x1c, d1, 64)
        d2 = torch.empty((B, 96, H, W), dtype=dt, device=dev)
        _hip.copy_view(out2, d2, 0)
        _hip.copy_view(x2c, d2, 64)
        out1 = self.EBl3(d1)
        out2 = self.EBr3(d2)
        return {"x1_hat": self.conv2.run(out1, res1=x1_hat), "x2_hat": self.conv2.run(out2, res1=x2_hat)}


class GMM_together(nn.Module):
    def __init__(self, N=128, M=192, K=5, **kwargs):
        super().__init__()
        self.m1 = HSIC(N, M, K)
        self.m2 = Independent_EN()

    def forward(self, x1, x2, h):
        out1 = self.m1(x1, x2, h)
        out2 = self.m2(out1["x1_hat"], out1["x2_hat"], h)
        return {"x1_hat": out2["x1_hat"], "x2_hat": out2["x2_hat"], "likelihoods": out1["likelihoods"]}
