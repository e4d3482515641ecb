"""The 128 -> 128 5x5 stride-2 convolution with fused forward GDN of the analysis transforms (g_a_conv2 / g_a_conv3) on a kernel of its
own (masic_amd/csrc/conv_s2_gdn.hip).

    if conv_s2.supported(cv, gdn, B, Hi, Wi):
        y = conv_s2.run(cv, gdn, x)        # x, y F16K values; the bits of cv.run_f16k(x, gdn=gdn)

Operands are conv_f16k's: the weight stream of `cv.packed_f16k_weight`, the GDN image of `nn.packed_gdn_f16k` -- no pack and no cache of
its own.  The form is fixed (bf16 F16K in and out without a channel view, one-product forward GDN); `supported` answers False for
everything else and the caller keeps conv_f16k for it.

The entry points are declared in include/masic_conv_s2.h, a side header of libmasic_hip.so bound by _lib.bind_header; the checks, the
launcher, `supported` and `run` are layer_kernel.GdnLayerKernel's.  No CPU path.
"""
from .layer_kernel import CHANNELS, GdnLayerKernel       # noqa: F401 (CHANNELS is one of this module's names)

PACKED_BYTES = 8 * 5 * 20480                      # the layer's slab stream: 8 chunks x 5 steps of 5 taps x 4 KiB


def out_hw(Hi, Wi):
    return (Hi - 1) // 2 + 1, (Wi - 1) // 2 + 1


_KERNEL = GdnLayerKernel("masic_conv_s2.h", "masic_conv_s2_", "conv_s2_gdn_f16k", transposed=False, inverse=False, packed_bytes=PACKED_BYTES,
                         out_hw=out_hw)
HEADER_PATH, SIGNATURES = _KERNEL.header_path, _KERNEL.signatures          # name -> (restype, argtypes) of every prototype of masic_conv_s2.h
kernel_name = _KERNEL.kernel_name                 # (B, Hi, Wi)
conv_s2_gdn_f16k = _KERNEL.launch                 # (x16, packed, bias, gdn_packed, B, Hi, Wi, out16=None)
supported, preferred, run = _KERNEL.supported, _KERNEL.preferred, _KERNEL.run          # preferred: wherever supported
