"""The 128 -> 128 transposed 5x5 stride-2 convolution with fused inverse GDN of the synthesis transforms (g_s_conv2 / g_s_conv3) on a
kernel of its own (masic_amd/csrc/deconv_igdn.hip).

    if deconv.supported(cv, gdn, B, Hi, Wi):
        y = deconv.run(cv, gdn, x)        # x, y F16K values; the bits of cv.run_f16k(x, gdn=gdn)

Operands are conv_f16k's: the weight stream of `cv.packed_f16k_weight`, the GDN image of `nn.packed_gdn_f16k` -- no pack and no cache of
its own.  The form is fixed (bf16 F16K in and out without a channel view, one-product inverse GDN); `supported` answers False for
everything else and the caller keeps conv_f16k for it.

The entry points are declared in include/masic_deconv.h, a side header of libmasic_hip.so bound by _lib.bind_header; the checks, the
launcher, `supported` and `run` are layer_kernel.GdnLayerKernel's.  No CPU path.
"""
from .layer_kernel import CHANNELS, GdnLayerKernel       # noqa: F401 (CHANNELS is one of this module's names)

PACKED_BYTES = 4 * (5 + 3 + 3 + 2) * 16384        # the layer's slab stream: 4 chunks x (5 + 3 + 3 + 2) steps of 2 taps x 2 blocks x 4 KiB
TILES = (0, 1, 2)                                 # 0: chosen from the shape, 1: 16 x 32 input pixels per workgroup, 2: 8 x 32
SPLITS = (0, 1, 2, 4)                             # workgroups per tile: 4 = one output phase each (what 0 chooses), 1 = all four phases

_KERNEL = GdnLayerKernel("masic_deconv.h", "masic_deconv_", "deconv_igdn_f16k", transposed=True, inverse=True, packed_bytes=PACKED_BYTES,
                         out_hw=lambda Hi, Wi: (2 * Hi, 2 * Wi), extras=(("tile", TILES), ("split", SPLITS)))
HEADER_PATH, SIGNATURES = _KERNEL.header_path, _KERNEL.signatures          # name -> (restype, argtypes) of every prototype of masic_deconv.h
kernel_name = _KERNEL.kernel_name                 # (B, Hi, Wi, tile=0, split=0)
deconv_igdn_f16k = _KERNEL.launch                 # (x16, packed, bias, gdn_packed, B, Hi, Wi, out16=None, tile=0, split=0): same bits for every tile and split
supported, preferred, run = _KERNEL.supported, _KERNEL.preferred, _KERNEL.run          # preferred: wherever supported
