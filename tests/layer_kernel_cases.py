"""What the GPU tests of the own-layer kernels (tests/test_gpu_deconv_igdn.py, tests/test_gpu_conv_s2_gdn.py) share: the one-product GDN
setting, prefilled output buffers, and a layer's operands with the output of the kernel it stands for, conv_f16k."""
import torch

from tests import f16k_ref as R
from tests.test_gpu_f16k_rows import _gdn_params

DEV = "cuda"


class one_product:
    """the fused GDN in its one-product form inside the block; the setting found is put back"""

    def __enter__(self):
        from masic_amd import ops
        self.was = ops._FUSED_GDN_PRODUCTS
        ops.set_fused_gdn_products(1)

    def __exit__(self, *exc):
        from masic_amd import ops
        ops.set_fused_gdn_products(self.was)
        return False


def prefilled(case):
    """an F16K output buffer of the case, every value R.PREFILL_BITS"""
    Ho, Wo = R.out_hw(case)
    return torch.full((case.B * 128 * Ho * Wo,), R.PREFILL_BITS, dtype=torch.int16, device=DEV)


def operands(case, seed, gdn_seed, inverse, out16=None):
    """x16, packed weights, bias, packed GDN on the device and conv_f16k's output (into out16 if given), on the CPU, for a 128 -> 128
    case of tests/f16k_ref.py: the inputs of R.inputs(case, seed), the GDN parameters of the row test's generator"""
    from masic_amd import ops
    x, w, bias = R.inputs(case, seed)
    beta, gamma = _gdn_params(gdn_seed)
    d = R.desc_of(case)
    x16, wp, bd = R.to_f16k(x).to(DEV), ops.pack_conv_f16k_weight(w.to(DEV), d), bias.to(DEV)
    gp = ops.pack_gdn_f16k(beta.to(DEV), gamma.to(DEV))
    with one_product():
        want = ops.conv2d_f16k(x16, wp, bd, d, gdn=(gp, inverse), out16=out16)
    torch.cuda.synchronize()
    return x16, wp, bd, gp, want.cpu()
