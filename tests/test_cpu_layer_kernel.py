"""masic_amd/layer_kernel.py, the code behind masic_amd.deconv and masic_amd.conv_s2: the answers that need no device.  `supported`
refuses every form the kernels do not run -- on stand-ins for the convolution and the GDN (the GPU tests ask the same of real modules) --
the kernels' names are what they were, and with no KernelTimer installed the per-layer path builds no descriptor."""
import pytest
import torch

SHAPE = (1, 32, 64)


class _Conv:
    masked_conv = False
    in_channels = out_channels = 128

    def __init__(self, transposed, geometry=(5, 5, 2, 2), **attrs):
        self.transposed_conv, self.geometry = transposed, geometry
        self.__dict__.update(attrs)

    def _geometry(self):
        return self.geometry

    def f16k_supported(self, B, Hi, Wi):
        return True


class _Gdn:
    def __init__(self, inverse, channels=128):
        self.inverse, self.beta = inverse, torch.ones(channels)


def _module(name):
    import importlib
    return importlib.import_module("masic_amd." + name)


@pytest.mark.parametrize("name,transposed", [("deconv", True), ("conv_s2", False)])
def test_supported_refuses_every_other_form(name, transposed):
    from masic_amd import _lib, ops
    mod = _module(name)
    cv, gdn = _Conv(transposed), _Gdn(transposed)
    assert mod.supported(cv, gdn, *SHAPE) is True and mod.supported(cv, gdn, 8, 128, 128) is True
    assert not mod.supported(cv, None, *SHAPE)                                       # no GDN
    assert not mod.supported(_Conv(not transposed), gdn, *SHAPE)                     # the other direction of the convolution
    assert not mod.supported(_Conv(transposed, masked_conv=True), gdn, *SHAPE)       # a masked convolution
    assert not mod.supported(_Conv(transposed, in_channels=192), gdn, *SHAPE)        # 192 -> 128
    assert not mod.supported(_Conv(transposed, out_channels=192), gdn, *SHAPE)       # 128 -> 192
    assert not mod.supported(_Conv(transposed, geometry=(3, 3, 1, 1)), gdn, *SHAPE)  # another geometry
    assert not mod.supported(_Conv(transposed, geometry=(5, 5, 1, 2)), gdn, *SHAPE)
    assert not mod.supported(cv, _Gdn(not transposed), *SHAPE)                       # the other direction of the GDN
    assert not mod.supported(cv, _Gdn(transposed, 192), *SHAPE)                      # a GDN of another width
    assert not mod.supported(cv, gdn, *SHAPE, products=3)                            # the three-product contraction
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ops, "_FUSED_GDN_PRODUCTS", 3)
        assert not mod.supported(cv, gdn, *SHAPE)
        assert mod.supported(cv, gdn, *SHAPE, products=1)
    assert not mod.supported(cv, gdn, *SHAPE, out_ctot=160, out_coff=16)             # a channel view of the output
    assert not mod.supported(cv, gdn, *SHAPE, out_ctot=160)
    assert not mod.supported(cv, gdn, *SHAPE, in_ctot=160, in_coff=16)               # ... of the input
    assert not mod.supported(cv, gdn, *SHAPE, in_ctot=160)
    assert mod.supported(cv, gdn, *SHAPE, out_ctot=128, in_ctot=128)
    assert not mod.supported(cv, gdn, *SHAPE, prec=_lib.PREC_FP8)                    # fp8 operands
    assert not mod.supported(cv, gdn, *SHAPE, prec=_lib.PREC_F32)                    # float32
    assert not mod.supported(cv, gdn, *SHAPE, y_pre=torch.empty(1, dtype=torch.int16))   # the pre-GDN output of a training step
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, -1), (70000, 8, 8), (1, 4096, 4096)):  # the library's answer for the shape
        assert not mod.supported(cv, gdn, *bad), bad
    cv.f16k_supported = lambda B, Hi, Wi: False                                      # ... and the module's
    assert not mod.supported(cv, gdn, *SHAPE)


def test_kernel_names():
    deconv, conv_s2 = _module("deconv"), _module("conv_s2")
    assert deconv.kernel_name(8, 128, 128) == deconv.kernel_name(1, 8, 8, 1) == deconv.kernel_name(1, 8, 8, 1, 4) == "deconv_igdn_f16k<8, 2, 5>"
    assert deconv.kernel_name(8, 64, 64, split=1) == deconv.kernel_name(8, 32, 32) == deconv.kernel_name(8, 128, 128, tile=2) == "deconv_igdn_f16k<8, 1, 5>"
    assert conv_s2.kernel_name(8, 256, 256) == conv_s2.kernel_name(1, 5, 7) == "conv_s2_gdn_f16k"
    with pytest.raises(RuntimeError, match="bad arguments"):
        deconv.kernel_name(8, 32, 32, tile=3)
    with pytest.raises(TypeError):
        conv_s2.kernel_name(8, 32, 32, tile=1)
    with pytest.raises(TypeError):
        deconv.kernel_name(8, 32, 32, 1, 4, 0)


def test_public_names_and_constants():
    deconv, conv_s2 = _module("deconv"), _module("conv_s2")
    assert (deconv.CHANNELS, deconv.PACKED_BYTES, deconv.TILES, deconv.SPLITS) == (128, 4 * 13 * 16384, (0, 1, 2), (0, 1, 2, 4))
    assert (conv_s2.CHANNELS, conv_s2.PACKED_BYTES) == (128, 8 * 5 * 20480)
    assert conv_s2.out_hw(5, 7) == (3, 4) and conv_s2.out_hw(32, 64) == (16, 32)
    for f in (deconv.deconv_igdn_f16k, deconv.supported, deconv.run, conv_s2.conv_s2_gdn_f16k, conv_s2.supported, conv_s2.run):
        assert callable(f)


@pytest.mark.parametrize("name,transposed", [("deconv", True), ("conv_s2", False)])
def test_no_descriptor_is_built_without_a_timer(name, transposed, monkeypatch):
    """supported() sits on the eval forward's per-layer path: with no KernelTimer set it reaches neither make_conv_desc nor a header"""
    from masic_amd import _lib, ops

    def refuse(*a, **k):
        raise AssertionError("called on the per-layer path")

    assert ops._timer is None
    monkeypatch.setattr(ops, "make_conv_desc", refuse)
    monkeypatch.setattr(ops, "_make_conv_desc", refuse)
    monkeypatch.setattr(_lib, "parse_header", refuse)
    monkeypatch.setattr(_lib, "bind_header", refuse)
    mod = _module(name)
    assert mod.supported(_Conv(transposed), _Gdn(transposed), *SHAPE) is True
    assert mod.kernel_name(*SHAPE)


def test_operands_raise_runtime_error_on_the_cpu():
    """the launchers' operand checks come first: a CPU tensor is refused before anything reaches the library"""
    deconv, conv_s2 = _module("deconv"), _module("conv_s2")
    x = torch.zeros(1 * 128 * 8 * 8, dtype=torch.int16)
    with pytest.raises(RuntimeError, match="F16K int16 CUDA buffer"):
        deconv.deconv_igdn_f16k(x, x, None, x, 1, 8, 8, tile=7)
    with pytest.raises(RuntimeError, match="F16K int16 CUDA buffer"):
        conv_s2.conv_s2_gdn_f16k(x, x, None, x, 1, 8, 8)
