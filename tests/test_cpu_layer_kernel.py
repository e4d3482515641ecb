"""masic_amd/layer_kernel.py, the code behind masic_amd.deconv, conv_s2, latent and d2s_layer: the answers that need no device.  The
shape queries are host arithmetic, `supported` refuses every form the kernels do not run -- on stand-ins for the convolution and the GDN
(the GPU tests ask the same of real modules) -- the launchers' first checks refuse their operands before anything touches a device, the
kernels' names are what they were, and with no KernelTimer installed the per-layer path builds no descriptor."""
import ctypes
import types

import pytest
import torch

# module -> (direction of the convolution, has a fused GDN, out_channels, C prefix of its entry points, a shape it takes, bias length)
LAYERS = {
    "deconv": (True, True, 128, "masic_deconv_igdn_f16k", (1, 32, 64), 128),
    "conv_s2": (False, True, 128, "masic_conv_s2_gdn_f16k", (1, 32, 64), 128),
    "latent": (False, False, 192, "masic_latent_s2_f16k", (1, 32, 64), 192),
    "d2s_layer": (True, False, 3, "masic_d2s_layer_f16k", (8, 256, 256), 32),            # a shape of d2s_layer.ROW
}
DIRECTIONS = [(name, LAYERS[name][0]) for name in LAYERS]
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

    f16k_multi_supported = d2s_supported = f16k_supported


class _Gdn:
    def __init__(self, inverse, channels=128):
        self.inverse, self.beta = inverse, torch.ones(channels)


def _module(name):
    import importlib
    return importlib.import_module("masic_amd." + name)


def _launch(name):
    mod = _module(name)
    return {"deconv": lambda: mod.deconv_igdn_f16k, "conv_s2": lambda: mod.conv_s2_gdn_f16k}.get(name, lambda: mod.launch)()


@pytest.mark.parametrize("name", LAYERS)
def test_shape_queries_need_no_gpu(name):
    """supported / preferred / kernel_name are host arithmetic: the shape limit and the name, then each rule of `preferred`"""
    from masic_amd import _lib
    mod, lib, stem = _module(name), _lib.lib, LAYERS[name][3]
    big = {"deconv": (8, 128, 128), "conv_s2": (8, 256, 256), "latent": (8, 64, 64), "d2s_layer": (8, 256, 256)}[name]
    assert getattr(lib, stem + "_supported")(1, 5, 7) == 1 and getattr(lib, stem + "_supported")(*big) == 1
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, -1), (70000, 8, 8), (1, 4096, 4096)) + (((1, 2048, 2048),) if name == "latent" else ()):
        assert getattr(lib, stem + "_supported")(*bad) == 0, bad
        assert name in ("deconv", "conv_s2") or getattr(lib, stem + "_preferred")(*bad) == 0, bad
    with pytest.raises(RuntimeError, match="bad arguments"):
        mod.kernel_name(0, 8, 8)
    extras = (0, 0) if name == "deconv" else ()
    assert getattr(lib, stem + "_kernel_name")(1, 5, 7, *extras, ctypes.create_string_buffer(8), 8) != 0       # a buffer too small
    if name in ("deconv", "conv_s2"):                                   # no rule of their own: wherever supported
        assert mod.preferred(None, *big) is True and mod.preferred(None, 1, 5, 7) is True
    if name == "latent":        # a threshold on the workgroup count (tiles of 4 x 32 output pixels, times B): 0 at two, 1 at the benchmark's 64
        assert mod.kernel_name(8, 64, 64) == mod.kernel_name(1, 5, 7) == "conv_s2_latent_f16k"
        assert not mod.preferred(None, 2, 8, 16) and mod.preferred(None, 8, 64, 64)
        took = [bool(lib.masic_latent_s2_f16k_preferred(8, 8 * k, 2)) for k in range(1, 33)]                 # 8 k workgroups
        assert took == sorted(took) and took[-1], "one threshold on the workgroup count"
    if name == "d2s_layer":     # never a shape conv_f16k runs on another row than ROW, and one threshold on that row's tile count
        assert mod.kernel_name(8, 256, 256) == mod.kernel_name(1, 5, 7) == "d2s_layer_f16k"
        shapes = [(8, 256, 256), (8, 128, 128), (1, 256, 256), (57, 65, 65), (88, 33, 65), (512, 32, 32), (511, 32, 32), (4096, 16, 31),
                  (8, 255, 225), (8, 256, 224), (16, 192, 160), (2, 512, 512), (1, 5, 7)]
        for s in shapes:
            if mod.preferred(None, *s):
                assert mod.takes_row(*s), s
        assert mod.takes_row(8, 256, 256) and mod.takes_row(57, 65, 65) and mod.takes_row(88, 33, 65)
        assert not mod.takes_row(8, 128, 128) and not mod.preferred(None, 8, 128, 128) and not mod.preferred(None, 1, 256, 256)
        took = [bool(lib.masic_d2s_layer_f16k_preferred(8 * k, 32, 32)) for k in range(1, 129)]             # 8 k tiles of conv_f16k
        assert took == sorted(took), "one threshold on the tile count"


@pytest.mark.parametrize("name,transposed", DIRECTIONS)
def test_supported_refuses_every_other_form(name, transposed):
    from masic_amd import _lib, ops
    mod = _module(name)
    _, fused, out_channels, _, shape, _ = LAYERS[name]
    cv, gdn = _Conv(transposed, out_channels=out_channels), _Gdn(transposed)
    form = (gdn,) if fused else ()                                                   # supported(cv, gdn, B, Hi, Wi, ...) / (cv, B, Hi, Wi, ...)

    def layer(direction=transposed, **attrs):
        return _Conv(direction, **dict(dict(out_channels=out_channels), **attrs))

    assert mod.supported(cv, *form, *shape) is True and (name == "d2s_layer" or mod.supported(cv, *form, 8, 128, 128) is True)
    assert not mod.supported(layer(not transposed), *form, *shape)                   # the other direction of the convolution
    assert not mod.supported(layer(masked_conv=True), *form, *shape)                 # a masked convolution
    assert not mod.supported(layer(in_channels=192), *form, *shape)                  # other widths
    assert not mod.supported(layer(in_channels=96), *form, *shape)
    assert not mod.supported(layer(out_channels={128: 192, 192: 128, 3: 9}[out_channels]), *form, *shape)
    assert not mod.supported(layer(geometry=(3, 3, 1, 1)), *form, *shape)            # another geometry
    assert not mod.supported(layer(geometry=(5, 5, 1, 2)), *form, *shape)
    assert not mod.supported(layer(geometry=(3, 3, 2, 1)), *form, *shape)
    assert not mod.supported(cv, *form, *shape, in_ctot=160, in_coff=16)             # a channel view of the input
    assert not mod.supported(cv, *form, *shape, in_ctot=160)
    assert mod.supported(cv, *form, *shape, in_ctot=128)
    assert not mod.supported(cv, *form, *shape, prec=_lib.PREC_FP8)                  # fp8 operands
    assert not mod.supported(cv, *form, *shape, prec=_lib.PREC_F32)                  # float32
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, -1), (70000, 8, 8), (1, 4096, 4096)):  # the library's answer for the shape
        assert not mod.supported(cv, *form, *bad), bad
    if fused:
        assert not mod.supported(cv, None, *shape)                                   # no GDN
        assert not mod.supported(cv, _Gdn(not transposed), *shape)                   # the other direction of the GDN
        assert not mod.supported(cv, _Gdn(transposed, 192), *shape)                  # a GDN of another width
        assert not mod.supported(cv, gdn, *shape, products=3)                        # the three-product contraction
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(ops, "_FUSED_GDN_PRODUCTS", 3)
            assert not mod.supported(cv, gdn, *shape)
            assert mod.supported(cv, gdn, *shape, products=1)
        assert not mod.supported(cv, gdn, *shape, out_ctot=160, out_coff=16)         # a channel view of the output
        assert not mod.supported(cv, gdn, *shape, out_ctot=160)
        assert mod.supported(cv, gdn, *shape, out_ctot=128, in_ctot=128)
        assert not mod.supported(cv, gdn, *shape, y_pre=torch.empty(1, dtype=torch.int16))   # the pre-GDN output of a training step
    if name == "d2s_layer":
        assert not mod.supported(cv, 8, 128, 128)                                    # conv_f16k's 32-channel-chunk row: another stream
        assert mod.supported(layer(out_channels=8), *shape) and not mod.supported(layer(out_channels=0), *shape)
    cv.f16k_supported = cv.f16k_multi_supported = cv.d2s_supported = lambda B, Hi, Wi: False     # ... and the module's
    assert not mod.supported(cv, *form, *shape)


def test_kernel_names():
    deconv, conv_s2 = _module("deconv"), _module("conv_s2")
    assert deconv.kernel_name(8, 128, 128) == deconv.kernel_name(1, 8, 8, 1) == deconv.kernel_name(1, 8, 8, 1, 4) == "deconv_igdn_f16k<8, 2, 5>"
    assert deconv.kernel_name(8, 64, 64, split=1) == deconv.kernel_name(8, 32, 32) == deconv.kernel_name(8, 128, 128, tile=2) == "deconv_igdn_f16k<8, 1, 5>"
    assert conv_s2.kernel_name(8, 256, 256) == conv_s2.kernel_name(1, 5, 7) == "conv_s2_gdn_f16k"
    with pytest.raises(RuntimeError, match="bad arguments"):
        deconv.kernel_name(8, 32, 32, tile=3)
    for name in ("conv_s2", "latent", "d2s_layer"):
        with pytest.raises(TypeError):
            _module(name).kernel_name(8, 32, 32, tile=1)
    with pytest.raises(TypeError):
        deconv.kernel_name(8, 32, 32, 1, 4, 0)


def test_public_names_and_constants():
    deconv, conv_s2, latent, d2s_layer = (_module(name) for name in LAYERS)
    assert (deconv.CHANNELS, deconv.PACKED_BYTES, deconv.TILES, deconv.SPLITS) == (128, 4 * 13 * 16384, (0, 1, 2), (0, 1, 2, 4))
    assert (conv_s2.CHANNELS, conv_s2.PACKED_BYTES) == (128, 8 * 5 * 20480)
    assert conv_s2.out_hw(5, 7) == (3, 4) and conv_s2.out_hw(32, 64) == (16, 32)
    assert (latent.IN_CHANNELS, latent.OUT_CHANNELS, latent.PACKED_BYTES) == (128, 192, 2 * 8 * 5 * 20480)
    assert latent.out_hw(5, 7) == (3, 4) and latent.out_hw(33, 130) == (17, 65)
    assert latent.WANT == ("y32", "round32", "round16", "abs16")
    assert (d2s_layer.IN_CHANNELS, d2s_layer.MAX_OUT_CHANNELS, d2s_layer.PACKED_BYTES) == (128, 8, 8 * 5 * 2 * 4096)
    assert d2s_layer.ROW == "conv_f16k<1, 2, 3, 5, 2, false, 1, 4, false>" and d2s_layer.conv_desc(1, 5, 7).Cout == 32
    for mod in (deconv, conv_s2, latent, d2s_layer):
        for f in (_launch(mod.__name__.rsplit(".", 1)[1]), mod.supported, mod.preferred, mod.run, mod.kernel_name):
            assert callable(f)
        assert mod.HEADER_PATH.endswith(".h") and mod.SIGNATURES


@pytest.mark.parametrize("name,transposed", DIRECTIONS)
def test_no_descriptor_is_built_without_a_timer(name, transposed, monkeypatch):
    """supported() and preferred() sit on the eval forward's per-layer path: with no KernelTimer set they reach neither make_conv_desc nor
    a header.  (d2s_layer.supported asks conv_f16k's plan once per shape, takes_row: its preferred and kernel_name only.)"""
    from masic_amd import _lib, ops

    def refuse(*a, **k):
        raise AssertionError("called on the per-layer path")

    assert ops._timer is None
    monkeypatch.setattr(ops, "make_conv_desc", refuse)
    monkeypatch.setattr(ops, "_make_conv_desc", refuse)
    monkeypatch.setattr(_lib, "parse_header", refuse)
    monkeypatch.setattr(_lib, "bind_header", refuse)
    mod = _module(name)
    _, fused, out_channels, _, shape, _ = LAYERS[name]
    if name != "d2s_layer":
        assert mod.supported(_Conv(transposed, out_channels=out_channels), *((_Gdn(transposed),) if fused else ()), *SHAPE) is True
    assert mod.preferred(None, *shape) in (True, False)
    assert mod.kernel_name(*SHAPE)


def test_operands_raise_runtime_error_on_the_cpu():
    """the launchers' operand checks come first: a CPU tensor is refused before anything reaches the library"""
    deconv, conv_s2, latent, d2s_layer = (_module(name) for name in LAYERS)
    x = torch.zeros(1 * 128 * 8 * 8, dtype=torch.int16)
    with pytest.raises(RuntimeError, match="F16K int16 CUDA buffer"):
        deconv.deconv_igdn_f16k(x, x, None, x, 1, 8, 8, tile=7)
    with pytest.raises(RuntimeError, match="F16K int16 CUDA buffer"):
        conv_s2.conv_s2_gdn_f16k(x, x, None, x, 1, 8, 8)
    with pytest.raises(RuntimeError, match="F16K int16 CUDA buffer"):
        latent.launch(x, x, None, 1, 8, 8, want=("nothing",))
    with pytest.raises(RuntimeError, match="F16K int16 CUDA buffer"):
        d2s_layer.launch(x, torch.empty(d2s_layer.PACKED_BYTES // 2, dtype=torch.int16), None, 1, 8, 8, 3)


@pytest.mark.parametrize("name", LAYERS)
def test_launch_refuses_a_wrong_pack_and_bias(name):
    """the checks that come before anything touches a device, on stand-ins for device tensors"""
    mod, launch, n_bias = _module(name), _launch(name), LAYERS[name][5]
    rest = {"deconv": (None,), "conv_s2": (None,)}.get(name, ()) + (1, 5, 7) + ((3,) if name == "d2s_layer" else ())
    meta = torch.device("meta")
    xm = types.SimpleNamespace(dtype=torch.int16, is_cuda=True, numel=lambda: 128 * 5 * 7, device=meta)
    pm = types.SimpleNamespace(dtype=torch.int16, numel=lambda: mod.PACKED_BYTES // 2 - 1, device=meta)
    with pytest.raises(RuntimeError, match="slab stream"):                               # a wrong pack size
        launch(xm, pm, None, *rest)
    pm = types.SimpleNamespace(dtype=torch.int16, numel=lambda: mod.PACKED_BYTES // 2, device=torch.device("cpu"))
    with pytest.raises(RuntimeError, match="slab stream"):                               # a pack on another device
        launch(xm, pm, None, *rest)
    pm = types.SimpleNamespace(dtype=torch.float32, numel=lambda: mod.PACKED_BYTES // 2, device=meta)
    with pytest.raises(RuntimeError, match="slab stream"):                               # a pack of another type
        launch(xm, pm, None, *rest)
    pm = types.SimpleNamespace(dtype=torch.int16, numel=lambda: mod.PACKED_BYTES // 2, device=meta)
    with pytest.raises(RuntimeError, match="bias must be a CUDA"):                       # a bias on another device
        launch(xm, pm, torch.zeros(n_bias), *rest)
