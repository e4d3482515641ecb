"""CPU checks of the LPIPS port (no GPU): the `lpips` name and lpips 0.1.4's signatures, the state-dict layout, reading trained
weights from files (never a download), the errors raised before any device work, and the restatement of tests/test_gpu_lpips.py
against closed forms and torch's own modules."""
import inspect
import json
import os

import pytest
import torch
import torch.nn as nn

from tests.test_gpu_lpips import CHNS, SCALE, SHIFT, ref_distance, ref_features, ref_lpips, ref_normalize, ref_scaling
from tests.util import GOLDEN


def _params(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]


def _rand_model():
    import lpips
    return lpips.LPIPS(pnet_rand=True, pretrained=False, verbose=False)


def test_lpips_exposes_the_hip_port_with_0_1_4_signatures():
    import lpips
    from masic_amd import lpips as L
    assert lpips.LPIPS is L.LPIPS and issubclass(lpips.LPIPS, nn.Module)
    E = inspect.Parameter.empty
    assert _params(lpips.LPIPS.__init__) == [("self", E), ("pretrained", True), ("net", "alex"), ("version", "0.1"), ("lpips", True),
                                             ("spatial", False), ("pnet_rand", False), ("pnet_tune", False), ("use_dropout", True),
                                             ("model_path", None), ("eval_mode", True), ("verbose", True)]
    assert _params(lpips.LPIPS.forward) == [("self", E), ("in0", E), ("in1", E), ("retPerLayer", False), ("normalize", False)]


def test_state_dict_has_lpips_layout():
    m = _rand_model()
    sd = m.state_dict()
    golden = json.load(open(os.path.join(GOLDEN, "lpips_state_keys.json")))
    assert len(golden) == 22
    assert [(k, list(v.shape)) for k, v in sd.items()] == [(g["key"], g["shape"]) for g in golden]
    assert all(v.dtype == torch.float32 for v in sd.values())
    for i, c in enumerate(CHNS):
        a, b = sd[f"lin{i}.model.1.weight"], sd[f"lins.{i}.model.1.weight"]
        assert tuple(a.shape) == (1, c, 1, 1) and a.data_ptr() == b.data_ptr()
    assert torch.equal(sd["scaling_layer.shift"].flatten(), torch.tensor(SHIFT))
    assert torch.equal(sd["scaling_layer.scale"].flatten(), torch.tensor(SCALE))
    assert not m.training and not any(p.requires_grad for p in m.parameters())


def _write_weight_files(tmp_path, monkeypatch, seed=3):
    """An alex.pth with the five lin keys and a backbone file in torchvision's layout under a private TORCH_HOME."""
    import lpips
    from masic_amd import lpips as L
    monkeypatch.setenv("TORCH_HOME", str(tmp_path / "torch_home"))
    g = torch.Generator().manual_seed(seed)
    lin = {f"lin{i}.model.1.weight": torch.rand(1, c, 1, 1, generator=g) for i, c in enumerate(CHNS)}
    src = _rand_model().state_dict()
    backbone = {}
    for key in ("net.slice1.0", "net.slice2.3", "net.slice3.6", "net.slice4.8", "net.slice5.10"):
        idx = key.rsplit(".", 1)[1]
        backbone[f"features.{idx}.weight"] = torch.randn(src[key + ".weight"].shape, generator=g)
        backbone[f"features.{idx}.bias"] = torch.randn(src[key + ".bias"].shape, generator=g)
    backbone["classifier.1.weight"] = torch.zeros(2, 2)          # the real file holds the classifier too
    lin_path = str(tmp_path / "alex.pth")
    assert L.backbone_path() == os.path.join(str(tmp_path / "torch_home"), "hub", "checkpoints", "alexnet-owt-7be5be79.pth")
    return lpips, lin, backbone, lin_path, L.backbone_path()


def test_trained_weights_round_trip_through_files(tmp_path, monkeypatch):
    lpips, lin, backbone, lin_path, net_path = _write_weight_files(tmp_path, monkeypatch)
    torch.save(lin, lin_path)
    os.makedirs(os.path.dirname(net_path))
    torch.save(backbone, net_path)
    m = lpips.LPIPS(net="alex", spatial=False, model_path=lin_path, verbose=False)
    sd = m.state_dict()
    for i in range(5):
        assert torch.equal(sd[f"lin{i}.model.1.weight"], lin[f"lin{i}.model.1.weight"])
        assert torch.equal(sd[f"lins.{i}.model.1.weight"], lin[f"lin{i}.model.1.weight"])
    for key in ("net.slice1.0", "net.slice2.3", "net.slice3.6", "net.slice4.8", "net.slice5.10"):
        idx = key.rsplit(".", 1)[1]
        assert torch.equal(sd[key + ".weight"], backbone[f"features.{idx}.weight"])
        assert torch.equal(sd[key + ".bias"], backbone[f"features.{idx}.bias"])
    # its own state dict loads back (22 keys, strict)
    m2 = _rand_model()
    m2.load_state_dict(sd)
    assert all(torch.equal(a, b) for a, b in zip(m2.state_dict().values(), sd.values()))
    # lin weights only / backbone only
    m3 = lpips.LPIPS(pnet_rand=True, model_path=lin_path, verbose=False)
    assert torch.equal(m3.lin4.model[1].weight, lin["lin4.model.1.weight"])
    m4 = lpips.LPIPS(pretrained=False, verbose=False)
    assert torch.equal(m4.net.slice5[0].weight, backbone["features.10.weight"])


def test_missing_weight_files_name_both_paths(tmp_path, monkeypatch):
    lpips, lin, backbone, lin_path, net_path = _write_weight_files(tmp_path, monkeypatch)
    with pytest.raises(FileNotFoundError) as e:
        lpips.LPIPS(model_path=lin_path, verbose=False)
    assert lin_path in str(e.value) and net_path in str(e.value)
    from masic_amd import lpips as L
    with pytest.raises(FileNotFoundError) as e:
        lpips.LPIPS(verbose=False)
    assert L.default_model_path() in str(e.value) and net_path in str(e.value)
    assert L.default_model_path().endswith(os.path.join("lpips", "weights", "v0.1", "alex.pth"))
    torch.save(lin, lin_path)                                     # the lin file alone is not enough for the default constructor
    with pytest.raises(FileNotFoundError) as e:
        lpips.LPIPS(model_path=lin_path, verbose=False)
    assert lin_path in str(e.value) and net_path in str(e.value)


def test_what_is_not_built_raises():
    import lpips
    for kw in (dict(net="vgg"), dict(net="squeeze"), dict(version="0.0"), dict(spatial=True), dict(lpips=False), dict(pnet_tune=True)):
        with pytest.raises(NotImplementedError):
            lpips.LPIPS(pnet_rand=True, pretrained=False, verbose=False, **kw)


def test_argument_errors_before_the_device():
    m = _rand_model()
    x = torch.rand(2, 3, 40, 48)
    with pytest.raises(ValueError):
        m(x[0], x[0])                                   # not 4-D
    with pytest.raises(ValueError):
        m(x[:, :1], x[:, :1])                           # not 3 channels
    with pytest.raises(ValueError):
        m(x, x[:, :, :32])                              # differing shapes
    with pytest.raises(ValueError):
        m(x.double(), x.double())                       # dtype
    with pytest.raises(ValueError):
        m(x, x.half())
    with pytest.raises(ValueError):
        m(x[:, :, :30], x[:, :, :30])                   # a side below 31
    with pytest.raises(ValueError):
        m(x[:, :, :, :30], x[:, :, :, :30])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(x[:, :, :31, :31].contiguous(), x[:, :, :31, :31].contiguous())
    xg = x.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError):
        m(xg, x)
    with pytest.raises(NotImplementedError):
        m(x, xg)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        m(xg, x)                                        # under no_grad the evaluators' call is admitted (and stops at the CPU tensor)
    m.train()
    with pytest.raises(NotImplementedError):
        m(x, x)
    t = _rand_model()
    assert not t.training
    import lpips
    assert lpips.LPIPS(pnet_rand=True, pretrained=False, verbose=False, eval_mode=False).training


# ---------------------------------------------------------------- the restatement against closed forms
def _sd64(seed=9):
    torch.manual_seed(seed)
    sd = {k: v.double() for k, v in _rand_model().state_dict().items()}
    g = torch.Generator().manual_seed(seed)
    for i, c in enumerate(CHNS):
        sd[f"lin{i}.model.1.weight"] = torch.rand(1, c, 1, 1, generator=g, dtype=torch.float64)
    return sd


def test_restatement_identical_inputs_give_zero():
    sd = _sd64()
    x = torch.rand(2, 3, 40, 52, dtype=torch.float64)
    val, res = ref_lpips(x, x.clone(), sd, normalize=True)
    assert torch.equal(val, torch.zeros(2, 1, 1, 1, dtype=torch.float64)) and len(res) == 5


def test_restatement_one_pixel_case_by_hand():
    """Features (3, 4) and (0, 5) at one pixel: unit vectors (.6, .8) and (0, 1); weights (2, 10): 2 * .36 + 10 * .04 = 1.12."""
    import lpips  # noqa: F401
    f0 = torch.tensor([3.0, 4.0], dtype=torch.float64).view(1, 2, 1, 1)
    f1 = torch.tensor([0.0, 5.0], dtype=torch.float64).view(1, 2, 1, 1)
    lin = torch.tensor([2.0, 10.0], dtype=torch.float64)
    assert abs(float(ref_distance(f0, f1, lin)) - 1.12) < 1e-9
    assert torch.allclose(ref_normalize(f0).flatten(), torch.tensor([0.6, 0.8], dtype=torch.float64), atol=1e-9, rtol=0)
    # an all-zero pixel is 0 / 1e-10 = 0, so its distance to a unit vector is the weight sum over that vector's squares
    z = torch.zeros_like(f0)
    assert float(ref_distance(z, z, lin)) == 0.0
    assert abs(float(ref_distance(z, f0, lin)) - (2 * 0.36 + 10 * 0.64)) < 1e-9
    # the spatial mean: two pixels, one of them identical in both pictures
    f0b, f1b = torch.cat([f0, f0], dim=3), torch.cat([f1, f0], dim=3)
    assert abs(float(ref_distance(f0b, f1b, lin)) - 0.56) < 1e-9
    # scaling layer by hand, with and without normalize
    x = torch.full((1, 3, 1, 1), 0.5, dtype=torch.float64)
    want = torch.tensor([(0.5 - s) / c for s, c in zip(SHIFT, SCALE)], dtype=torch.float64)
    assert torch.allclose(ref_scaling(x).flatten(), want, atol=1e-7, rtol=0)
    want_n = torch.tensor([(0.0 - s) / c for s, c in zip(SHIFT, SCALE)], dtype=torch.float64)
    assert torch.allclose(ref_scaling(x, normalize=True).flatten(), want_n, atol=1e-7, rtol=0)


def test_restatement_feature_stack_equals_torch_modules():
    """torchvision's alexnet.features, built from torch's own modules with the same weights, tapped after each ReLU."""
    sd = _sd64()
    feats = nn.Sequential(
        nn.Conv2d(3, 64, kernel_size=11, stride=4, padding=2), nn.ReLU(), nn.MaxPool2d(kernel_size=3, stride=2),
        nn.Conv2d(64, 192, kernel_size=5, padding=2), nn.ReLU(), nn.MaxPool2d(kernel_size=3, stride=2),
        nn.Conv2d(192, 384, kernel_size=3, padding=1), nn.ReLU(),
        nn.Conv2d(384, 256, kernel_size=3, padding=1), nn.ReLU(),
        nn.Conv2d(256, 256, kernel_size=3, padding=1), nn.ReLU()).double()
    for key, idx in (("net.slice1.0", 0), ("net.slice2.3", 3), ("net.slice3.6", 6), ("net.slice4.8", 8), ("net.slice5.10", 10)):
        with torch.no_grad():
            feats[idx].weight.copy_(sd[key + ".weight"])
            feats[idx].bias.copy_(sd[key + ".bias"])
    x = torch.rand(1, 3, 67, 93, dtype=torch.float64)
    taps = ref_features(x, sd, normalize=False)
    h, want = ref_scaling(x), []
    with torch.no_grad():
        for idx, layer in enumerate(feats):
            h = layer(h)
            if idx in (1, 4, 7, 9, 11):
                want.append(h)
    assert [tuple(t.shape) for t in taps] == [(1, 64, 16, 22), (1, 192, 7, 10), (1, 384, 3, 4), (1, 256, 3, 4), (1, 256, 3, 4)]
    for a, b in zip(taps, want):
        assert torch.allclose(a, b, atol=1e-12, rtol=1e-12)
