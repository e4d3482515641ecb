"""The UDH homography net's module interface (coremasic/mywork/model.py) without a GPU: state-dict layout against the reference's
recorded one, checkpoint loading through the drivers' wrapper, the seeded weight helper, and the argument errors."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import udh_weights as UW
from tests.util import load_npz


@pytest.fixture(scope="module")
def fx():
    return load_npz("udh_net.npz")


@pytest.fixture(scope="module")
def model():
    import model
    return model


@pytest.mark.parametrize("p", [32, 64, 128])
def test_state_dict_names_and_shapes_match_the_reference(fx, model, p):
    sd = model.Net(patch_size=p).state_dict()
    names = [str(n) for n in fx[f"w{p}/names"]]
    assert list(sd) == names and len(names) == 20
    for n, shape in zip(names, fx[f"w{p}/shapes"]):
        assert tuple(sd[n].shape) == tuple(int(v) for v in shape[:sd[n].dim()]), n


def test_checkpoint_with_model_prefix_loads_through_the_drivers_wrapper(fx, model):
    class HomographyModel(nn.Module):                  # newtrain_codec_real.py / test3_real.py
        def __init__(self):
            super().__init__()
            self.model = model.Net(patch_size=32)

    arrays = UW.tensors(model.Net(patch_size=32).state_dict(), UW.WEIGHT_SEED)
    ckpt = {"state_dict": {"model." + k: torch.from_numpy(v) for k, v in arrays.items()}}
    wrapper = HomographyModel()
    wrapper.load_state_dict(ckpt["state_dict"])
    for k, v in arrays.items():
        assert np.array_equal(wrapper.model.state_dict()[k].numpy(), v), k


@pytest.mark.parametrize("p", [32, 64, 128])
def test_weight_helper_reproduces_the_recorded_weights(fx, model, p):
    arrays = UW.fill(model.Net(patch_size=p), UW.WEIGHT_SEED)
    for i, n in enumerate(fx[f"w{p}/names"]):
        s, head = UW.fingerprint(arrays[str(n)])
        assert s == float(fx[f"w{p}/sum"][i]), n
        assert np.array_equal(head, fx[f"w{p}/head"][i][:head.size]), n


def test_constructor_and_argument_errors(model):
    with pytest.raises(NotImplementedError):
        model.Net(batch_norm=True)
    with pytest.raises(NotImplementedError):
        model.Block(2, 64, batch_norm=True)
    with pytest.raises(ValueError):
        model.Net(patch_size=48)
    net = model.Net(patch_size=32)
    a, b = UW.patches(1, 1, 32)
    with pytest.raises(RuntimeError, match="eval"):
        net(a, b)                                      # a fresh module is in training mode
    net.eval()
    with pytest.raises(RuntimeError, match="CUDA"):
        net(a, b)                                      # CPU tensors: there is no CPU path
    with pytest.raises(RuntimeError, match="eval"):
        net.train()(a, b)
    with pytest.raises(NotImplementedError):
        model.photometric_loss(None, None, None, None)
