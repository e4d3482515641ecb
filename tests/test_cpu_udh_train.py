"""The training stage of the UDH homography net without a GPU: the plain-torch restatement (tests/udh_train_ref.py) against the
reference's recorded step (tests/golden/udh_train.npz), its loss under gradcheck, and the interface of udh/udh/model.py.

Bound for every comparison with the reference: tests/util.assert_close semantics (error over the tensor's peak), limit
max(1e-4, 2 x the reference's own float32-against-float64 floor recorded in the fixture)."""
import numpy as np
import pytest
import torch

from tests import udh_train_ref as TR
from tests import udh_weights as UW
from tests.udh_train_cases import CASES, case_inputs, check_step, load_udh_model
from tests.util import load_npz


@pytest.fixture(scope="module")
def fx():
    return load_npz("udh_train.npz")


@pytest.mark.parametrize("index", range(len(CASES)))
def test_ref_reproduces_the_reference_step(fx, index):
    p = CASES[index][0]
    a, b, img, pb, corners, masks = case_inputs(fx, index)
    net = TR.Net(p)
    UW.fill(net, UW.WEIGHT_SEED)
    delta = net(a, b, masks)
    loss = TR.photometric_loss(delta, img, pb, corners)
    loss.backward()
    check_step(fx, index, loss, delta, {n: q.grad for n, q in net.named_parameters()}, "udh_train_ref")


def test_fixture_inputs_are_in_general_position(fx):
    most = 0.0
    for index in range(len(CASES)):
        a, b, img, pb, corners, masks = case_inputs(fx, index)
        net = TR.Net(CASES[index][0])
        UW.fill(net, UW.WEIGHT_SEED)
        assert TR.kink_margin(net.double(), a, b, masks) >= TR.KINK_MARGIN, index
        coord, diff, outside = TR.margins(torch.from_numpy(fx[f"c{index}/delta"]), img, pb, corners)
        assert coord > TR.MARGIN_COORD and diff >= TR.MARGIN_DIFF, (index, coord, diff)
        most = max(most, outside)
    assert most >= 0.01


def test_ref_loss_gradcheck():
    img, pb, corners = TR.loss_inputs([1, 2], (20, 24), (8, 12), 2.0)
    delta = torch.from_numpy(np.random.default_rng(5).uniform(-2, 2, (2, 4, 2))).requires_grad_(True)
    assert TR.in_general_position(delta, img, pb, corners)
    assert torch.autograd.gradcheck(lambda d: TR.photometric_loss(d, img.double(), pb.double(), corners.double()), (delta,),
                                    eps=1e-6, atol=1e-7, rtol=1e-4)


@pytest.mark.parametrize("p", [32, 64, 128])
def test_module_interface_and_state_dict(p):
    import model as codec_model
    M = load_udh_model()
    for name in ("Net", "Block", "Flatten", "photometric_loss"):
        assert hasattr(M, name), name
    sd, ref = M.Net(patch_size=p).state_dict(), codec_model.Net(patch_size=p).state_dict()
    assert list(sd) == list(ref) and len(sd) == 20
    for n in sd:
        assert tuple(sd[n].shape) == tuple(ref[n].shape), n
    assert list(sd) == list(TR.Net(p).state_dict())


def test_constructor_and_argument_errors():
    M = load_udh_model()
    with pytest.raises(NotImplementedError):
        M.Net(batch_norm=True)
    with pytest.raises(NotImplementedError):
        M.Block(2, 64, batch_norm=True)
    with pytest.raises(ValueError, match="256"):
        M.Net(patch_size=256)
    net = M.Net(patch_size=32)
    a, b = UW.patches(1, 1, 32)
    for mode in (True, False):
        net.train(mode)
        with pytest.raises(RuntimeError, match="CUDA"):
            net(a, b)                                  # CPU tensors: there is no CPU path
    img, pb, corners = TR.loss_inputs([1], (40, 48), (32, 32), 6.0)
    with pytest.raises(RuntimeError, match="CUDA"):
        M.photometric_loss(torch.zeros(1, 4, 2, requires_grad=True), img, pb, corners)
    import model as codec_model
    with pytest.raises(NotImplementedError, match="udh/udh/model.py"):
        codec_model.photometric_loss(None, None, None, None)
