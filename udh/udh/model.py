"""Training-stage module of the UDH homography net, MI355X-native (module signature of the reference's udh/udh/model.py).

`from model import Net, photometric_loss` gives udh/udh/train.py the names it imports: `Net(patch_size=p)` with the reference's 20
state-dict tensors, trainable through HIP kernels, and the photometric loss with its gradient.  The implementation and its
contracts (dropout masks, float32 operands, no CPU path) are in masic_amd/udh_train.py.  The codec-side
coremasic/mywork/model.py keeps the same names for the frozen, inference-only net; a checkpoint trained here loads there unchanged.
"""
from masic_amd.udh_train import Block, Flatten, Net, photometric_loss  # noqa: F401

__all__ = ["Net", "Block", "Flatten", "photometric_loss"]
