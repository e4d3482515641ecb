"""Seeded weights and inputs of the UDH homography net for the golden generator and the tests (plain numpy: PCG64 streams do not
depend on the torch build).  A checkpoint cannot be committed -- Linear 1 alone is 134 MB at patch size 128 -- so both sides rebuild
identical weights from the seed; tests/golden/udh_net.npz records each tensor's float64 sum and leading values to prove it."""
import numpy as np
import torch

WEIGHT_SEED = 7
CASES = ((32, 1), (32, 3), (64, 9), (128, 2))      # (patch_size, B)
SAMPLE_STRIDE = 7                                  # block outputs are recorded at every 7th element of the flattened tensor


def case_seed(p, B):
    return 1000 + 10 * p + B


def tensors(state_dict, seed):
    """name -> float32 array, drawn in state-dict order: He-scaled normals for weights, uniform(-0.1, 0.1) for biases."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, t in state_dict.items():
        shape = tuple(t.shape)
        if len(shape) > 1:
            fan_in = int(np.prod(shape[1:]))
            out[name] = (rng.standard_normal(shape, dtype=np.float32) * np.float32(np.sqrt(2.0 / fan_in))).astype(np.float32)
        else:
            out[name] = rng.uniform(-0.1, 0.1, shape).astype(np.float32)
    return out


def fill(net, seed):
    """Loads the seeded weights into `net` through load_state_dict (on the device the parameters live on); returns the arrays."""
    arrays = tensors(net.state_dict(), seed)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in arrays.items()})
    return arrays


def patches(seed, B, p):
    """Two [B,1,p,p] float32 standard-normal inputs."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((B, 1, p, p), dtype=np.float32)
    b = rng.standard_normal((B, 1, p, p), dtype=np.float32)
    return torch.from_numpy(a), torch.from_numpy(b)


def fingerprint(array):
    """(float64 sum, first four values) of a tensor."""
    flat = np.asarray(array).reshape(-1)
    return float(flat.astype(np.float64).sum()), flat[:4].astype(np.float32)
