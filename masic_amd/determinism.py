"""Deterministic mode: training steps whose results are bitwise reproducible.

By default the large weight gradients are split-K sums whose partial tiles are added with float atomics, so the order of the
adds -- and the last bits of every weight gradient -- depends on timing; Adam turns those bits into visibly different models after
a few steps.  With the mode on, the wrappers in masic_amd/ops.py call the `_det` entry points of the library instead
(include/masic_hip.h, "Deterministic mode"): each pixel split stores its partial tile into its own slab of a workspace and one
finishing launch sums the slabs in split order, and the warp backward's fallback for extreme homographies is a store-and-sum
instead of a float-atomic scatter.  Same inputs, noise, device model and library build give the same bits.  DESIGN.md section 13
has the layout and the cost; the default path is unchanged.

The effective mode is this module's flag OR torch.are_deterministic_algorithms_enabled(), so `torch.use_deterministic_algorithms(True)`
turns it on as well.  torch.backends.cudnn.deterministic is deliberately not read: it selects among cuDNN / MIOpen convolution
algorithms, which this library does not use, and PyTorch does not treat it as a request for determinism of other operators either.

The mode is read at call time, per call.  A captured graph (masic_amd.graph.GraphedTrainStep) replays the kernels of the mode that was in
effect at capture.
"""
import contextlib

import torch

_ON = False


def set_deterministic(on: bool):
    """Turn this module's flag on or off (torch.use_deterministic_algorithms can turn the mode on independently)."""
    global _ON
    _ON = bool(on)


def is_deterministic() -> bool:
    """The effective mode: this module's flag or torch's deterministic-algorithms switch."""
    return _ON or torch.are_deterministic_algorithms_enabled()


@contextlib.contextmanager
def deterministic(on: bool = True):
    """Set this module's flag for the duration of the block; the previous value is restored on exit, also after an exception."""
    prev = _ON
    set_deterministic(on)
    try:
        yield
    finally:
        set_deterministic(prev)
