"""Homography without a trained net: the eight corner offsets of a grey patch pair by coarse-to-fine photometric alignment, one HIP
launch for the whole batch (masic_amd/csrc/align.hip).

    delta, info = align_patches(a, b)                  # a, b float32 [B,1,P,P] on the device, P in {32, 64, 128}
    codec = StereoCodec(hsic, PatchAligner().eval())   # encode without weights for the homography

`delta` [B,4,2] has the meaning of the UDH net's output and of `udh_train.photometric_loss(delta, a, b, s)`: b(u) ~ a(W(u)) with
W(s_k) = s_k + delta_k on the square s = (0,0), (P,0), (P,P), (0,P).  `info` [B,4] holds the masked MSE at the start value, the
masked MSE and the valid fraction at the returned delta, and a status: 0 the estimate, 1 a guard fired (non-finite input, fewer
than a quarter of the pixels valid, a non-positive pivot, a corner outside [-P/2, 3P/2]), 2 the result's MSE exceeds the start's.
With status 1 or 2 `delta` is the start value (`delta0`, or zeros) exactly.  The result is bit-reproducible and an item's bits depend
on neither B nor its batch mates.

The entry points are declared in include/masic_align.h, a side header of libmasic_hip.so bound by _lib.bind_header.  No CPU path:
tensors must live on an MI355X (`cuda`) device.
"""
import torch
import torch.nn as nn

from . import _lib
from .ops import _dev, _p, _stream

HEADER_PATH = _lib.header_path("masic_align.h")
PATCH_SIZES = (32, 64, 128)
ITERS = (30, 15, 10)              # Gauss-Newton steps, coarse to fine; the last `levels` entries are used


SIGNATURES = _lib.bind_header(HEADER_PATH, "masic_align_")          # name -> (restype, argtypes) of every prototype of masic_align.h


def align_patches(a, b, delta0=None, *, search_radius=12, iters=ITERS, damping=1e-6):
    """(delta [B,4,2], info [B,4]) float32 from grey patches a, b float32 [B,1,P,P] on the device.  delta0 [B,4,2] (optional): the
    start value; it replaces the integer translation search in [-search_radius, search_radius]^2 on the 32 x 32 level.  iters: three
    Gauss-Newton step counts, coarse to fine (the last one or two are used at P = 32 or 64)."""
    _dev(a, "a"); _dev(b, "b")
    if a.dim() != 4 or a.shape[1] != 1 or a.shape[2] != a.shape[3] or a.shape[2] not in PATCH_SIZES or b.shape != a.shape or a.shape[0] < 1:
        raise ValueError(f"masic_amd.align_patches: a and b must be [B,1,P,P] with P in {PATCH_SIZES} and B >= 1, got {tuple(a.shape)} and "
                         f"{tuple(b.shape)}")
    B, P = a.shape[0], a.shape[2]
    if b.device != a.device:
        raise ValueError("masic_amd.align_patches: a and b live on different devices")
    if delta0 is not None:
        _dev(delta0, "delta0")
        if tuple(delta0.shape) != (B, 4, 2) or delta0.device != a.device:
            raise ValueError(f"masic_amd.align_patches: delta0 must be [{B},4,2] on the patches' device, got {tuple(delta0.shape)}")
    iters = tuple(int(i) for i in iters)
    if len(iters) != 3:
        raise ValueError(f"masic_amd.align_patches: iters holds three step counts (coarse to fine), got {iters}")
    delta = torch.empty((B, 4, 2), dtype=torch.float32, device=a.device)
    info = torch.empty((B, 4), dtype=torch.float32, device=a.device)
    nbytes = _lib.lib.masic_align_workspace_bytes(B, P)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=a.device) if nbytes else None
    with torch.cuda.device(a.device):
        _lib.check(_lib.lib.masic_align_patches(_p(a), _p(b), _p(delta0), _p(delta), _p(info), _p(ws), B, P, int(search_radius), iters[0],
                                                iters[1], iters[2], float(damping), _stream()), "align_patches")
    return delta, info


class PatchAligner(nn.Module):
    """A drop-in for the UDH net without parameters or buffers: forward(a, b) -> delta [B,4,2], the state dict is empty.  With `init`
    (a module or any callable mapping the two patches to offsets, e.g. a trained net) its output is the start value and the aligner
    refines it.  `init` is called, not owned: it is kept out of the module tree, so the state dict stays empty and `.eval()`, `.to()`
    and `.train()` of the aligner do not reach it -- the caller puts it on the device and in eval mode.  `last_info` is the info
    tensor of the last call."""

    def __init__(self, init=None, search_radius=12, iters=ITERS, damping=1e-6):
        super().__init__()
        self.__dict__["init"] = init          # not a submodule (see the class docstring)
        self.search_radius, self.iters, self.damping = int(search_radius), tuple(iters), float(damping)
        self.last_info = None

    def forward(self, a, b):
        with torch.no_grad():
            delta0 = None if self.init is None else self.init(a, b).detach().reshape(-1, 4, 2).float().contiguous()
            delta, self.last_info = align_patches(a, b, delta0, search_radius=self.search_radius, iters=self.iters, damping=self.damping)
        return delta
