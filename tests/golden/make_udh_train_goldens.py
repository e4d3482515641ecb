"""Writes tests/golden/udh_train.npz: one training step of the REFERENCE's UDH homography net (udh/udh/model.py: Net +
photometric_loss, loss.backward()) on the CPU.  Needs the reference tree and oracle/_ref (`make -C oracle ref`); run from the
repository root:  python tests/golden/make_udh_train_goldens.py

kornia is not part of the reference tree: oracle/ref_import installs a stand-in with warp_perspective (oracle/hsic_oracle.py), and
this generator adds get_perspective_transform to it from tests/udh_train_ref.py -- PARITY UNPINNED for both, as oracle/udh_oracle.py
declares.  Everything else (the net, Dropout, the loss's own lines, autograd) is the reference's code.

Cases (patch, B, img H x W, mode): see CASES.  Weights: tests/udh_weights.py, WEIGHT_SEED.  Patches: UW.patches(seed, 1, p), ONE
SEED PER PAIR, the first at which the float64 net stays clear of its own kinks -- every ReLU argument and every max-pool decision
further than 4 float32 roundoffs of its terms' magnitudes from the switch (tests/udh_train_ref.py: kink_margin, asserted for the
batch with the recorded masks too).  Without this rule a float32 evaluation may take another ReLU branch than float64 does: stock
torch on an MI355X did at one of 73728 units of layer 7 in the (64, 9) case and moved that layer's bias gradient by 6e-3 of its
peak, where the bound is 1e-4.

The loss inputs come from tests/udh_train_ref.py: loss_pair, ONE SEED PER PAIR, chosen here as the first seed for which, in float64,
no sample coordinate lies within 1e-4 px of an integer and no |diff| is below 1e-5 (asserted; at such points the loss is not
differentiable, two correct float32 evaluations may take different one-sided derivatives, and parity is undefined).  The seed is
chosen per pair and not per case because the condition is one on every sample: a 9 x 64 x 64 case has 36864 of them and almost no
case seed passes, while each pair's 4096 samples pass for about one seed in five.  In at least one case >= 1 % of the samples
fall outside img_a (asserted).

Per case c<i>/: `patch_seeds` and `seeds` (the pair seeds of the patches and of the loss inputs), `loss`, `delta`, the gradients of
the 20 parameters g/<name> (tensors above 4096 entries as 512 sampled entries @idx/@val + @norm + @absmax, as cqe_train.npz), and the reference's own float32 floor
floor/<key>: its float32 result against `net.double()` on the same inputs and masks, error over the tensor's peak.  In train mode
`m1`, `m2` are the masks the reference drew (np.packbits of the keep-bits), recorded by forward hooks on its two Dropout modules as
`output != 0`; where a Dropout INPUT is zero the bit is immaterial -- the value is zero either way and the ReLU in front has zero
derivative there -- so a zero bit is stored."""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import ref_import  # noqa: E402
from tests import udh_train_ref as TR  # noqa: E402
from tests import udh_weights as UW  # noqa: E402
from tests.udh_train_cases import CASES, RHO  # noqa: E402  (the cases and the corner perturbation range in pixels)



def case_seed(index, p, B):
    return 5000 + 100 * index + UW.case_seed(p, B) % 97


def load_reference_model():
    ref_import.load()                                  # installs the kornia / torchvision stand-ins the file imports
    sys.modules["kornia"].get_perspective_transform = TR.get_perspective_transform
    path = os.path.join(ref_import.REF, "udh", "udh", "model.py")
    spec = importlib.util.spec_from_file_location("udh_model_reference", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def put(fx, key, g, rs):
    g = g.detach().numpy()
    if g.size <= 4096:
        fx[key] = g.copy()
        return
    idx = rs.randint(0, g.size, size=512)
    fx[key + "@idx"] = idx.astype(np.int64)
    fx[key + "@val"] = g.reshape(-1)[idx].copy()
    fx[key + "@norm"] = np.array(float(np.sqrt((g.astype(np.float64) ** 2).sum())))
    fx[key + "@absmax"] = np.array(float(np.abs(g).max()))


def floor(a32, a64):
    peak = float(a64.abs().max())
    return float((a32.double() - a64).abs().max()) / (peak if peak > 0 else 1.0)


def step(M, net, a, b, img, pb, corners, masks, record):
    """One forward + backward of the reference; Dropout outputs are recorded into `record`, or replayed from `masks`."""
    hooks = []
    drops = [net.fc[1], net.fc[4]]
    for i, d in enumerate(drops):
        if masks is None:
            hooks.append(d.register_forward_hook(lambda mod, inp, out, i=i: record.__setitem__(i, (out != 0).detach())))
        else:
            hooks.append(d.register_forward_hook(lambda mod, inp, out, i=i: inp[0] * (2.0 * masks[i].to(inp[0].dtype))))
    net.zero_grad()
    delta = net(a, b)
    loss = M.photometric_loss(delta, img, pb, corners)
    loss.backward()
    for h in hooks:
        h.remove()
    return loss.detach(), delta.detach(), {n: p.grad.detach().clone() for n, p in net.named_parameters()}


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    M = load_reference_model()
    rs = np.random.RandomState(11)
    fx = {}
    most_outside = 0.0
    for index, (p, B, img_hw, mode) in enumerate(CASES):
        seed = case_seed(index, p, B)
        net = M.Net(patch_size=p)
        UW.fill(net, UW.WEIGHT_SEED)
        net.train(mode == "train")
        # one patch seed per pair: the first at which the float64 net is clear of its own kinks (TR.kink_margin)
        ref64 = TR.Net(p)
        UW.fill(ref64, UW.WEIGHT_SEED)
        ref64.double()
        patch_seeds = []
        for n in range(B):
            for s in range(seed * 1000 + 100000 * n, seed * 1000 + 100000 * n + 20000):
                if TR.kink_margin(ref64, *UW.patches(s, 1, p)) >= TR.KINK_MARGIN:
                    patch_seeds.append(s)
                    break
            else:
                raise RuntimeError(f"no patch seed clear of the kinks for pair {n}")
        a, b = TR.patch_batch(patch_seeds, p)
        torch.manual_seed(seed)
        # the first forward fixes delta (and the masks); the pair seeds are then chosen against it
        record = {}
        with torch.no_grad():
            hooks = [d.register_forward_hook(lambda mod, inp, out, i=i: record.__setitem__(i, (out != 0).detach()))
                     for i, d in enumerate((net.fc[1], net.fc[4]))]
            delta0 = net(a, b)
            for h in hooks:
                h.remove()
        masks = (record[0], record[1]) if mode == "train" else None
        kink = TR.kink_margin(ref64, a, b, masks)
        assert kink >= TR.KINK_MARGIN, ("the drawn masks put a hidden unit at its kink: change the case seed", kink)
        seeds = TR.find_pair_seeds(delta0, img_hw, (p, p), RHO[p], first=seed * 1000)
        img, pb, corners = TR.loss_inputs(seeds, img_hw, (p, p), RHO[p])
        coord, diff, outside = TR.margins(delta0, img, pb, corners)
        assert coord > TR.MARGIN_COORD and diff >= TR.MARGIN_DIFF, (coord, diff)
        most_outside = max(most_outside, outside)
        replay = masks if masks is not None else None
        if replay is None:                              # eval: Dropout is the identity, nothing to replay
            l32, d32, g32 = step(M, net, a, b, img, pb, corners, None, {})
        else:
            l32, d32, g32 = step(M, net, a, b, img, pb, corners, replay, None)
        assert torch.equal(d32, delta0), "replaying the recorded masks must reproduce the reference's own forward"
        net.double()
        dm = None if replay is None else replay
        l64, d64, g64 = step(M, net, a.double(), b.double(), img.double(), pb.double(), corners.double(), dm, {} if dm is None else None)
        key = f"c{index}/"
        fx[key + "seeds"] = np.array(seeds, dtype=np.int64)
        fx[key + "patch_seeds"] = np.array(patch_seeds, dtype=np.int64)
        fx[key + "loss"] = l32.numpy().copy()
        fx[key + "delta"] = d32.numpy().copy()
        fx[key + "floor/loss"] = np.array(floor(l32, l64))
        fx[key + "floor/delta"] = np.array(floor(d32, d64))
        if masks is not None:
            fx[key + "m1"] = np.packbits(masks[0].numpy().astype(np.uint8), axis=1)
            fx[key + "m2"] = np.packbits(masks[1].numpy().astype(np.uint8), axis=1)
        worst = 0.0
        for n in g32:
            put(fx, key + "g/" + n, g32[n], rs)
            f = floor(g32[n], g64[n])
            fx[key + "floor/g/" + n] = np.array(f)
            worst = max(worst, f)
        print(f"case {index} p={p} B={B} img {img_hw} {mode}: seeds {seeds}, loss {float(l32):.6f}, peak |delta| {float(d32.abs().max()):.3f}, "
              f"margins coord {coord:.2e} px diff {diff:.2e} kink {kink:.1e}, outside {outside:.3f}, float32 floor: loss {floor(l32, l64):.1e} "
              f"delta {floor(d32, d64):.1e} worst gradient {worst:.1e}")
    assert most_outside >= 0.01, most_outside
    path = os.path.join(ROOT, "tests", "golden", "udh_train.npz")
    np.savez_compressed(path, **fx)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
