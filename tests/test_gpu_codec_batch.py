"""GPU tests (-m gpu) of the batched bitstream path HSIC.compress_batch / decompress_batch (masic_amd/codec.py encode_views /
decode_views; the batched kernels of masic_amd/csrc/skinny.hip and codec.hip).  The contract: the files of a batch are byte for byte
those of compress on each pair alone, and every slice of a batched decode equals decompress of that pair alone."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIELDS = ("x1_hat", "x2_hat", "y1_hat", "y2_hat", "z1_hat", "z2_hat")


def _net(N, M, K, seed, prec):
    import MASIC
    from masic_amd import nn as mnn, synth
    mnn.set_precision(prec)
    net = MASIC.HSIC(N, M, K)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=seed))
    net = net.to(DEV).eval()
    net.update()
    return net


def _files(path, name):
    return tuple(open(os.path.join(path, name + ext), "rb").read() for ext in (".npz", ".bin"))


def _count_calls(monkeypatch, mod, name):
    calls = []
    orig = getattr(mod, name)

    def wrapped(*a, **k):
        calls.append(1)
        return orig(*a, **k)
    monkeypatch.setattr(mod, name, wrapped)
    return calls


@pytest.mark.parametrize("N,M,K,H,W,B,prec", [(32, 48, 3, 128, 192, 3, "f32"), (32, 48, 3, 128, 192, 3, "bf16"),
                                              (128, 192, 5, 256, 320, 2, "bf16")])
def test_batch_files_equal_single_pair_files(tmp_path, monkeypatch, N, M, K, H, W, B, prec):
    from masic_amd import codec, nn as mnn, synth
    try:
        net = _net(N, M, K, 21, prec)
        x1, x2, hm = (t.to(DEV) for t in synth.synth_inputs(B, H, W, seed=21))
        one, many = tmp_path / "one", tmp_path / "many"
        one.mkdir()
        many.mkdir()
        names = [f"pair{i}" for i in range(B)]
        with torch.no_grad():
            singles = [net.compress(x1[i:i + 1], x2[i:i + 1], hm[i:i + 1], names[i], str(one)) for i in range(B)]
            calls = _count_calls(monkeypatch, codec, "encode_views")
            enc = net.compress_batch(x1, x2, hm, names, str(many))
        if prec == "bf16" and M == 192:
            assert len(calls) == 2                                      # both views through the batched coding loop
        for i, n in enumerate(names):
            assert _files(one, n) == _files(many, n), n
            assert enc["bytes"][i] == singles[i]["bytes"] and enc["bpp"][i] == singles[i]["bpp"]
        for k in FIELDS:
            assert enc[k].shape[0] == B
            assert torch.equal(enc[k], torch.cat([s[k] for s in singles])), k
    finally:
        mnn.set_precision("f32")


def test_batch_round_trip_and_cross_decoding(tmp_path, monkeypatch):
    from masic_amd import codec, nn as mnn, synth
    B, H, W = 3, 128, 192
    try:
        net = _net(128, 192, 5, 27, "bf16")
        x1, x2, hm = (t.to(DEV) for t in synth.synth_inputs(B, H, W, seed=27))
        names = ["a", "b", "c"]
        with torch.no_grad():
            enc = net.compress_batch(x1, x2, hm, names, str(tmp_path))
            calls = _count_calls(monkeypatch, codec, "decode_views")
            dec = net.decompress_batch(names, hm, str(tmp_path))
            assert len(calls) == 2
            for k in FIELDS:
                assert torch.equal(enc[k], dec[k]), k                  # lossless latents, identical reconstructions
            # one pair of the batch through the single-pair decoder
            d1 = net.decompress(None, None, hm[1:2], "b", str(tmp_path))
            for k in FIELDS:
                assert torch.equal(d1[k], dec[k][1:2]), k
            # files of single compress calls through the batched decoder
            for i, n in enumerate(("s0", "s1")):
                net.compress(x1[i:i + 1], x2[i:i + 1], hm[i:i + 1], n, str(tmp_path))
            ds = net.decompress_batch(["s0", "s1"], hm[:2], str(tmp_path))
            for k in FIELDS:
                assert torch.equal(ds[k], enc[k][:2]), k
            # another order of the names: the results permute with it
            perm = [2, 0, 1]
            dp = net.decompress_batch([names[i] for i in perm], hm[perm], str(tmp_path))
            for k in FIELDS:
                assert torch.equal(dp[k], enc[k][perm]), k
    finally:
        mnn.set_precision("f32")


def test_batched_pixel_list_kernels_equal_the_single_image_kernels():
    """skinny.hip over a batch (list entries b * h * w + p): every image's sigma / mu / logits are BIT-identical to the one-image
    kernels on that image, whatever the order of the list and however it is split across launches -- for the left view's layers
    and the right view's (whose context model is gated per image)."""
    from masic_amd import nn as mnn, synth
    from MASIC import _warp_matrices
    try:
        net = _net(128, 192, 5, 31, "bf16")
        B, M, h, w = 3, 192, 8, 12
        H, W = 16 * h, 16 * w
        HW = h * w
        g = torch.Generator().manual_seed(31)
        y_hat = torch.randint(-6, 7, (B, M, h, w), generator=g).float().to(DEV)
        z_hat = torch.randn((B, 128, h // 4, w // 4), generator=g).to(DEV)
        x1_hat = torch.rand((B, 3, H, W), generator=g).to(DEV)
        _, _, hm = synth.synth_inputs(B, H, W, seed=31)
        hm = hm.to(DEV)
        rs = np.random.RandomState(31)
        with torch.no_grad():
            for view in ("left", "right"):
                def build(i):
                    if view == "left":
                        return net._left_params_fn(z_hat[i:i + 1], h, w)
                    m_fwd, m_back = _warp_matrices(hm[i:i + 1], (H, W), (H, W), want_inverse=True)
                    return net._right_params_fn(z_hat[i:i + 1], x1_hat[i:i + 1], m_fwd, m_back, H, W, h, w)[0]
                head, ctx, C = ((net._h_s1_same_resolution, net.context_prediction1, 4 * M) if view == "left"
                                else (net._h_s2_same_resolution, net.context_prediction2, 5 * M))
                want = []
                for i in range(B):
                    src = net._batch_params([build(i)], head, ctx, C, h, w)
                    assert src is not None and src.skinny
                    src.set_latent(y_hat[i:i + 1])
                    src.run(torch.arange(HW, dtype=torch.int32, device=DEV), None, 0, HW)
                    want.append([t.clone() for t in (src.sigma, src.mu, src.logits)])
                bp = net._batch_params([build(i) for i in range(B)], head, ctx, C, h, w)
                assert bp is not None and bp.skinny
                bp.set_latent(y_hat)
                for trial in range(2):
                    for t in (bp.sigma, bp.mu, bp.logits):
                        t.fill_(float("nan"))
                    q = rs.permutation(B * HW).astype(np.int32)
                    cuts = sorted(rs.choice(np.arange(1, B * HW), size=2, replace=False)) if trial else [B * HW // 2]
                    for part in np.split(q, cuts):
                        bp.run(torch.from_numpy(part).to(DEV), None, 0, part.size)
                    for i in range(B):
                        for a, b, name in zip((bp.sigma, bp.mu, bp.logits), want[i], ("sigma", "mu", "logits")):
                            assert torch.equal(a[i:i + 1], b), (view, trial, i, name)
                # padding entries and a list with one pixel of the last image only
                for t in (bp.sigma, bp.mu, bp.logits):
                    t.fill_(float("nan"))
                p = (B - 1) * HW + 5 * w + 7
                bp.run(torch.tensor([-1, p, -1], dtype=torch.int32, device=DEV), None, 0, 3)
                for a, b in zip((bp.sigma, bp.mu, bp.logits), want[B - 1]):
                    assert torch.equal(a[B - 1].reshape(a.shape[1], HW)[:, 5 * w + 7], b[0].reshape(b.shape[1], HW)[:, 5 * w + 7])
                    assert int(torch.isnan(a).sum()) == a.numel() - a.shape[1]
    finally:
        mnn.set_precision("f32")


@pytest.mark.parametrize("use_graph", [True, False])
def test_batched_tables_and_decode_steps_equal_the_single_pair_coder(use_graph):
    """masic_gmm_cdf_rows_batch + masic_rans_decode_step_batch on synthetic entropy parameters: three pairs with different channel sets
    and alphabets -- one with 41 entries (register form of the decode kernel), one with 81 (general form) in the same launch, one with
    no coded channel.  The encoder's streams equal those of each pair alone, coded as B = 1 with the full-latent parameter form as the
    single-pair methods do (same (start, freq) of every symbol), and the device decoder gets every symbol back."""
    from masic_amd import codec
    B, M, K, h, w = 3, 24, 3, 12, 10
    HW = h * w
    rs = np.random.RandomState(7)
    minmaxes = [20, 40, 5]
    chans = [sorted(rs.choice(M, 5, replace=False).tolist()), sorted(rs.choice(M, 3, replace=False).tolist()), []]
    sigma = torch.from_numpy(rs.uniform(0.05, 6.0, (B, K * M, h, w)).astype(np.float32)).to(DEV)
    mu = torch.from_numpy(rs.uniform(-8.0, 8.0, (B, K * M, h, w)).astype(np.float32)).to(DEV)
    logits = torch.from_numpy((rs.standard_normal((B, K * M, h, w)) * 2).astype(np.float32)).to(DEV)
    y = np.zeros((B, M, h, w), dtype=np.float32)
    for b in range(B):
        for m in chans[b]:
            y[b, m] = rs.randint(-minmaxes[b], minmaxes[b] + 1, (h, w))
    y_hat = torch.from_numpy(y).to(DEV)

    class Fixed:
        """the entropy parameters as given: no layers to run"""
        skinny = True

        def __init__(self):
            self.sigma, self.mu, self.logits = sigma, mu, logits
            self.y16 = torch.zeros(B * 32 * HW, dtype=torch.int16, device=DEV)

        def set_latent(self, y):
            pass

        def run(self, *a):
            pass

    blobs = codec.encode_views(Fixed(), y_hat, M, K, chans, minmaxes, 0.11)
    for b in range(B):
        single, = codec.encode_views(lambda _y, b=b: (sigma[b:b + 1], mu[b:b + 1], logits[b:b + 1]), y_hat[b:b + 1], M, K,
                                     [chans[b]], [minmaxes[b]], 0.11)
        assert blobs[b] == single, b
    assert len(codec.split_channels(blobs[2])[0]) == 0
    got = codec.decode_views(Fixed(), blobs, (h, w), M, K, chans, minmaxes, 0.11, DEV, use_graph=use_graph)
    assert torch.equal(got, y_hat)
    # each pair alone through the single-pair device decoder agrees
    for b in range(2):
        one = codec.decode_views(lambda _y, b=b: (sigma[b:b + 1], mu[b:b + 1], logits[b:b + 1]), [blobs[b]], (h, w), M, K,
                                 [chans[b]], [minmaxes[b]], 0.11, DEV, use_graph=False)
        assert torch.equal(one, y_hat[b:b + 1])


def test_batch_errors(tmp_path):
    from masic_amd import nn as mnn, synth
    try:
        net = _net(32, 48, 3, 5, "bf16")
        x1, x2, hm = (t.to(DEV) for t in synth.synth_inputs(2, 128, 192, seed=5))
        a1, a2, ah = (t.to(DEV) for t in synth.synth_inputs(1, 128, 256, seed=6))
        with torch.no_grad():
            net.compress_batch(x1, x2, hm, ["p0", "p1"], str(tmp_path))
            net.compress(a1, a2, ah, "wide", str(tmp_path))
            with pytest.raises(ValueError, match="picture size"):
                net.decompress_batch(["p0", "wide"], torch.cat([hm[:1], ah]), str(tmp_path))
            with pytest.raises(ValueError):
                net.compress_batch(x1[:, :, :100], x2[:, :, :100], hm, ["q0", "q1"], str(tmp_path))    # not a multiple of 64
            with pytest.raises(ValueError):
                net.compress_batch(x1, x2, hm, ["q0"], str(tmp_path))                                # one name per pair
            mnn.set_precision("f32")
            with pytest.raises(ValueError, match="operand mode"):
                net.decompress_batch(["p0", "p1"], hm, str(tmp_path))
            mnn.set_precision("bf16")
            # pair 1's .bin cut inside its last channel stream: the bounded word reads report it, naming the pair
            path = os.path.join(tmp_path, "p1.bin")
            raw = open(path, "rb").read()
            open(path, "wb").write(raw[:-4])
            with pytest.raises((RuntimeError, ValueError), match=r"pair 1 \(p1\)"):
                net.decompress_batch(["p0", "p1"], hm, str(tmp_path))
            dec = net.decompress_batch(["p0"], hm[:1], str(tmp_path))            # the device is fine afterwards
            assert dec["x1_hat"].shape[0] == 1
            net.train()
            with pytest.raises(RuntimeError):
                net.compress_batch(x1, x2, hm, ["q0", "q1"], str(tmp_path))
            with pytest.raises(RuntimeError):
                net.decompress_batch(["p0"], hm[:1], str(tmp_path))
    finally:
        mnn.set_precision("f32")


def test_fp8_mode_batch_files_equal_single_files_and_decode_into_a_fresh_model(tmp_path):
    """The fp8 operand mode is accepted: its pairs are coded one after the other (no pixel-list form), the files equal compress's,
    and they decode into a fresh, uncalibrated model through the scale table in the stream.  Pairs whose tables differ are refused."""
    import MASIC
    from masic_amd import fp8, nn as mnn, synth
    N, M, K, H, W, B = 128, 192, 5, 128, 192, 2
    try:
        net = _net(N, M, K, 23, "fp8")
        x1, x2, hm = (t.to(DEV) for t in synth.synth_inputs(B, H, W, seed=23))
        fp8.calibrate(net, [(x1[:1], x2[:1], hm[:1])])
        one, many = tmp_path / "one", tmp_path / "many"
        one.mkdir()
        many.mkdir()
        with torch.no_grad():
            singles = [net.compress(x1[i:i + 1], x2[i:i + 1], hm[i:i + 1], f"q{i}", str(one)) for i in range(B)]
            enc = net.compress_batch(x1, x2, hm, ["q0", "q1"], str(many))
        for i in range(B):
            assert _files(one, f"q{i}") == _files(many, f"q{i}")
        for k in FIELDS:
            assert torch.equal(enc[k], torch.cat([s[k] for s in singles])), k
        sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items() if not k.endswith(("._offset", "._quantized_cdf", "._cdf_length"))}
        other = MASIC.HSIC(N, M, K)
        other.load_state_dict(sd, strict=False)
        other = other.to(DEV).eval()
        other.update()
        with torch.no_grad():
            dec = other.decompress_batch(["q0", "q1"], hm, str(many))
        for k in FIELDS:
            assert torch.equal(enc[k], dec[k]), k
        assert not fp8.export_scales(other)
        # a pair written under another calibration cannot share the batch
        fp8.calibrate(net, [(x1[1:], x2[1:], hm[1:])], margin=3.0)
        with torch.no_grad():
            net.compress(x1[1:], x2[1:], hm[1:], "r1", str(many))
            with pytest.raises(ValueError, match="scales"):
                other.decompress_batch(["q0", "r1"], hm, str(many))
    finally:
        mnn.set_precision("f32")
