"""GPU tests (-m gpu) of the banded y bitstream: HSIC.compress(..., band_rows=S) cuts the latent into bands of S rows whose context model
does not look across the band's top edge, so that the bands' coding wavefronts run side by side (masic_amd/codec.py wavefront_steps; the
banded context kernel skinny_f16k_bands of masic_amd/csrc/skinny.hip behind include/masic_bands.h).

1. the banded kernel against the float64 reference of tests/gemm_ref.py applied to each band as an image of its own;
2. on the real HSIC(128,192,5) modules: the banded launch equals the unbanded launch on each band cut out, bit for bit, however the
   pixels are launched;
3. round trips (float32, bf16, the wide model), the "MSR3" header, one band = today's bytes;  4. the number of decode steps;
5. batches;  6. a file decoded with another band_rows than it was written with is refused;  7. the fp8 mode;  8. stereo files."""
import os
import shutil

import numpy as np
import pytest
import torch

from tests import bands_ref as BR
from tests import f16k_ref as R
from tests import gemm_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIELDS = ("x1_hat", "x2_hat", "y1_hat", "y2_hat", "z1_hat", "z2_hat")
_NETS = {}


def _net(N, M, K, seed, prec):
    """cached per (shape, seed, operand mode): the models are in eval mode and no test here changes one"""
    from masic_amd import nn as mnn
    key = (N, M, K, seed, prec)
    if key not in _NETS:
        _NETS[key] = BR.hsic(N, M, K, seed, prec)
    mnn.set_precision(prec)
    return _NETS[key]


def _read(path, name, ext):
    with open(os.path.join(str(path), name + ext), "rb") as f:
        return f.read()


# ------------------------------------------------------------------------------------------ 1. the kernel against float64
@pytest.mark.parametrize("S", [1, 3, 8])
def test_banded_context_kernel_vs_float64(S):
    """sc-ragged's operands (B = 3, 80 -> 160 channels into a channel view, leaky, gated) on an 8 x 12 latent: bands of 1 row, of 3, 3
    and 2 rows, and one band.  (a) whole numbers under gemm_ref.exact_bound < 2^24: every partial sum is exact in float32, so the
    F16K output must be the float64 reference rounded once to bf16, bit for bit; (b) real operands at gemm_ref.gate_for.  With the
    four lists of gemm_ref.pixel_lists; unlisted pixels and the channels outside the view keep their prefill."""
    from masic_amd import ops
    from tests import test_gpu_gemm_rows as T
    case = G.by_id("sc-ragged")._replace(H=8, W=12)
    assert case.ctx and case.B == 3 and case.gate is not None
    l, = case.layers
    assert (l.Cin, l.Cout, l.out) == (80, 160, "f16k")
    B, H, W, HW = case.B, case.H, case.W, case.H * case.W
    assert [b - a for a, b in BR.bands(H, 3)] == [3, 3, 2]
    ctot, coff = l.view
    for exact in (True, False):
        (x, w, bias, _, _), = T._references(case, integers=exact)
        if exact:
            assert G.exact_bound(case, l, x, w, bias) < 2 ** 24, "every partial sum must be a float32 integer"
        v64 = BR.banded_layer64(case, l, x, w, bias, S)
        if S < H:
            assert not torch.equal(v64, G.layer64(case, l, x, w, bias)), "the band top must matter to the reference"
        gate = G.gate_plane(case, 0 if exact else 500)
        full = G.whole_buffer(l, G.expected(l, v64, gate[:, case.gate[1]:case.gate[1] + 1]), G.prefill_of(l, listed=True))
        wp, _ = T._pack(case, l, w)
        xb = T._x_buffer(case, x)
        every = None
        for plist in G.pixel_lists(case):
            out = T._out_buffer(l, B, H, W, listed=True)
            layer = dict(x=xb, wp=wp, bias=bias.to(DEV), Cin=l.Cin, Cout=l.Cout, act=l.act, out_ctot=ctot, out_coff=coff, y16=out)
            step = None if plist.step is None else torch.tensor([plist.step], dtype=torch.int32, device=DEV)
            ops.skinny_group([layer], plist.pix.to(DEV), step, plist.list_stride, plist.npix, H, W, ctx=True, gate=gate.to(DEV),
                             gate_c=case.gate[1], nimg=B, band_rows=S)
            torch.cuda.synchronize()
            y = T._decode(l, out, B, H, W, None)
            name = f"band_rows {S}, list '{plist.name}', {'whole numbers' if exact else 'real operands'}"
            want = G.scatter_ref(full, plist.named, B, HW, G.prefill_of(l, listed=True))
            named = ~torch.isnan(G.scatter_ref(torch.zeros(B, 1, H, W), plist.named, B, HW, float("nan")))[:, 0]
            written = torch.zeros((B, ctot, H, W), dtype=torch.bool)
            written[:, coff:coff + l.Cout] = named[:, None]
            assert torch.equal(R.bits(y)[~written], R.bits(want)[~written]), f"{name}: unlisted pixels and the channels outside the view keep the prefill"
            if exact:
                assert T._same(l, y, want), f"{name}: exact operands, exact sums"
            else:
                e = float((y[written].double() - want[written].double()).abs().max()) / float(full[:, coff:coff + l.Cout].double().abs().max())
                print(f"bands | {name} | gate {G.gate_for(l):.1e} | error {e:.3e}")
                assert e <= G.gate_for(l), f"{name}: {e:.3e} > {G.gate_for(l):.1e}"
            if every is not None:
                assert torch.equal(R.bits(y)[written], R.bits(every)[written]), f"{name}: differs from the all-pixels launch at its pixels"
            if plist.name == "all":
                every = y


def test_band_rows_is_refused_outside_the_context_model():
    from masic_amd import ops
    pix = torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="band_rows"):
        ops.skinny_group([{}], pix, None, 0, 1, 4, 4, ctx=False, band_rows=2)
    with pytest.raises(ValueError, match="band_rows"):
        ops.skinny_group([{}], pix, None, 0, 1, 4, 4, ctx=True, band_rows=-1)


# ------------------------------------------------------------------------------------------ 2. banded = unbanded on each band
@pytest.mark.parametrize("S", [1, 5, 16])
def test_banded_launch_equals_the_unbanded_launch_on_each_band_and_does_not_depend_on_the_list(S):
    """HSIC(128,192,5)'s left-view layers over B = 2 latents of 16 x 24: sigma / mu / logits of the banded launch over all pixels are,
    bit for bit, (i) those of the unbanded kernels on every band cut out as a batch of images of its own, (ii) those of the banded
    launches coding step by coding step through the device step counter, into poisoned buffers, (iii) those of single pixels alone (one
    on a band's top row, one below it); and with one band (S = 16) those of the unbanded launch."""
    import MASIC
    from masic_amd import codec, nn as mnn
    from masic_amd.f16k import F16K
    try:
        net = _net(128, 192, 5, 31, "bf16")
        M, K, h, w, B = 192, 5, 16, 24, 2
        HW = h * w
        head, ctx = net._h_s1_same_resolution, net.context_prediction1
        g = torch.Generator().manual_seed(31 + S)
        y_hat = torch.randint(-6, 7, (B, M, h, w), generator=g).float().to(DEV)
        z_hat = torch.randn((B, 128, h // 4, w // 4), generator=g).to(DEV)
        outs = lambda s: (s.sigma, s.mu, s.logits)
        with torch.no_grad():
            parts = [net._left_params_fn(z_hat[i:i + 1], h, w) for i in range(B)]
            cat = torch.cat([p.cat16.to_nchw() for p in parts])                      # the hyper half is filled; the context half is the launches' to write
            src = net._batch_params(parts, head, ctx, 4 * M, h, w)
            assert src is not None and src.skinny
            src.set_latent(y_hat)
            allpix = torch.arange(B * HW, dtype=torch.int32, device=DEV)
            src.run(allpix, None, 0, B * HW, band_rows=S)
            ref = [t.clone() for t in outs(src)]
            assert all(bool(torch.isfinite(t).all()) for t in ref)
            # (i) every band as images of its own through the unbanded kernels
            for r0, r1 in BR.bands(h, S):
                hb = r1 - r0
                sk = net._skinny_params(head, ctx, F16K.from_nchw(cat[:, :, r0:r1].contiguous()), None)
                band = MASIC.HSIC._PixelParams(sk)
                band.set_latent(y_hat[:, :, r0:r1].contiguous())
                band.run(torch.arange(B * hb * w, dtype=torch.int32, device=DEV), None, 0, B * hb * w)
                for a, b, name in zip(outs(band), ref, ("sigma", "mu", "logits")):
                    assert torch.equal(a, b[:, :, r0:r1]), (name, r0, r1)
            if S >= h:
                src.run(allpix, None, 0, B * HW)
                for a, b, name in zip(outs(src), ref, ("sigma", "mu", "logits")):
                    assert torch.equal(a, b), f"one band: {name} differs from the unbanded kernel's"
            else:
                src.run(allpix, None, 0, B * HW)
                assert not torch.equal(src.mu, ref[1]), "the band top must matter"
            # (ii) the decoder's form
            steps = codec.wavefront_steps(h, w, S)
            assert len(steps) == w + 3 * (S - 1)
            _, packed = codec._batch_step_lists(h, w, B, torch.device(DEV), S)
            step_d = torch.zeros(1, dtype=torch.int32, device=DEV)
            for t in outs(src):
                t.fill_(float("nan"))
            for _ in range(len(steps)):
                src.run(packed, step_d, B * h, B * h, band_rows=S)
                step_d += 1
            for a, b, name in zip(outs(src), ref, ("sigma", "mu", "logits")):
                assert torch.equal(a, b), f"step by step: {name}"
            # (iii) single pixels of image 1: the top row of the band that holds row 7, and row 7
            for row in sorted({(7 // S) * S if S < h else 0, 7}):
                p = row * w + 9
                for t in outs(src):
                    t.fill_(float("nan"))
                src.run(torch.tensor([HW + p], dtype=torch.int32, device=DEV), None, 0, 1, band_rows=S)
                for a, b in zip(outs(src), ref):
                    assert torch.equal(a.view(B, K * M, HW)[1, :, p], b.view(B, K * M, HW)[1, :, p]), row
                    assert int(torch.isnan(a).sum()) == K * M * (B * HW - 1)
    finally:
        mnn.set_precision("f32")


# ------------------------------------------------------------------------------------------ 3. round trips
@pytest.mark.parametrize("N,M,K,H,W,prec,bands,one_band", [(32, 48, 3, 128, 192, "f32", (1, 3, 4), (8, 100)),
                                                           (32, 48, 3, 128, 192, "bf16", (1, 3, 4), (8, 100)),
                                                           (128, 192, 5, 256, 320, "bf16", (4,), ())])
def test_round_trip(tmp_path, N, M, K, H, W, prec, bands, one_band):
    from masic_amd import nn as mnn, synth
    try:
        net = _net(N, M, K, 21, prec)
        x1, x2, hm = (t.to(DEV) for t in synth.synth_inputs(1, H, W, seed=21))
        pid = {"f32": 0, "bf16": 1}[prec]
        with torch.no_grad():
            fwd = net(x1, x2, hm)
            plain = net.compress(x1, x2, hm, "plain", str(tmp_path))
            assert _read(tmp_path, "plain", ".bin")[:8] == b"MSR2" + bytes([pid, 0, 0, 0])
            for S in bands:
                name = f"bands{S}"
                enc = net.compress(x1, x2, hm, name, str(tmp_path), band_rows=S)
                dec = net.decompress(None, None, hm, name, str(tmp_path))
                for k in FIELDS:
                    assert torch.equal(enc[k], dec[k]), (S, k)                     # lossless latents, identical reconstructions
                    assert torch.equal(enc[k], plain[k]), (S, k)                   # the latents do not depend on band_rows
                assert torch.equal(enc["y1_hat"], fwd["y1_hat"])
                raw = _read(tmp_path, name, ".bin")
                assert raw[:8] == b"MSR3" + bytes([pid, 0, S, 0])
                assert _read(tmp_path, name, ".npz") == _read(tmp_path, "plain", ".npz")
                assert raw[8:] != _read(tmp_path, "plain", ".bin")[8:], "other tables at the band tops: other bytes"
                print(f"bands | HSIC({N},{M},{K}) {H}x{W} {prec} | band_rows {S}: {enc['bytes']} bytes, band_rows 0: {plain['bytes']} (synthetic weights)")
            for S in one_band:                                                     # one band covers the latent: today's streams
                name = f"one{S}"
                enc = net.compress(x1, x2, hm, name, str(tmp_path), band_rows=S)
                raw = _read(tmp_path, name, ".bin")
                assert raw[:8] == b"MSR3" + bytes([pid, 0, S, 0])
                assert raw[8:] == _read(tmp_path, "plain", ".bin")[8:]
                dec = net.decompress(None, None, hm, name, str(tmp_path))
                for k in FIELDS:
                    assert torch.equal(enc[k], dec[k]), (S, k)
    finally:
        mnn.set_precision("f32")


# ------------------------------------------------------------------------------------------ 4. step count
def test_a_view_is_decoded_in_w_plus_3_band_rows_minus_1_steps(tmp_path, monkeypatch):
    import functools
    from masic_amd import codec, nn as mnn, synth
    try:
        net = _net(128, 192, 5, 21, "bf16")
        H, W, S = 128, 192, 3
        h, w = H // 16, W // 16
        x1, x2, hm = (t.to(DEV) for t in synth.synth_inputs(1, H, W, seed=24))
        with torch.no_grad():
            net.compress(x1, x2, hm, "pair", str(tmp_path), band_rows=S)
            graph = net.decompress(None, None, hm, "pair", str(tmp_path))
            per_view, steps = [], []
            decode_views, step_entry = codec.decode_views, codec.lib.masic_rans_decode_step_batch

            def counted_step(*a):
                steps.append(1)
                return step_entry(*a)

            def counted_views(*a, **k):
                before = len(steps)
                out = decode_views(*a, **dict(k, use_graph=False))
                per_view.append(len(steps) - before)
                return out
            monkeypatch.setattr(codec.lib, "masic_rans_decode_step_batch", counted_step)
            monkeypatch.setattr(codec, "decode_views", counted_views)
            loop = net.decompress(None, None, hm, "pair", str(tmp_path))
        assert per_view == [w + 3 * (S - 1)] * 2 and w + 3 * (S - 1) < w + 3 * (h - 1)
        for k in FIELDS:
            assert torch.equal(loop[k], graph[k]), k
    finally:
        mnn.set_precision("f32")


# ------------------------------------------------------------------------------------------ 5. batch
def test_batch_files_equal_single_files_and_one_band_rows_per_batch(tmp_path):
    from masic_amd import nn as mnn, synth
    B, H, W, S = 3, 128, 192, 3
    try:
        net = _net(128, 192, 5, 21, "bf16")
        x1, x2, hm = (t.to(DEV) for t in synth.synth_inputs(B, H, W, seed=27))
        one, many = tmp_path / "one", tmp_path / "many"
        one.mkdir()
        many.mkdir()
        names = ["a", "b", "c"]
        with torch.no_grad():
            singles = [net.compress(x1[i:i + 1], x2[i:i + 1], hm[i:i + 1], n, str(one), band_rows=S) for i, n in enumerate(names)]
            enc = net.compress_batch(x1, x2, hm, names, str(many), band_rows=S)
            for i, n in enumerate(names):
                assert _read(one, n, ".npz") == _read(many, n, ".npz") and _read(one, n, ".bin") == _read(many, n, ".bin"), n
                assert _read(many, n, ".bin")[:8] == b"MSR3" + bytes([1, 0, S, 0])
                assert enc["bytes"][i] == singles[i]["bytes"]
            dec = net.decompress_batch(names, hm, str(many))
            for k in FIELDS:
                assert torch.equal(dec[k], enc[k]), k
            for i, n in enumerate(names):
                d1 = net.decompress(None, None, hm[i:i + 1], n, str(many))
                for k in FIELDS:
                    assert torch.equal(d1[k], dec[k][i:i + 1]) and torch.equal(d1[k], singles[i][k]), (n, k)
            net.compress(x1[1:2], x2[1:2], hm[1:2], "other", str(many), band_rows=2)
            net.compress(x1[1:2], x2[1:2], hm[1:2], "none", str(many))
            for second in ("other", "none"):
                with pytest.raises(ValueError, match=rf"pair 1 \({second}\) was coded with band_rows"):
                    net.decompress_batch(["a", second], hm[:2], str(many))
    finally:
        mnn.set_precision("f32")


# ------------------------------------------------------------------------------------------ 6. the wrong schedule
def test_a_file_decoded_with_another_band_rows_is_refused(tmp_path):
    """byte 6 of a band_rows = 4 file patched to 2: the decoder walks another schedule with other band tops, so its tables are not the
    encoder's and the streams do not end where and how they must (codec.py: the final-state check).  The refusal is an exception of
    the decoder's own; the device goes on working."""
    from masic_amd import codec, nn as mnn, synth
    try:
        net = _net(128, 192, 5, 21, "bf16")
        H, W = 128, 192
        x1, x2, hm = (t.to(DEV) for t in synth.synth_inputs(1, H, W, seed=33))
        with torch.no_grad():
            enc = net.compress(x1, x2, hm, "pair", str(tmp_path), band_rows=4)
            raw = bytearray(_read(tmp_path, "pair", ".bin"))
            assert raw[:4] == b"MSR3" and raw[6] == 4
            raw[6] = 2
            shutil.copy(os.path.join(str(tmp_path), "pair.npz"), os.path.join(str(tmp_path), "patched.npz"))
            with open(os.path.join(str(tmp_path), "patched.bin"), "wb") as f:
                f.write(bytes(raw))
            with pytest.raises(codec.PairStreamError):
                net.decompress(None, None, hm, "patched", str(tmp_path))
            torch.cuda.synchronize()
            dec = net.decompress(None, None, hm, "pair", str(tmp_path))
        for k in FIELDS:
            assert torch.equal(enc[k], dec[k]), k
    finally:
        mnn.set_precision("f32")


# ------------------------------------------------------------------------------------------ 7. fp8
def test_fp8_mode_round_trip_into_a_fresh_model(tmp_path):
    """the shape and calibration of tests/test_gpu_codec.py::test_fp8_mode_compress_decompress_into_a_fresh_model with band_rows = 2:
    the full-latent parameter form, whose context model runs on the bands as images"""
    import MASIC
    from masic_amd import fp8, nn as mnn, synth
    N, M, K, H, W = 128, 192, 5, 128, 192
    try:
        net = BR.hsic(N, M, K, 23, "fp8")
        x1, x2, hm = (t.to(DEV) for t in synth.synth_inputs(1, H, W, seed=23))
        fp8.calibrate(net, [(x1, x2, hm)])
        with torch.no_grad():
            fwd = net(x1, x2, hm)
            enc = net.compress(x1, x2, hm, "pair8", str(tmp_path), band_rows=2)
            dec = net.decompress(None, None, hm, "pair8", str(tmp_path))
        for k in FIELDS:
            assert torch.equal(enc[k], dec[k]), k
        assert torch.equal(fwd["y1_hat"], enc["y1_hat"])
        raw = _read(tmp_path, "pair8", ".bin")
        assert raw[:4] == b"MSR3" and raw[4] == 2 and raw[5] & 1 and raw[6] == 2
        sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items() if not k.endswith(("._offset", "._quantized_cdf", "._cdf_length"))}
        other = MASIC.HSIC(N, M, K)
        other.load_state_dict(sd, strict=False)
        other = other.to(DEV).eval()
        other.update()
        with torch.no_grad():
            dec2 = other.decompress(None, None, hm, "pair8", str(tmp_path))
        for k in FIELDS:
            assert torch.equal(enc[k], dec2[k]), ("fresh decoder", k)
        assert not fp8.export_scales(other)
    finally:
        mnn.set_precision("f32")


# ------------------------------------------------------------------------------------------ 8. stereo files
def test_stereo_files_carry_band_rows_and_decode_without_the_argument(tmp_path):
    from masic_amd import StereoCodec, nn as mnn, stereofile as SF, synth
    from masic_amd.align import PatchAligner

    def pictures(B, H, W, seed):
        x1, x2, _ = synth.synth_inputs(B, H, W, seed=seed)
        u8 = lambda x: torch.from_numpy(np.ascontiguousarray(np.rint(x.numpy() * 255).astype(np.uint8).transpose(0, 2, 3, 1))).to(DEV)
        return u8(x1), u8(x2)

    def msf(path, name):
        return _read(path, name, ".msf")
    try:
        hsic = _net(32, 48, 3, 21, "bf16")
        sc = StereoCodec(hsic, PatchAligner().eval(), band_rows=2)
        many, one = tmp_path / "many", tmp_path / "one"
        many.mkdir()
        one.mkdir()
        left, right = pictures(2, 100, 150, seed=41)                     # padded to 128 x 192
        names = ["a", "b"]
        enc = sc.encode(left, right, names, str(many))
        whole = pictures(1, 128, 192, seed=43)                           # no padding
        enc_w = sc.encode(whole[0], whole[1], ["w"], str(many))
        for i, n in enumerate(names):
            sc.encode(left[i], right[i], n, str(one))
            assert msf(many, n) == msf(one, n), n
        for n in names + ["w"]:
            streams = SF.parse(msf(many, n), "test").streams
            assert streams[:4] == b"MSR3" and streams[6] == 2, n
        plain = StereoCodec(hsic)                                        # decode needs neither the aligner nor band_rows
        assert plain.band_rows == 0
        dec = plain.decode(names, str(many))
        assert torch.equal(dec["left"], enc["left_hat"]) and torch.equal(dec["right"], enc["right_hat"])
        assert torch.equal(dec["x1_hat"], enc["x1_hat"]) and torch.equal(dec["x2_hat"], enc["x2_hat"])
        dec_w = plain.decode("w", str(many))
        assert torch.equal(dec_w["left"], enc_w["left_hat"]) and torch.equal(dec_w["right"], enc_w["right_hat"])
        assert dec_w["left"].shape == (1, 128, 192, 3) and dec["left"].shape == (2, 100, 150, 3)
    finally:
        mnn.set_precision("f32")
