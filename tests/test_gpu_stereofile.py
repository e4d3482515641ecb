"""GPU tests (-m gpu) of the self-contained stereo files: the two batched kernels at the ends of the pipeline (ops.pairs_prep,
ops.planes_to_u8; masic_amd/csrc/data.hip) and masic_amd.StereoCodec, which decodes a .msf file with nothing but the file and the
weights.  Every comparison is bitwise."""
import os

import numpy as np
import pytest
import torch

from tests import udh_weights as UW

pytestmark = pytest.mark.gpu
DEV = "cuda"
H0, W0 = 100, 150                 # padded to 128 x 192
_CACHE = {}


def _ops():
    from masic_amd import ops
    return ops


def _hsic(N, M, K, seed, prec):
    import MASIC
    from masic_amd import nn as mnn, synth
    mnn.set_precision(prec)
    net = MASIC.HSIC(N, M, K)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=seed))
    net = net.to(DEV).eval()
    net.update()
    return net


def _fresh_copy(net, N, M, K):
    """A second model that shares nothing with `net` but the weights of its state_dict()."""
    import MASIC
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items() if not k.endswith(("._offset", "._quantized_cdf", "._cdf_length"))}
    other = MASIC.HSIC(N, M, K)
    other.load_state_dict(sd, strict=False)
    other = other.to(DEV).eval()
    other.update()
    return other


def _udh():
    if "udh" not in _CACHE:
        import model
        net = model.Net(patch_size=128).to(DEV).eval()
        UW.fill(net, UW.WEIGHT_SEED)
        _CACHE["udh"] = net
    return _CACHE["udh"]


def _pictures(B, H, W, seed):
    """B stereo pairs of smooth 8-bit pictures, uint8 [B,H,W,3] x 2 on the device."""
    from masic_amd import synth
    x1, x2, _ = synth.synth_inputs(B, H, W, seed=seed)
    u8 = lambda x: torch.from_numpy(np.ascontiguousarray(np.rint(x.numpy() * 255).astype(np.uint8).transpose(0, 2, 3, 1))).to(DEV)
    return u8(x1), u8(x2)


def _msf(path, name):
    with open(os.path.join(path, name + ".msf"), "rb") as f:
        return f.read()


def _random_pictures(P, H, W, seed):
    rng = np.random.default_rng(seed)
    pics = rng.integers(0, 256, (P, H, W, 3), dtype=np.uint8)
    pics[:, H // 2] = 0                       # a row of 0 and a row of 255: the ends of the range
    pics[:, H // 2 + 1] = 255
    return pics


# ------------------------------------------------------------------------------------------ 1. prep kernel
@pytest.mark.parametrize("H,W", [(64, 64), (65, 127), (100, 150)])
def test_pairs_prep_planes_padding_and_patches(H, W):
    """Inside the picture: pair_prep's crop and float32(u8) / float32(255); outside: the replicated edge; patches: pair_prep's of the
    unpadded picture at (64, 64); picture p's results depend neither on P nor on its place in the stack."""
    ops = _ops()
    pics = _random_pictures(6, H, W, seed=H * 1000 + W)
    Hp, Wp = -(-H // 64) * 64, -(-W // 64) * 64
    stack6 = torch.from_numpy(pics).to(DEV)
    got6 = ops.pairs_prep(stack6)
    assert got6.planes.shape == (6, 3, Hp, Wp) and got6.patches.shape == (6, 1, 128, 128)
    assert got6.planes.dtype == torch.float32 and got6.patches.dtype == torch.float32
    want = pics.astype(np.float32).transpose(0, 3, 1, 2) / np.float32(255)
    want = np.pad(want, ((0, 0), (0, 0), (0, Hp - H), (0, Wp - W)), mode="edge")
    assert np.array_equal(got6.planes.cpu().numpy(), want)
    for p in range(6):
        crop, patch = ops.pair_prep(stack6[p], (0, 0), (H, W), 256, (64, 64), 128)
        assert torch.equal(got6.planes[p, :, :H, :W], crop), p
        assert torch.equal(got6.patches[p], patch), p
    order = [4, 1]
    got2 = ops.pairs_prep(stack6[order].contiguous())
    assert got2.planes.shape == (2, 3, Hp, Wp)
    for i, p in enumerate(order):
        assert torch.equal(got2.planes[i], got6.planes[p]) and torch.equal(got2.patches[i], got6.patches[p]), p
    # other paddings and patch positions go through the same two launches
    other = ops.pairs_prep(stack6[:2].contiguous(), pad_to=1, patch_xy=(0, 128))
    assert other.planes.shape == (2, 3, H, W) and np.array_equal(other.planes.cpu().numpy(), want[:2, :, :H, :W])
    assert torch.equal(other.patches[1], ops.pair_prep(stack6[1], (0, 0), (H, W), 256, (0, 128), 128)[1])


def test_kernel_argument_errors_are_reported():
    ops = _ops()
    pics = torch.zeros((2, 65, 70, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="error -1"):
        ops.pairs_prep(pics, patch_xy=(64, 129))              # homopatch + patch_y > homopic
    with pytest.raises(RuntimeError, match="error -1"):
        ops.pairs_prep(pics, homopic=128, patch_xy=(1, 0))
    with pytest.raises(RuntimeError, match="error -1"):
        ops.pairs_prep(pics[:, :, :0].contiguous())           # an empty extent
    with pytest.raises(RuntimeError):
        ops.pairs_prep(pics.cpu())
    with pytest.raises(RuntimeError):
        ops.pairs_prep(pics.float())
    x = torch.zeros((2, 3, 64, 128), device=DEV)
    for hw in ((65, 128), (64, 129), (0, 128), (64, 0)):
        with pytest.raises(RuntimeError, match="error -1"):
            ops.planes_to_u8(x, hw)
    with pytest.raises(RuntimeError):
        ops.planes_to_u8(x.cpu(), (64, 128))
    assert ops.planes_to_u8(x, (64, 128)).shape == (2, 64, 128, 3)


# ------------------------------------------------------------------------------------------ 2. output kernel
def test_planes_to_u8_against_the_float32_formula_and_as_inverse_of_the_prep():
    ops = _ops()
    k = np.arange(256, dtype=np.float32)
    exact = k / np.float32(255)
    ties = (k + np.float32(0.5)) / np.float32(255)
    special = np.array([-0.3, 1.7, np.inf, -np.inf, np.nan, -0.0, 1.0, np.nextafter(np.float32(1), np.float32(2))], dtype=np.float32)
    values = np.concatenate([exact, ties, np.nextafter(ties, np.float32(-1)), np.nextafter(ties, np.float32(2)), special])
    rng = np.random.default_rng(3)
    x = values[rng.integers(0, values.size, (2, 3, 128, 192))]
    at = np.arange(values.size)
    x[1, 2, at // 150, at % 150] = values                      # every value at least once inside the [:100, :150] window
    assert values.size < 100 * 150 and np.isnan(x[1, 2, :100, :150]).any()
    with np.errstate(invalid="ignore"):
        want = np.floor(np.clip(x, np.float32(0), np.float32(1)) * np.float32(255) + np.float32(0.5))
    assert want.dtype == np.float32
    want = np.where(np.isnan(x), 0, want).astype(np.uint8).transpose(0, 2, 3, 1)
    got = ops.planes_to_u8(torch.from_numpy(x).to(DEV), (100, 150))
    assert got.dtype == torch.uint8 and got.shape == (2, 100, 150, 3)
    assert np.array_equal(got.cpu().numpy(), want[:, :100, :150])
    assert np.array_equal(ops.planes_to_u8(torch.from_numpy(x).to(DEV), (128, 192)).cpu().numpy(), want)
    # every k / 255 comes back as k
    ramp = torch.from_numpy(np.tile(exact, 3 * 4).reshape(1, 3, 4, 256)).to(DEV)
    assert np.array_equal(ops.planes_to_u8(ramp, (4, 256)).cpu().numpy(), np.tile(np.arange(256, dtype=np.uint8)[None, None, :, None], (1, 4, 1, 3)))
    for H, W in ((100, 150), (65, 127), (3, 1030)):            # the last: two workgroups along a row
        pics = torch.from_numpy(_random_pictures(3, H, W, seed=H + W)).to(DEV)
        assert torch.equal(ops.planes_to_u8(ops.pairs_prep(pics).planes, (H, W)), pics), (H, W)
        assert torch.equal(ops.planes_to_u8(ops.pairs_prep(pics, pad_to=1).planes, (H, W)), pics), (H, W)


# ------------------------------------------------------------------------------------------ 3. round trip from the file alone
def _encoded(prec, tmp_path_factory):
    """One pair at 100 x 150 encoded in the operand mode `prec` (cached per module run): the model, the directory, encode's result."""
    from masic_amd import StereoCodec, nn as mnn
    if prec not in _CACHE:
        try:
            hsic = _hsic(32, 48, 3, 21, prec)
            left, right = _pictures(1, H0, W0, seed=31)
            path = str(tmp_path_factory.mktemp("msf_" + prec))
            with torch.no_grad():
                enc = StereoCodec(hsic, _udh()).encode(left, right, ["pair"], path)
            _CACHE[prec] = (hsic, path, enc, left, right)
        finally:
            mnn.set_precision("f32")
    return _CACHE[prec]


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_round_trip_with_nothing_but_the_file(tmp_path, tmp_path_factory, prec):
    from masic_amd import StereoCodec, nn as mnn, stereofile as SF
    ops = _ops()
    hsic, path, enc, left, right = _encoded(prec, tmp_path_factory)
    try:
        mnn.set_precision(prec)
        data = _msf(path, "pair")
        assert enc["bytes"] == [len(data)] and enc["bpp"] == [len(data) * 8.0 / (H0 * W0)]
        assert enc["left_hat"].shape == (1, H0, W0, 3) and enc["left_hat"].dtype == torch.uint8
        assert enc["x1_hat"].shape == (1, 3, 128, 192) and enc["delta_q"].dtype == torch.int16 and enc["delta_q"].shape == (1, 8)
        dec = StereoCodec(hsic).decode(["pair"], path)                     # no pictures, no h_matrix, no homography net
        assert torch.equal(dec["left"], enc["left_hat"]) and torch.equal(dec["right"], enc["right_hat"])
        assert torch.equal(dec["h_matrix"], enc["h_matrix"])
        assert torch.equal(dec["x1_hat"], enc["x1_hat"]) and torch.equal(dec["x2_hat"], enc["x2_hat"])
        one = StereoCodec(hsic).decode("pair", path)                       # one name as a string
        assert torch.equal(one["left"], dec["left"]) and torch.equal(one["right"], dec["right"])

        # the homography: the synthetic net's offsets are not multiples of 1/64 (else the comparison below shows nothing), the file
        # carries their quantised form, and both sides use the matrix of the DEQUANTISED offsets
        planes, patches = ops.pairs_prep(torch.cat((left, right)))
        delta = _udh()(patches[:1], patches[1:])
        d = delta.reshape(8).cpu().numpy()
        print("udh offsets:", d)
        assert np.abs(d).max() < 500 and (np.rint(d * np.float32(64)) != d * np.float32(64)).any()
        f = SF.parse(data, "test")
        assert (f.H0, f.W0) == (H0, W0)
        assert np.array_equal(f.delta_q, SF.quantise(d)) and np.array_equal(enc["delta_q"].numpy().reshape(8), f.delta_q)
        corners = torch.tensor([[[0., 0.], [128., 0.], [128., 128.], [0., 128.]]], device=DEV)
        dq = torch.from_numpy(SF.dequantise(f.delta_q).reshape(1, 4, 2)).to(DEV)
        assert torch.equal(enc["h_matrix"], ops.homography_from_corners(corners, dq, (H0, W0), (256, 256)))
        assert not torch.equal(enc["h_matrix"], ops.homography_from_corners(corners, delta, (H0, W0), (256, 256)))

        # the sections are the two files compress writes for the padded planes, and the pictures are decompress's, cropped
        with torch.no_grad():
            ref = hsic.compress(planes[:1], planes[1:], enc["h_matrix"], "ref", str(tmp_path))
            out = hsic.decompress(None, None, enc["h_matrix"], "ref", str(tmp_path))
        npz, binf = (open(os.path.join(str(tmp_path), "ref" + ext), "rb").read() for ext in (".npz", ".bin"))
        assert f.header == npz and f.streams == binf and len(data) == 38 + len(npz) + len(binf)
        assert torch.equal(enc["x1_hat"], ref["x1_hat"]) and torch.equal(enc["x2_hat"], ref["x2_hat"])
        assert torch.equal(dec["left"], ops.planes_to_u8(out["x1_hat"], (H0, W0)))
        assert torch.equal(dec["right"], ops.planes_to_u8(out["x2_hat"], (H0, W0)))
    finally:
        mnn.set_precision("f32")


# ------------------------------------------------------------------------------------------ 4. batch
def test_batch_files_equal_single_files_and_sizes_must_agree(tmp_path):
    from masic_amd import StereoCodec, nn as mnn
    try:
        hsic = _hsic(32, 48, 3, 21, "bf16")
        sc = StereoCodec(hsic, _udh())
        left, right = _pictures(3, H0, W0, seed=41)
        names = ["a", "b", "c"]
        one, many = tmp_path / "one", tmp_path / "many"
        one.mkdir()
        many.mkdir()
        enc = sc.encode(left, right, names, str(many))
        singles = [sc.encode(left[i], right[i], n, str(one)) for i, n in enumerate(names)]          # [H0,W0,3] and one name
        for i, n in enumerate(names):
            assert _msf(str(many), n) == _msf(str(one), n), n
            for k in ("h_matrix", "delta_q", "left_hat", "right_hat", "x1_hat", "x2_hat"):
                assert torch.equal(enc[k][i:i + 1], singles[i][k]), (n, k)
            assert enc["bytes"][i] == singles[i]["bytes"][0] == len(_msf(str(many), n))
        assert len({_msf(str(many), n) for n in names}) == 3
        dec = StereoCodec(hsic).decode(names, str(many))
        assert torch.equal(dec["left"], enc["left_hat"]) and torch.equal(dec["right"], enc["right_hat"])
        for i, n in enumerate(names):
            d1 = StereoCodec(hsic).decode([n], str(many))
            for k in ("left", "right", "h_matrix", "x1_hat", "x2_hat"):
                assert torch.equal(dec[k][i:i + 1], d1[k]), (n, k)
        small = _pictures(1, 64, 64, seed=42)
        sc.encode(small[0], small[1], ["small"], str(many))
        with pytest.raises(ValueError, match=r"pair 1 \(small\) is 64x64"):
            StereoCodec(hsic).decode(["a", "small", "c"], str(many))
        # refusals of encode that name their cause
        with pytest.raises(ValueError, match="uint8"):
            sc.encode(left.float(), right.float(), names, str(many))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            sc.encode(left.cpu(), right.cpu(), names, str(many))
        with pytest.raises(ValueError, match="one shape"):
            sc.encode(left, right[:, :, :W0 - 1].contiguous(), names, str(many))
        with pytest.raises(ValueError, match="3 pairs and 2 names"):
            sc.encode(left, right, names[:2], str(many))
        with pytest.raises(ValueError, match="exceeds 65535"):
            sc.encode(left[:1, :1, :1].expand(1, 65500, 1, 3), right[:1, :1, :1].expand(1, 65500, 1, 3), ["tall"], str(many))
        _udh().train()
        try:
            with pytest.raises(RuntimeError, match="training mode"):
                sc.encode(left, right, names, str(many))
        finally:
            _udh().eval()
    finally:
        mnn.set_precision("f32")


# ------------------------------------------------------------------------------------------ 5. a decoder that never saw the pictures
@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_a_fresh_model_decodes_the_files(tmp_path_factory, prec):
    from masic_amd import StereoCodec, nn as mnn
    hsic, path, enc, _, _ = _encoded(prec, tmp_path_factory)
    try:
        mnn.set_precision(prec)
        dec = StereoCodec(_fresh_copy(hsic, 32, 48, 3)).decode(["pair"], path)
        assert torch.equal(dec["left"], enc["left_hat"]) and torch.equal(dec["right"], enc["right_hat"])
        assert torch.equal(dec["h_matrix"], enc["h_matrix"])
    finally:
        mnn.set_precision("f32")


def test_fp8_mode_file_decodes_into_a_fresh_uncalibrated_model(tmp_path):
    from masic_amd import StereoCodec, fp8, nn as mnn, synth
    N, M, K = 128, 192, 5
    try:
        hsic = _hsic(N, M, K, 23, "fp8")
        left, right = _pictures(1, 128, 192, seed=23)
        planes = _ops().pairs_prep(torch.cat((left, right))).planes
        fp8.calibrate(hsic, [(planes[:1], planes[1:], synth.synth_inputs(1, 128, 192, seed=23)[2].to(DEV))])
        enc = StereoCodec(hsic, _udh()).encode(left, right, ["q"], str(tmp_path))
        other = _fresh_copy(hsic, N, M, K)
        dec = StereoCodec(other).decode(["q"], str(tmp_path))
        assert torch.equal(dec["left"], enc["left_hat"]) and torch.equal(dec["right"], enc["right_hat"])
        assert not fp8.export_scales(other)                    # the scales came from the file and did not stay in the model
    finally:
        mnn.set_precision("f32")


# ------------------------------------------------------------------------------------------ 6. enhancement
def test_enhancement_is_the_cqe_network_on_the_decoded_planes(tmp_path_factory):
    import MASIC
    from masic_amd import StereoCodec, nn as mnn
    ops = _ops()
    hsic, path, enc, _, _ = _encoded("bf16", tmp_path_factory)
    try:
        mnn.set_precision("bf16")
        torch.manual_seed(5)
        cqe = MASIC.Independent_EN().to(DEV).eval()
        sc = StereoCodec(hsic, cqe=cqe)
        plain = sc.decode(["pair"], path)
        better = sc.decode(["pair"], path, enhance=True)
        with torch.no_grad():
            want = cqe(plain["x1_hat"], plain["x2_hat"], plain["h_matrix"])
        assert torch.equal(better["x1_hat"], want["x1_hat"]) and torch.equal(better["x2_hat"], want["x2_hat"])
        assert torch.equal(better["left"], ops.planes_to_u8(want["x1_hat"], (H0, W0)))
        assert torch.equal(better["right"], ops.planes_to_u8(want["x2_hat"], (H0, W0)))
        assert not torch.equal(better["left"], plain["left"])
        assert torch.equal(plain["left"], enc["left_hat"])
        with pytest.raises(RuntimeError, match="cqe=None"):
            StereoCodec(hsic).decode(["pair"], path, enhance=True)
        cqe.train()
        with pytest.raises(RuntimeError, match="training mode"):
            sc.decode(["pair"], path, enhance=True)
    finally:
        mnn.set_precision("f32")


# ------------------------------------------------------------------------------------------ 7. damage on the device path
def test_a_flipped_stream_bit_and_another_operand_mode_are_refused(tmp_path, tmp_path_factory):
    """The flipped bit sits where tests/test_gpu_codec_verify.py places it: the lowest clear bit of the last word of the longest view-2
    channel stream.  The device check catches it either at the end (the coder misses its final state) or earlier (the damaged coder
    runs out of words); decode reports both as CorruptStreamError."""
    from masic_amd import StereoCodec, codec, nn as mnn, stereofile as SF
    hsic, path, enc, _, _ = _encoded("bf16", tmp_path_factory)
    try:
        mnn.set_precision("bf16")
        data = _msf(path, "pair")
        f = SF.parse(data, "test")
        raw = f.streams
        assert raw[:4] == b"MSR2" and not raw[5] & 1
        off = 8
        for view in range(2):
            n = int(np.frombuffer(raw[off:off + 4], dtype=np.uint32)[0])
            lengths = np.frombuffer(raw[off + 4:off + 4 + 4 * n], dtype=np.uint32).astype(np.int64)
            starts = off + 4 + 4 * n + np.concatenate([[0], np.cumsum(lengths)[:-1]])
            off = int(off + 4 + 4 * n + lengths.sum())
        assert off == len(raw) and n > 0
        j = int(np.argmax(lengths))
        assert lengths[j] > 8                                               # its last word is a renormalisation word
        word_at = 38 + len(f.header) + int(starts[j] + lengths[j]) - 4
        word = int(np.frombuffer(data[word_at:word_at + 4], dtype=np.uint32)[0])
        assert word != 0xffffffff
        bad = bytearray(data)
        bit = next(b for b in range(32) if not (word >> b) & 1)
        bad[word_at + bit // 8] ^= 1 << (bit % 8)
        with open(os.path.join(str(tmp_path), "bad.msf"), "wb") as g:
            g.write(bytes(bad))
        with pytest.raises(codec.CorruptStreamError) as ei:
            StereoCodec(hsic).decode(["bad"], str(tmp_path))
        print("flipped stream bit:", ei.value)
        assert ei.value.pair == 0 and ("final state" in str(ei.value) or "ended before its last symbol" in str(ei.value))
        mnn.set_precision("f32")
        with pytest.raises(ValueError, match="written in the bf16 operand mode"):
            StereoCodec(hsic).decode(["pair"], path)
    finally:
        mnn.set_precision("f32")


# ------------------------------------------------------------------------------------------ 8. capture
def test_both_kernels_capture_into_a_graph_on_a_side_stream():
    ops = _ops()
    a = torch.from_numpy(_random_pictures(4, 65, 127, seed=1)).to(DEV)
    b = torch.from_numpy(_random_pictures(4, 65, 127, seed=2)).to(DEV)
    static = a.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.planes_to_u8(ops.pairs_prep(static).planes, (65, 127))          # allocator warm before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        prep = ops.pairs_prep(static)
        back = ops.planes_to_u8(prep.planes, (65, 127))
    for pics in (a, b, a):
        static.copy_(pics)
        g.replay()
        torch.cuda.synchronize()
        eager = ops.pairs_prep(pics)
        assert torch.equal(prep.planes, eager.planes) and torch.equal(prep.patches, eager.patches)
        assert torch.equal(back, pics)
