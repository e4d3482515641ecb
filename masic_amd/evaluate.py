"""Test-split evaluation: where a checkpoint lies on the rate-distortion plane.

The reference's evaluators (coremasic/mywork/test2_real.py:172-252, test3_real.py:141-232) run one pair at a time and average per-pair
values.  The mean of per-pair PSNRs is not the PSNR of the mean MSE, so a batched evaluation needs per-pair sums: masic_amd.metrics.

    pair_metrics(out_net, d1, d2)            per-pair mse and bpp of one forward output, float64 [B] device tensors, one kernel call
    evaluate_folder(hsic, homo, root, ...)   ESTIMATE mode: HSIC.forward (then the enhancement net) over a folder's split, rate from
                                             the likelihoods, distortion from the float reconstructions
    evaluate_files(codec, root, ...)         FILES mode: StereoCodec.encode / decode of whole pictures, rate from the .msf files' sizes,
                                             distortion from the decoded 8-bit pictures
    Report                                   names, per-pair table, means, the reference's one-line summary, JSON

Every pair of the split is taken once, in file order; the last batch may be short and no pair is dropped.  Modules in training mode are
put into eval mode for the run and every module's flag is set back afterwards, also when the run raises; masic_amd.nn's precision is
read, never set.  Refusals (an unknown metric, "lpips" without lpips_fn, pictures too small for MS-SSIM, modules on the CPU, a missing
split directory) happen before the first launch.  No CPU path.
"""
import contextlib
import json
import math
import os
import tempfile

import numpy as np

METRICS = ("psnr", "ms_ssim", "lpips")
MS_SSIM_MIN_SIDE = 176            # five levels of an 11-tap window: 11 * 2^4
LIK_KEYS = ("y1", "y2", "z1", "z2")          # the order HSIC.forward lists them in and loss.rate_distortion adds them in
PSNR_CAP_DB = 100.0               # files mode: the PSNR of two pictures whose mse is below 1e-10 (test3_real.py:69-74)


# ------------------------------------------------------------------------------------------ the report
def psnr_from_mse(mse):
    """10 log10(1 / mse) of float planes in [0, 1] (test2_real.py:67-70), elementwise in float64; mse = 0 gives inf"""
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(1.0 / np.asarray(mse, dtype=np.float64))


def psnr_from_mse_u8(mse):
    """20 log10(1 / sqrt(mse)) of 8-bit pictures, mse of the bytes over 255^2; 100 dB where mse < 1e-10 (test3_real.py:69-74)"""
    mse = np.asarray(mse, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return np.where(mse < 1.0e-10, PSNR_CAP_DB, 20.0 * np.log10(1.0 / np.sqrt(np.where(mse < 1.0e-10, 1.0, mse))))


class Report:
    """The per-pair table of one evaluation and what is derived from it.

    names: the left pictures' basenames, in file order; pairs: {metric: float64 array of n}; mean: {metric: float}, the float64 mean
    over the pairs in that order; mode: "estimate" or "files"; n; roundtrip_exact: files mode without enhancement only, else None.

    Built from the measured columns -- mse1, mse2, and what of bpp*, ms_ssim1/2, lpips1/2 was measured --; the rest is derived here:
    psnr1 / psnr2 from the mse columns (psnr_from_mse, in files mode psnr_from_mse_u8), and psnr, ms_ssim, lpips as the mean of the two
    views per pair."""

    def __init__(self, names, pairs, mode, roundtrip_exact=None):
        if mode not in ("estimate", "files"):
            raise ValueError(f"Report: mode {mode!r} is neither 'estimate' nor 'files'")
        self.names = [str(n) for n in names]
        self.mode, self.n, self.roundtrip_exact = mode, len(self.names), roundtrip_exact
        self.pairs = {k: np.asarray(v, dtype=np.float64).reshape(-1) for k, v in pairs.items()}
        for k, v in self.pairs.items():
            if len(v) != self.n:
                raise ValueError(f"Report: column {k!r} holds {len(v)} values for {self.n} pairs")
        if self.n < 1:
            raise ValueError("Report: no pairs")
        p = self.pairs
        to_psnr = psnr_from_mse_u8 if mode == "files" else psnr_from_mse
        for v in ("1", "2"):
            if "mse" + v in p and "psnr" + v not in p:
                p["psnr" + v] = to_psnr(p["mse" + v])
        for k in ("psnr", "ms_ssim", "lpips"):
            if k + "1" in p and k + "2" in p and k not in p:
                p[k] = (p[k + "1"] + p[k + "2"]) / 2
        self.mean = {k: float(np.mean(v)) for k, v in p.items()}

    def fields(self):
        """[(label, value, format)] of line(), in its order"""
        m, files = self.mean, self.mode == "files"
        out = [("PSNR (dB)", (m["psnr1"] + m["psnr2"]) / 2, ".3f")]
        if "bpp" in m:
            # per view: the reference divides the pair's bits per pixel by two (test2_real.py:238, test3_real.py:220)
            out.append(("BPP", m["bpp"] / 2, ".3f") if files else ("Bpp loss", m["bpp"] / 2, ".4f"))
        for key, label in (("ms_ssim", "MS-SSIM"), ("lpips", "LPIPS")):
            if key in m:
                out += [(label + v, m[key + v], ".4f") for v in ("", "1", "2")]
        out += [("PSNR1", m["psnr1"], ".3f"), ("PSNR2", m["psnr2"], ".3f")]
        if not files and "bpp1" in m and "bpp2" in m:
            out += [("BPP1", m["bpp1"], ".3f"), ("BPP2", m["bpp2"], ".3f")]          # a .msf file has no per-view byte split
        return out

    def line(self, epoch=0):
        """The one-line summary: 'Test epoch <epoch>:' and then fields 'Label: value' separated by '|'.  The first field counts the
        pairs (the reference's has the time there, and its table script drops the first field); PSNR (dB) is the mean of the two
        views, Bpp loss / BPP is per view."""
        parts = [f"Pairs: {self.n}"] + [f"{label}: {value:{fmt}}" for label, value, fmt in self.fields()]
        return f"Test epoch {epoch}: " + " |\t".join(parts)

    def to_json(self):
        return json.dumps({"mode": self.mode, "n": self.n, "names": self.names, "roundtrip_exact": self.roundtrip_exact,
                           "mean": self.mean, "pairs": {k: [float(x) for x in v] for k, v in self.pairs.items()}})

    @classmethod
    def from_json(cls, text):
        d = json.loads(text)
        return cls(d["names"], d["pairs"], d["mode"], d.get("roundtrip_exact"))


# ------------------------------------------------------------------------------------------ checks
def _check_metrics(metrics, lpips_fn, who):
    if isinstance(metrics, str):
        metrics = (metrics,)
    metrics = tuple(metrics)
    for m in metrics:
        if m not in METRICS:
            raise ValueError(f"{who}: unknown metric {m!r}; the metrics are {', '.join(METRICS)}")
    if "lpips" in metrics and lpips_fn is None:
        raise ValueError(f"{who}: 'lpips' needs lpips_fn (an lpips.LPIPS module with weights of yours: none ship, none are fetched)")
    return metrics


def _check_batch_size(batch_size, who):
    if isinstance(batch_size, bool) or not isinstance(batch_size, int) or batch_size < 1:
        raise ValueError(f"{who}: batch_size must be a positive integer, got {batch_size!r}")
    return batch_size


def _device_of(module, who, name):
    import torch
    p = next(iter(module.parameters()), None) if isinstance(module, torch.nn.Module) else None
    if p is not None and p.device.type != "cuda":
        raise RuntimeError(f"{who}: the {name} module must live on a CUDA (HIP) device -- the MI355X path has no CPU fallback")
    return None if p is None else p.device


def _check_ms_ssim(metrics, hw, what, who):
    if "ms_ssim" in metrics and min(hw) < MS_SSIM_MIN_SIDE:
        raise ValueError(f"{who}: 'ms_ssim' needs pictures of at least {MS_SSIM_MIN_SIDE} x {MS_SSIM_MIN_SIDE} (five levels of an 11-tap "
                         f"window), {what} is {hw[0]} x {hw[1]}")


@contextlib.contextmanager
def _eval_mode(*modules):
    """Every given torch module in eval mode; each submodule's training flag is set back on the way out"""
    import torch
    seen = {}
    for mod in modules:
        if isinstance(mod, torch.nn.Module):
            for m in mod.modules():
                seen.setdefault(id(m), (m, m.training))
    try:
        for mod in modules:
            if isinstance(mod, torch.nn.Module):
                mod.eval()
        yield
    finally:
        for m, flag in seen.values():
            m.training = flag


# ------------------------------------------------------------------------------------------ per-pair values on the device
def pair_metrics(out_net, d1, d2):
    """Per-pair rate and distortion of one forward output: {name: float64 [B] device tensor}.

    mse1, mse2: sum (x_hat - x)^2 / (3 H W) of each view.  With out_net["likelihoods"] (keys y1, y2, z1, z2) also bpp_y1, bpp_y2,
    bpp_z1, bpp_z2 = sum log lik / (-ln 2 H W), bpp1 = y1 + z1, bpp2 = y2 + z2, bpp = ((y1 + y2) + z1) + z2.  Entry b of each is
    what loss.rate_distortion returns for the one-pair slices [b:b+1], bit for bit.  One metrics.pair_rd call; nothing waits for the
    device."""
    from . import metrics
    liks = out_net.get("likelihoods")
    if liks is not None and tuple(liks.keys()) != LIK_KEYS:
        raise ValueError(f"masic_amd.evaluate.pair_metrics: likelihoods {tuple(liks.keys())}, expected {LIK_KEYS}")
    if getattr(d1, "dim", lambda: 0)() != 4:
        raise ValueError("masic_amd.evaluate.pair_metrics: d1, d2 must be [B,3,H,W] pictures")
    H, W = d1.shape[-2:]
    tensors = [] if liks is None else [liks[k].contiguous() for k in LIK_KEYS]
    s = metrics.pair_rd(out_net["x1_hat"].contiguous(), d1.contiguous(), out_net["x2_hat"].contiguous(), d2.contiguous(), tensors)
    n_pic = d1.numel() // d1.shape[0]
    out = {"mse1": s[:, 0] / n_pic, "mse2": s[:, 1] / n_pic}
    if liks is not None:
        per = {k: s[:, 2 + i] / (-math.log(2) * (H * W)) for i, k in enumerate(LIK_KEYS)}
        out.update({"bpp_" + k: v for k, v in per.items()})
        out["bpp1"], out["bpp2"] = per["y1"] + per["z1"], per["y2"] + per["z2"]
        out["bpp"] = sum(per.values())
    return out


def _quality(x1_hat, x1, x2_hat, x2, metrics, lpips_fn):
    """ms_ssim1/2 and lpips1/2 of float planes in [0, 1], float64 [B] device tensors"""
    out = {}
    if "ms_ssim" in metrics:
        from pytorch_msssim import ms_ssim
        out["ms_ssim1"] = ms_ssim(x1_hat, x1, data_range=1, size_average=False).double()
        out["ms_ssim2"] = ms_ssim(x2_hat, x2, data_range=1, size_average=False).double()
    if "lpips" in metrics:
        out["lpips1"] = lpips_fn(x1, x1_hat).reshape(x1.shape[0]).double()
        out["lpips2"] = lpips_fn(x2, x2_hat).reshape(x2.shape[0]).double()
    return out


def _read_back(columns):
    """[{name: float64 [b] device tensor}] per batch -> {name: float64 numpy [N]} with one copy to the host"""
    import torch
    keys = list(columns[0])
    table = torch.stack([torch.cat([c[k] for c in columns]) for k in keys]).cpu().numpy()
    return {k: table[i].copy() for i, k in enumerate(keys)}


# ------------------------------------------------------------------------------------------ estimate mode
def evaluate_folder(hsic, homo, root, split="test", patch_size=(256, 256), batch_size=8, cqe=None, metrics=("psnr", "ms_ssim"),
                    lpips_fn=None, seed=0, root_add=""):
    """ESTIMATE mode -> Report.  hsic: MASIC.HSIC; homo: model.Net or align.PatchAligner (what StereoBatch.h_matrix takes); cqe:
    MASIC.Independent_EN or None.  Per batch of a DeviceStereoFolder(root, split, patch_size, seed=seed): h_matrix, the eval-mode
    HSIC.forward under no_grad, then cqe(x1_hat, x2_hat, h_matrix) when given.  Rate comes from the codec's likelihoods; distortion,
    MS-SSIM (pytorch_msssim.ms_ssim, data_range=1) and LPIPS (lpips_fn(x, x_hat), only when given) from the final reconstructions
    against the originals.  Per-pair values stay on the device and are read back once, after the last batch."""
    import torch
    from . import data
    who = "masic_amd.evaluate.evaluate_folder"
    metrics = _check_metrics(metrics, lpips_fn, who)
    batch_size = _check_batch_size(batch_size, who)
    dev = _device_of(hsic, who, "hsic")
    for name, m in (("homo", homo), ("cqe", cqe), ("lpips_fn", lpips_fn)):
        _device_of(m, who, name)
    if dev is None:
        raise RuntimeError(f"{who}: hsic has no parameters to take the device from")
    pairs = data.scan_pairs(root, split, root_add)
    if not pairs:
        raise ValueError(f"{who}: no stereo pairs under {os.path.join(str(root), split)}")
    first = data._picture_hw(pairs[0][0])
    _check_ms_ssim(metrics, data.effective_crop(first, patch_size), f"the crop of {os.path.basename(pairs[0][0])}", who)
    ds = data.DeviceStereoFolder(root, split, patch_size, root_add=root_add, seed=seed, device=dev)
    columns = []
    with _eval_mode(hsic, homo, cqe, lpips_fn), torch.no_grad(), torch.cuda.device(dev):
        for b in ds.batches(batch_size, shuffle=False, drop_last=False):
            h_matrix = b.h_matrix(homo)
            out = hsic(b.d1, b.d2, h_matrix)
            if cqe is not None:
                en = cqe(out["x1_hat"], out["x2_hat"], h_matrix)
                out = {"x1_hat": en["x1_hat"], "x2_hat": en["x2_hat"], "likelihoods": out["likelihoods"]}
            col = pair_metrics(out, b.d1, b.d2)
            col.update(_quality(out["x1_hat"], b.d1, out["x2_hat"], b.d2, metrics, lpips_fn))
            columns.append(col)
        table = _read_back(columns)
    return Report(ds.names, table, "estimate")


# ------------------------------------------------------------------------------------------ files mode
def _groups(sizes, batch_size):
    """Consecutive pairs of one picture size, at most batch_size of them: [(first, last + 1)]"""
    out, i = [], 0
    while i < len(sizes):
        j = i + 1
        while j < len(sizes) and j - i < batch_size and sizes[j] == sizes[i]:
            j += 1
        out.append((i, j))
        i = j
    return out


def evaluate_files(codec, root, split="test", batch_size=8, enhance=False, metrics=("psnr", "ms_ssim"), lpips_fn=None, out_dir=None):
    """FILES mode -> Report.  codec: a masic_amd.StereoCodec with its homography net (and cqe for enhance=True).  Whole pictures of any
    size (data.decode_rgb8); consecutive pairs of one size share a call, up to batch_size pairs.  Each call runs StereoCodec.encode
    into out_dir (a temporary directory by default; the files are named <left picture's basename>.msf) and StereoCodec.decode from the
    files alone.  bpp = 8 * (size of the .msf) / (H0 W0), for the pair; mse = u8_sse(decoded, original) / (3 H0 W0 255^2) per view,
    PSNR by psnr_from_mse_u8; MS-SSIM / LPIPS on the u8 / 255 float planes of the unpadded pictures.  Without enhance the decoded
    pictures must equal encode's left_hat / right_hat (RuntimeError otherwise; Report.roundtrip_exact)."""
    import torch
    from . import data, metrics as M
    who = "masic_amd.evaluate.evaluate_files"
    metrics = _check_metrics(metrics, lpips_fn, who)
    batch_size = _check_batch_size(batch_size, who)
    if codec.udh is None:
        raise RuntimeError(f"{who}: the codec was built without the homography net (udh=None): it cannot encode")
    if enhance and codec.cqe is None:
        raise RuntimeError(f"{who}: enhance=True needs the enhancement network, and the codec was built with cqe=None")
    dev = _device_of(codec.hsic, who, "hsic")
    for name, m in (("udh", codec.udh), ("cqe", codec.cqe), ("lpips_fn", lpips_fn)):
        _device_of(m, who, name)
    if dev is None:
        raise RuntimeError(f"{who}: hsic has no parameters to take the device from")
    pairs = data.scan_pairs(root, split)
    if not pairs:
        raise ValueError(f"{who}: no stereo pairs under {os.path.join(str(root), split)}")
    names = [os.path.basename(a) for a, _ in pairs]
    sizes = [data._picture_hw(a) for a, _ in pairs]
    for (a, b), hw in zip(pairs, sizes):
        if data._picture_hw(b) != hw:
            raise ValueError(f"{who}: {a} and {b} differ in size: the views of a pair must have one shape")
        _check_ms_ssim(metrics, hw, os.path.basename(a), who)
    columns, exact = [], (None if enhance else True)
    with contextlib.ExitStack() as stack:
        if out_dir is None:
            out_dir = stack.enter_context(tempfile.TemporaryDirectory(prefix="masic_eval_"))
        else:
            os.makedirs(out_dir, exist_ok=True)
        stack.enter_context(_eval_mode(codec.hsic, codec.udh, codec.cqe, lpips_fn))
        stack.enter_context(torch.no_grad())
        stack.enter_context(torch.cuda.device(dev))
        for i, j in _groups(sizes, batch_size):
            H0, W0 = sizes[i]
            left = torch.from_numpy(np.stack([data.decode_rgb8(a) for a, _ in pairs[i:j]])).to(dev)
            right = torch.from_numpy(np.stack([data.decode_rgb8(b) for _, b in pairs[i:j]])).to(dev)
            enc = codec.encode(left, right, names[i:j], out_dir)
            dec = codec.decode(names[i:j], out_dir, enhance=enhance)
            if not enhance and not (torch.equal(dec["left"], enc["left_hat"]) and torch.equal(dec["right"], enc["right_hat"])):
                raise RuntimeError(f"{who}: pairs {names[i]} .. {names[j - 1]}: the pictures decoded from the files differ from the "
                                   "encoder's reconstruction")
            nbytes = [os.path.getsize(os.path.join(out_dir, n + ".msf")) for n in names[i:j]]
            sse = M.u8_sse(torch.cat((dec["left"], dec["right"])), torch.cat((left, right))).double()       # exact below 2^53
            col = {"bytes": torch.tensor(nbytes, dtype=torch.float64).to(dev, non_blocking=True),
                   "pixels": torch.full((j - i,), float(H0 * W0), dtype=torch.float64, device=dev),
                   "sse1": sse[:j - i], "sse2": sse[j - i:]}
            if "ms_ssim" in metrics or "lpips" in metrics:
                planes = lambda u8: (u8.permute(0, 3, 1, 2).float() / 255).contiguous()
                col.update(_quality(planes(dec["left"]), planes(left), planes(dec["right"]), planes(right), metrics, lpips_fn))
            columns.append(col)
        table = _read_back(columns)
    pixels = table.pop("pixels")
    table["bpp"] = 8 * table["bytes"] / pixels
    for v in ("1", "2"):
        table["mse" + v] = table.pop("sse" + v) / (3 * pixels * 255 ** 2)
    return Report(names, table, "files", roundtrip_exact=exact)
